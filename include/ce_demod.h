/*
 * ce_demod.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: a max-log LLR soft demapper with the
 * PUSCH descrambling of TS 38.211 6.3.1.1 undone, the consumer of ce_eq_equalize's `x_hat` and `nvar`.
 *
 * The reference (pjookim/srsran-ce-pytorch) stops at the channel estimate.  The operator is pinned by the float64
 * restatement in tests/demod_oracle.py (a brute-force minimum over all 2^Qm constellation points) and the tolerance
 * rule stated there.
 *
 * Inputs, per slot: x_hat, complex64, dense, M = n_symbols symbols (M = n_data_re * L from the equalizer, layer
 * fastest); nvar, float32, the same shape (the complex noise variance of each symbol, 1 / SINR).
 * Modulation order Qm in {2, 4, 6, 8}: QPSK, 16QAM, 64QAM, 256QAM with the Gray maps of TS 38.211 5.1.3 - 5.1.6, e.g.
 *     16QAM   d = ((1 - 2 b0)(2 - (1 - 2 b2)) + j (1 - 2 b1)(2 - (1 - 2 b3))) / sqrt(10)
 * pi/2-BPSK and UCI placeholder bits are out of scope; transform precoding is undone before this stage (ce_tp.h).
 *
 * LLR of bit j of symbol i (y = x_hat_i, the minima over the constellation points s with that bit value):
 *     llr(i Qm + j) = (min_{s: b_j(s) = 1} |y - s|^2  -  min_{s: b_j(s) = 0} |y - s|^2) / nvar_i
 * exact max-log, positive when bit 0 is likelier; nvar is the complex noise variance, so there is no factor 2.  The maps
 * are separable (even bits: real axis, odd bits: imaginary axis, m = Qm / 2 bits each), so the kernel never searches:
 * with A = 1 / sqrt(2, 10, 42, 170) and, per axis, v_0 = y_axis / A, v_k = 2^(m-k) - |v_{k-1}|,
 *     bit k of the axis:  f = sign(v_k) (s + 1) (2 |v_k| + 1 - s),  s = min(2 floor(|v_k| / 2) + 1, 2^(m-k) - 1)
 *     llr = f * (A^2 / nvar_i)
 * in float32 (s is the nearest level of the folded axis; f is the piecewise-linear closed form of the difference of the
 * two squared distances in units of A^2).
 *
 * Erasures: all Qm LLRs of symbol i are 0 where nvar_i is not both finite and > 0, or where either part of x_hat_i is
 * not finite -- this covers the equalizer's "no usable channel" convention (x_hat = 0, nvar = +inf).  |x_hat| above
 * 2^60 and a noise variance below the smallest normal float32 are outside the operator's range.
 *
 * Descrambling (plan flag): llr'(n) = (1 - 2 c(n)) llr(n), n = 0 .. G - 1, G = M Qm; c is the Gold sequence of 38.211
 * 5.2.1 with c_init = (n_RNTI 2^15 + n_ID) mod 2^31 in unsigned 32-bit arithmetic.
 *
 * Output [slot][G], dense, in the format chosen at plan creation:
 *     CE_DEMOD_OUT_F32   float32, the LLR as computed
 *     CE_DEMOD_OUT_I8    int8, clamp(round(llr * llr_scale), -127, 127), round = to nearest, ties to even
 */
#ifndef CE_DEMOD_H
#define CE_DEMOD_H

#include "ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_DEMOD_MAX_BITS 2097152 /* 2^21 >= G: 273 PRB x 13 symbols x 4 layers x 256QAM = 1 362 816 */
#define CE_DEMOD_BLOCK_WORDS 8    /* 32-bit words of c per Gold block: one jump entry set per 256 bits */
#define CE_DEMOD_TILE_SYMBOLS 1024 /* symbols one workgroup handles: 32 Qm words of c = 4 Qm whole blocks */

#define CE_DEMOD_OUT_F32 0
#define CE_DEMOD_OUT_I8 1

typedef struct ce_demod_desc {
  int32_t abi_version; /* = CE_ABI_VERSION */
  int32_t device;      /* HIP device ordinal the plan lives on */
  int32_t qm;          /* 2, 4, 6 or 8 */
  int32_t out_format;  /* CE_DEMOD_OUT_F32 or CE_DEMOD_OUT_I8 */
  int32_t descramble;  /* 0 or 1 */
  int32_t n_symbols;   /* M >= 1 symbols per slot; M * qm <= CE_DEMOD_MAX_BITS */
  float llr_scale;     /* int8 format: positive and finite (ignored for float32) */
} ce_demod_desc;

typedef struct ce_demod_plan ce_demod_plan; /* opaque: the Gold tables on the device */

typedef struct ce_demod_info {
  int32_t n_bits;         /* G = n_symbols * qm: LLRs per slot */
  int32_t out_elem_bytes; /* 4 or 1 */
  int64_t bytes_per_slot; /* n_symbols * 12 + G * out_elem_bytes */
} ce_demod_info;

/* What ce_demod_plan_create derives on the host.  Bit n of c sits in bit n % 32 of word n / 32; c = x1 ^ x2 and x2 is
 * linear over GF(2) in c_init.  Word w = CE_DEMOD_BLOCK_WORDS * blk + k of c is
 *     x1[w] ^ (the k-th word stepped from the 31-bit x2 state  XOR over the set bits i of c_init of jump[blk][i]),
 * where jump[blk][i] holds x2(Nc + 32 CE_DEMOD_BLOCK_WORDS blk + j), j = 0 .. 30, for c_init = 1 << i (bit j = x2 at
 * offset j), and stepping is the recurrence x2(n + 31) = x2(n + 3) ^ x2(n + 2) ^ x2(n + 1) ^ x2(n).  Only a descrambling
 * plan holds tables (n_words = n_blocks = 0 otherwise). */
typedef struct ce_demod_host_view {
  int32_t n_bits;      /* G */
  int32_t n_words;     /* ceil(G / 32): x1 words kept */
  int32_t block_words; /* CE_DEMOD_BLOCK_WORDS */
  int32_t n_blocks;    /* ceil(n_words / block_words): jump entry sets kept */
  int32_t tile_symbols; /* CE_DEMOD_TILE_SYMBOLS */
  int32_t n_tiles;     /* workgroups per slot */
  int64_t table_bytes; /* bytes of the device tables: x1 padded to whole blocks + 32 rows x n_blocks of jump entries */
} ce_demod_host_view;

/* Validation and integer derivation of ce_demod_plan_create without touching a GPU: usable on a CPU-only host. */
int ce_demod_derive_host(const ce_demod_desc* desc, ce_demod_host_view* view);

/* Host only: the derived tables of a descrambling descriptor into caller buffers: x1[n_words], and
 * jump[n_blocks * 31] with the entry of block blk and c_init bit i at jump[blk * 31 + i]. */
int ce_demod_copy_tables(const ce_demod_desc* desc, uint32_t* x1, uint32_t* jump);

/* Validates the descriptor, derives the tables once and uploads them.  Synchronous; not for the per-slot loop. */
int ce_demod_plan_create(const ce_demod_desc* desc, ce_demod_plan** out);
void ce_demod_plan_destroy(ce_demod_plan* plan);
int ce_demod_plan_get_info(const ce_demod_plan* plan, ce_demod_info* info);

/*
 * Demaps n_slots slots in ONE launch on `stream` (a hipStream_t; NULL = the default stream).  Asynchronous;
 * n_slots == 0 launches nothing.
 *  x_hat      complex64 [slot][n_symbols], dense;  nvar  float32, the same shape
 *  rnti, n_id int32 device arrays; slot b reads element b * strides[0] / [1] of them (strides in elements, >= 0;
 *             0 = one value for the whole batch).  They enter only the unsigned 32-bit arithmetic of c_init: an
 *             out-of-range value gives the sequence of the wrapped c_init and cannot address memory.  Not read (may be
 *             NULL, as may `strides`) by a plan without descrambling.
 *  out        [slot][G] float32 or int8 as the plan says, dense
 * x_hat, nvar and out must be 16-byte aligned (CE_ERR_INVALID otherwise); a slot's row inside them need not be.  Every
 * address comes from the block index, the thread index and host-derived plan values.
 */
int ce_demod_demap(const ce_demod_plan* plan, const void* x_hat, const float* nvar, const int32_t* rnti,
                   const int32_t* n_id, const int64_t strides[2], int64_t n_slots, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_DEMOD_H */

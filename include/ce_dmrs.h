/*
 * ce_dmrs.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: PUSCH DM-RS generation on the GPU.
 *
 * The reference (pjookim/srsran-ce-pytorch) takes `pilots` as an input and has no generator, and no third-party test
 * vector ships with this repository: the operator is pinned by the bit-serial restatement of TS 38.211 in
 * tests/dmrs_oracle.py and by the anchors of tests/test_dmrs.py.  Its result is integer work plus one sign flip, so
 * every comparison is bit for bit.
 *
 * Operator, per slot b with parameters (slot, N_ID, n_SCID) and per DM-RS symbol `sym` of the slot:
 *     c_init = (2^17 (n_symb_slot * slot + sym + 1) (2 N_ID + 1) + 2 N_ID + n_SCID) mod 2^31    (38.211 6.4.1.1.1.1,
 *              Rel-15 form, transform precoding off), in unsigned 32-bit arithmetic
 *     c(n)   = x1(n + 1600) ^ x2(n + 1600), the length-31 Gold sequence of 38.211 5.2.1 with x2(0..30) = c_init
 *     r(m)   = a (1 - 2 c(2m)) + j a (1 - 2 c(2m + 1)),  a = float32 0x3f3504f3
 * Output [slot][n_re][n_dmrs_total][n_layers] complex64, dense -- the `pilots` layout of ce_estimate_batch:
 *     column s  hop 1's DM-RS symbols ascending, then hop 2's
 *     row k     the k-th set bit of kron(mask_prbs, re_mask[layer / 2]) of the column's hop (T:571-576); for a pilot
 *               in PRB q of the grid, ordinal j among the set bits of its PRB: m = ppp (grid_start_crb + q) + j,
 *               ppp = set bits per PRB (6: configuration type 1, 4: type 2)
 *     layer l   r(m) for even l, (-1)^m r(m) for odd l (w_f of the CDM group's second port; w_t = +1: ports 0-3)
 */
#ifndef CE_DMRS_H
#define CE_DMRS_H

#include "ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_DMRS_MAX_WORDS 136 /* 32-bit words of c one hop's pilots span: 2 ppp <= 12 bits per PRB, <= 4096 bits per grid,
                                 i.e. 128 words + 1 for an unaligned start (104 for 273 PRB), rounded up */
#define CE_DMRS_MAX_RE 2048   /* pilots per column: ppp * active PRBs <= 6 * 341 */

typedef struct ce_dmrs_hop_desc {
  uint8_t dmrs_symbols[CE_MAX_SYMBOLS]; /* 1 where the OFDM symbol carries DM-RS */
  uint16_t re_mask[CE_MAX_CDM];         /* standard masks only: type 1 0x555 / 0xAAA, type 2 0x0C3 / 0x30C / 0xC30 */
  const uint8_t* mask_prbs;             /* n_prb_grid bytes (0/1); host memory, read during create */
} ce_dmrs_hop_desc;

typedef struct ce_dmrs_desc {
  int32_t abi_version;    /* = CE_ABI_VERSION */
  int32_t device;         /* HIP device ordinal the plan lives on */
  int32_t n_prb_grid;     /* 12 * n_prb_grid <= CE_FFT_SIZE, as for ce_plan_desc */
  int32_t grid_start_crb; /* CRB of the grid's subcarrier 0 (>= 0); 6 (grid_start_crb + n_prb_grid) <= 2^20 */
  int32_t n_sym;          /* OFDM symbols in the grid (<= n_symb_slot) */
  int32_t n_symb_slot;    /* 14, or 12 (extended cyclic prefix) */
  int32_t n_layers;       /* 1..CE_MAX_LAYERS; layer l reads re_mask[l / 2] */
  int32_t n_hops;         /* 1 or 2; every hop has the same number of active PRBs */
  ce_dmrs_hop_desc hop[CE_MAX_HOPS];
} ce_dmrs_desc;

typedef struct ce_dmrs_plan ce_dmrs_plan; /* opaque: jump tables and pilot lists on the device */

typedef struct ce_dmrs_info {
  int32_t n_re;           /* pilots per column (= pilots.shape[1]) */
  int32_t n_dmrs_total;   /* columns over both hops (= pilots.shape[2]) */
  int64_t bytes_per_slot; /* n_re * n_dmrs_total * n_layers * 8 */
} ce_dmrs_info;

/* What ce_dmrs_plan_create derives on the host.  The generator is linear over GF(2) in c_init, so word w of c (bit n of
 * c in bit n % 32 of word n / 32) is  x1[w] ^ XOR over the set bits i of c_init of t[i][w];  only the words
 * word0 .. word0 + n_words - 1 that a hop's pilots touch are kept (index 0 = word0). */
typedef struct ce_dmrs_host_view {
  int32_t n_re, n_dmrs_total, ppp, reserved0;
  int32_t col_hop[CE_MAX_SYMBOLS];              /* per column: its hop ... */
  int32_t col_sym[CE_MAX_SYMBOLS];              /* ... and its OFDM symbol index in the slot */
  int32_t word0[CE_MAX_HOPS], n_words[CE_MAX_HOPS];
  uint32_t x1[CE_MAX_HOPS][CE_DMRS_MAX_WORDS];      /* words of c for c_init = 0 */
  uint32_t t[CE_MAX_HOPS][31][CE_DMRS_MAX_WORDS];   /* words of c for c_init = 1 << i, XORed with x1 */
  int32_t m[CE_MAX_HOPS][CE_DMRS_MAX_RE];       /* sequence index of row k (the same for every CDM column: the standard
                                                   masks of one type have ppp set bits per PRB each) */
  uint8_t odd_sign[CE_MAX_HOPS][CE_DMRS_MAX_RE]; /* 1: odd layers carry -r(m) in row k (m odd) */
} ce_dmrs_host_view;

/* Validation and integer derivation of ce_dmrs_plan_create without touching a GPU: usable on a CPU-only host. */
int ce_dmrs_derive_host(const ce_dmrs_desc* desc, ce_dmrs_host_view* view);

/* Validates the descriptor, derives the tables once and uploads them.  Synchronous; not for the per-slot loop. */
int ce_dmrs_plan_create(const ce_dmrs_desc* desc, ce_dmrs_plan** out);
void ce_dmrs_plan_destroy(ce_dmrs_plan* plan);
int ce_dmrs_plan_get_info(const ce_dmrs_plan* plan, ce_dmrs_info* info);

/*
 * Writes pilots_out[n_slots][n_re][n_dmrs_total][n_layers] (complex64, dense, on the plan's device) in ONE launch on
 * `stream` (a hipStream_t; NULL = the default stream).  Asynchronous; n_slots == 0 launches nothing.
 *  slot, n_id, n_scid   int32 device arrays; slot b reads element b * strides[0] / [1] / [2] of them (strides in
 *                       elements, >= 0; 0 = one value for the whole batch).  The kernel computes c_init from them in
 *                       unsigned 32-bit arithmetic and uses them for nothing else: an out-of-range value gives the
 *                       sequence of the wrapped c_init and cannot address memory.
 */
int ce_dmrs_generate(const ce_dmrs_plan* plan, const int32_t* slot, const int32_t* n_id, const int32_t* n_scid,
                     const int64_t strides[3], int64_t n_slots, void* pilots_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_DMRS_H */

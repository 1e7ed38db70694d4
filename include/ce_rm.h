/*
 * ce_rm.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: LDPC rate recovery with HARQ combining,
 * the consumer of ce_demod_demap's `llr[slot][G]` and the producer of the per-code-block soft buffers an LDPC decoder
 * reads.  All section numbers are TS 38.212.
 *
 * The reference (pjookim/srsran-ce-pytorch) stops at the channel estimate.  The operator is pinned by the literal
 * restatement of the specification's loops in tests/rm_oracle.py; results are compared by value, without a tolerance.
 *
 * Host derivation (ce_rm_derive_host, integers only; A = tbs, G = g_bits, L = n_layers, Qm = qm):
 *     B = A + 24 if A > 3824, else A + 16                                                   (5.1, 6.2.1)
 *     K_cb = 8448 (BG1) / 3840 (BG2);  B <= K_cb: C = 1, B' = B;  else C = ceil(B / (K_cb - 24)), B' = B + 24 C
 *     K' = B' / C;  K_b = 22 (BG1);  BG2: 10 if B > 640, 9 if B > 560, 8 if B > 192, else 6  (5.2.2)
 *     Zc = the smallest a 2^j (a in {2,3,5,7,9,11,13,15}, j >= 0, a 2^j <= 384) with K_b Zc >= K'
 *     K = 22 Zc / 10 Zc;  N = 66 Zc / 50 Zc;  N_cb = N, or min(N, n_ref) with limited-buffer rate matching
 *     fillers of the circular buffer: [f0, f1) = [K' - 2 Zc, K - 2 Zc)  (the first 2 Zc systematic bits are punctured
 *     and not part of the buffer);  P = N_cb - (f1 - f0), the non-filler positions of one turn
 *     q = G / (L Qm):  E_r = L Qm floor(q / C) for r <= C - (q mod C) - 1, else L Qm ceil(q / C)          (5.4.2.1)
 *     k0[rv] = floor(num[rv] N_cb / (den Zc)) Zc,  num = (0, 17, 33, 56), den = 66 (BG1) / (0, 13, 25, 43), 50 (BG2)
 *
 * Operator, per slot and code block r.  The block's LLRs f_0 .. f_{E_r - 1} start at element sum_{s<r} E_s of the
 * slot's row (5.5).  Deinterleaving (5.4.2.2): e_{i E_r/Qm + j} = f_{i + j Qm}.  Bit selection (5.4.2.1): e_k belongs
 * to buffer position n_k, the k-th non-filler position met walking (k0 + j) mod N_cb for j = 0, 1, ...
 *     out[slot][r][n], n = 0 .. N_cb - 1:
 *       at a filler position   +127 (int8) / filler_llr (float32), whatever harq_in holds there
 *       elsewhere              acc = harq_in[slot][r][n] (0 without harq_in);  acc += e_k for every k with n_k = n, in
 *                              ascending k
 * float32: each += is one IEEE addition in that order (reproducible bit for bit).  int8: the sum is taken in 32-bit
 * integers and clamped once to [-127, 127].  A position that no e_k reaches keeps harq_in (or 0).
 *
 * The kernel gathers over output positions: with rank(n) = n for n < f0, n - (f1 - f0) for n >= f1, and s = rank(k0)
 * (s = f0 where k0 lies in [f0, f1)), position n receives k = (rank(n) - s) mod P, then k + P, k + 2 P .. while
 * k < E_r; the source of k is element sum_{s<r} E_s + (k mod (E_r/Qm)) Qm + floor(k / (E_r/Qm)) of the slot's row.
 */
#ifndef CE_RM_H
#define CE_RM_H

#include "ce_demod.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_RM_F32 0
#define CE_RM_I8 1
#define CE_RM_MAX_SLOT_ELEMS 16777216 /* 2^24 >= C * N_cb: outputs per slot (the largest NR transport block: < 2^23) */
#define CE_RM_TILE_UNITS 1024         /* 4-byte units of the output one workgroup writes */

typedef struct ce_rm_desc {
  int32_t abi_version; /* = CE_ABI_VERSION */
  int32_t device;      /* HIP device ordinal the plan lives on */
  int32_t base_graph;  /* 1 or 2 (7.2.2 of 38.214 / 6.2.2 of 38.212: the caller's choice, stated explicitly) */
  int32_t tbs;         /* A >= 1: transport block size in bits */
  int32_t qm;          /* 2, 4, 6 or 8 */
  int32_t n_layers;    /* 1 .. 4 */
  int32_t g_bits;      /* G: LLRs in a slot's row; a multiple of n_layers * qm, <= CE_DEMOD_MAX_BITS */
  int32_t format;      /* CE_RM_F32 or CE_RM_I8: input, harq_in and output alike */
  int32_t n_ref;       /* 0: no limited-buffer rate matching; otherwise N_ref >= K - 2 Zc */
  float filler_llr;    /* float32 format: positive and finite (ignored for int8, whose fillers are +127) */
} ce_rm_desc;

typedef struct ce_rm_plan ce_rm_plan; /* opaque */

typedef struct ce_rm_info {
  int32_t n_code_blocks;  /* C */
  int32_t n_cb;           /* N_cb */
  int32_t elem_bytes;     /* 4 or 1 */
  int32_t reserved0;
  int64_t bytes_per_slot; /* (G + C * N_cb) * elem_bytes: LLRs in, buffers out; harq_in adds C * N_cb * elem_bytes */
} ce_rm_info;

/* What ce_rm_plan_create derives on the host: every value of the derivation above, and the launch geometry. */
typedef struct ce_rm_host_view {
  int32_t b;         /* B */
  int32_t k_cb;      /* K_cb */
  int32_t c;         /* C */
  int32_t b_prime;   /* B' */
  int32_t k_prime;   /* K' */
  int32_t k_b;       /* K_b */
  int32_t zc;        /* Zc */
  int32_t k;         /* K */
  int32_t n;         /* N */
  int32_t n_cb;      /* N_cb */
  int32_t f0, f1;    /* filler positions [f0, f1) of the circular buffer */
  int32_t p;         /* P */
  int32_t n_lo;      /* blocks r < n_lo have E_r = e_lo, the others e_hi */
  int32_t e_lo, e_hi;
  int32_t k0[4];     /* per rv */
  int32_t s[4];      /* per rv: rank(k0), or f0 where k0 is a filler position */
  int32_t unit_elems; /* output elements per 4-byte unit: 1 (float32) or 4 (int8) */
  int32_t tiles_per_block; /* workgroups per code block: CE_RM_TILE_UNITS units each */
  int32_t n_tiles;   /* workgroups per slot = C * tiles_per_block */
} ce_rm_host_view;

/* Validation and integer derivation of ce_rm_plan_create without touching a GPU: usable on a CPU-only host.
 * CE_ERR_INVALID: base graph, qm, layer count or format unsupported; A < 1; B mod C != 0; K' > K_b 384; G no multiple
 * of n_layers * qm; q < C; G > CE_DEMOD_MAX_BITS; n_ref neither 0 nor >= K - 2 Zc; filler_llr not positive and finite
 * (float32).  CE_ERR_UNSUPPORTED: C * N_cb > CE_RM_MAX_SLOT_ELEMS. */
int ce_rm_derive_host(const ce_rm_desc* desc, ce_rm_host_view* view);

/* Validates the descriptor and keeps the derived values; the plan holds no device memory. */
int ce_rm_plan_create(const ce_rm_desc* desc, ce_rm_plan** out);
void ce_rm_plan_destroy(ce_rm_plan* plan);
int ce_rm_plan_get_info(const ce_rm_plan* plan, ce_rm_info* info);

/*
 * Rate recovery of n_slots slots in ONE launch on `stream` (a hipStream_t; NULL = the default stream).  Asynchronous;
 * n_slots == 0 launches nothing.
 *  llr        [slot][G] float32 or int8 as the plan says, dense (ce_demod_demap's output); must not overlap `out`
 *  rv         int32 device array; slot b reads element b * rv_stride (in elements, >= 0; 0 = one value for the whole
 *             batch).  Only rv & 3 is used, so an out-of-range value cannot address memory.
 *  harq_in    [slot][C][N_cb], the buffer kept from the earlier transmissions, the plan's format; may be NULL (all zero)
 *             and may be `out` itself (the in-place update of a HARQ process): every output element is read and written
 *             by one thread only.  Any other overlap with `out` is undefined.
 *  out        [slot][C][N_cb], dense
 * llr, harq_in and out must be 16-byte aligned (CE_ERR_INVALID otherwise); the rows inside them need not be.  No
 * atomics, no zeroing pass, no scratch; every address comes from the block index, the thread index, host-derived plan
 * values and rv & 3.
 */
int ce_rm_recover(const ce_rm_plan* plan, const void* llr, const int32_t* rv, int64_t rv_stride, int64_t n_slots,
                  const void* harq_in, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_RM_H */

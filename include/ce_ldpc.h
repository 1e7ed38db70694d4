/*
 * ce_ldpc.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: a layered normalised min-sum decoder for
 * quasi-cyclic LDPC codes of the NR shape (TS 38.212 5.3.2) behind ce_rm_recover, one launch for all code blocks of a batch.
 *
 * The reference (pjookim/srsran-ce-pytorch) stops at the channel estimate.  The base-graph tables of TS 38.212 (Tables
 * 5.3.2-2 and 5.3.2-3) are NOT part of this library: the decoder takes the base graph as data in its descriptor (rows,
 * columns, circulant shifts), nothing in the kernel depends on which graph it is given, and it is tested on seeded
 * random graphs of the NR shape only (tests/ldpc_oracle.py `random_graph`).  No test against the real tables exists or is
 * claimed.  All arithmetic is integer; tests/ldpc_oracle.py restates it (`decode_ref`, `decode_loop`) and results are
 * compared by value, without a tolerance.
 *
 * Code: n_cols base columns of zc bits each, n_rows base rows, n_sys = n_cols - n_rows; edge e of base row r joins the
 * lifted check (r, z) to the variable (col_e, (z + shift_e) mod zc), z < zc (the right-shifted identity of 5.3.2).
 *
 * Channel values, for codeword index i = c zc + z:
 *     ch_i = 0                                     for i < n_punctured_cols zc
 *     ch_i = q(in[i - n_punctured_cols zc])        while that index is < n_in
 *     ch_i = 0                                     beyond
 * q of int8: the value itself, -128 taken as -127.  q of float32, in this order: v = llr * llr_scale (one float32
 * multiplication); NaN -> 0; v clamped to [-127, 127] (+-inf -> +-127); (int)rintf(v), half to even.  Positive means bit 0
 * (the demapper's convention and the rate recovery's +127 fillers).
 *
 * Operator.  State: L_i, starting at ch_i, and R_e[z], starting at 0, for each edge e and z < zc.  One iteration visits the
 * rows in descriptor order; row r does for every z, independently (var_e = col_e zc + (z + shift_e) mod zc):
 *     t_e  = L[var_e] - R_e[z]                       (32-bit)
 *     s_e  = t_e < 0          a_e = min(|t_e|, 127)
 *     min1 = smallest a_e,  min2 = second smallest (equal to min1 on a tie),  idx = an edge attaining min1
 *     sgn  = XOR of all s_e
 *     m_e  = (3 * (e == idx ? min2 : min1)) >> 2     (normalised min-sum, factor 3/4, <= 95)
 *     R_e[z]   = (sgn ^ s_e) ? -m_e : m_e
 *     L[var_e] = t_e + R_e[z]
 * Which edge is idx on a tie changes no value.  There is no saturation step: L_i = ch_i + sum of R over the variable's
 * edges holds at every point, so |L| <= 127 + 95 * 46 = CE_LDPC_L_BOUND = 4497 and L fits int16.
 * After each complete iteration h_i = L_i < 0, and the block's parity holds if every check of the plan's rows XORs to 0.
 * With early_stop a block whose parity holds stops there (its outputs are its state at that iteration); without it
 * exactly max_iters iterations run and the parity is evaluated once at the end.
 *
 * The caller may pass a prefix of the rows of a larger graph (with n_cols shrunk by the rows left out): that is how a high
 * code rate uses fewer layers.  Columns no row touches are allowed.
 */
#ifndef CE_LDPC_H
#define CE_LDPC_H

#include "ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_LDPC_MAX_ZC 384
#define CE_LDPC_MAX_ROWS 46
#define CE_LDPC_MAX_COLS 68
#define CE_LDPC_MAX_ROW_DEGREE 19
#define CE_LDPC_L_BOUND 4497     /* 127 + 95 * 46: the largest |L| any plan can reach */
#define CE_LDPC_LDS_MAX 163840   /* one CU's LDS: what a workgroup may take */
#define CE_LDPC_F32 0
#define CE_LDPC_I8 1
/* The kernel keeps, per lifted check, the row's last result in 5 bytes: one dword (bit e < 19: R_e is negative; bits
 * 19..23: idx; bits 24..30: (3 min1) >> 2) and one byte ((3 min2) >> 2). */
#define CE_LDPC_STATE_IDX_SHIFT 19
#define CE_LDPC_STATE_MAG_SHIFT 24

typedef struct ce_ldpc_desc {
  int32_t abi_version;      /* = CE_ABI_VERSION */
  int32_t device;           /* HIP device ordinal the plan lives on */
  int32_t zc;               /* lifting size, 2 .. 384, any integer (the NR set is a subset) */
  int32_t n_rows;           /* M_b: 1 .. 46 */
  int32_t n_cols;           /* N_b: <= 68 and > n_rows; n_sys = n_cols - n_rows */
  int32_t n_punctured_cols; /* 0 .. n_sys leading columns that are not transmitted (NR: 2) */
  int32_t n_in;             /* input row length: 1 <= n_in, n_in + n_punctured_cols zc <= n_cols zc (NR: N_cb) */
  int32_t k_out;            /* hard bits written per block: 1 .. n_sys zc (NR: K') */
  int32_t in_format;        /* CE_LDPC_I8 or CE_LDPC_F32 */
  int32_t max_iters;        /* 1 .. 255 */
  int32_t early_stop;       /* 0 or 1 */
  float llr_scale;          /* float32 input only: positive and finite */
  /* the graph as a CSR edge list in host memory, read at plan creation only: every row has 2 .. CE_LDPC_MAX_ROW_DEGREE
   * edges, the columns within a row are distinct, col in 0 .. n_cols - 1, shift in 0 .. zc - 1 */
  const int32_t* row_start; /* [n_rows + 1], row_start[0] = 0, n_edges = row_start[n_rows] */
  const int32_t* col;       /* [n_edges] */
  const int32_t* shift;     /* [n_edges] */
} ce_ldpc_desc;

typedef struct ce_ldpc_plan ce_ldpc_plan; /* opaque */

typedef struct ce_ldpc_info {
  int32_t n_edges;
  int32_t row_bytes;            /* bytes per block of `hard`: 16 ceil(k_out / 128) */
  int32_t n_bits;               /* n_cols zc: elements per block of `post` */
  int32_t blocks_per_workgroup;
  int32_t threads;
  int32_t lds_bytes;
} ce_ldpc_info;

/* What ce_ldpc_plan_create derives on the host. */
typedef struct ce_ldpc_host_view {
  int32_t n_sys;
  int32_t n_edges;
  int32_t max_row_degree;
  int32_t max_col_degree;
  int32_t row_bytes;            /* 16 ceil(k_out / 128) */
  int32_t n_bits;               /* n_cols zc */
  int32_t threads_per_block;    /* zc: one lifted check per thread */
  int32_t blocks_per_workgroup; /* max(1, min(256 / zc, 80896 / lds_bytes_per_block)): two such workgroups fit a CU */
  int32_t threads;              /* threads_per_block * blocks_per_workgroup */
  int32_t lds_l_bytes;          /* per block: L as int16, n_cols zc elements, rounded up to 16 bytes */
  int32_t lds_state32_bytes;    /* per block: n_rows zc dwords (rounded up to 16 bytes) */
  int32_t lds_state8_bytes;     /* per block: n_rows zc bytes, rounded up to 16 bytes */
  int32_t lds_bytes_per_block;  /* the sum of the three */
  int32_t lds_flag_bytes;       /* per workgroup: one dword per block and one for the workgroup, rounded up to 16 bytes */
  int32_t lds_bytes;            /* blocks_per_workgroup * lds_bytes_per_block + lds_flag_bytes */
  int32_t schedule_bytes;       /* the plan's device buffer: (n_rows + 1) row starts, then (col zc) << 16 | shift per edge */
  int32_t state_idx_shift;      /* CE_LDPC_STATE_IDX_SHIFT */
  int32_t state_mag_shift;      /* CE_LDPC_STATE_MAG_SHIFT */
} ce_ldpc_host_view;

/* Validation and derivation of ce_ldpc_plan_create without touching a GPU: usable on a CPU-only host.
 * CE_ERR_INVALID with a text naming the field for anything outside the ranges stated at ce_ldpc_desc;
 * CE_ERR_UNSUPPORTED for a plan whose lds_bytes exceed CE_LDPC_LDS_MAX (none within those ranges does: the largest,
 * 46 x 68 at zc = 384, takes 140 560 bytes). */
int ce_ldpc_derive_host(const ce_ldpc_desc* desc, ce_ldpc_host_view* view);

/* Validates the descriptor and uploads the schedule. */
int ce_ldpc_plan_create(const ce_ldpc_desc* desc, ce_ldpc_plan** out);
void ce_ldpc_plan_destroy(ce_ldpc_plan* plan);
int ce_ldpc_plan_get_info(const ce_ldpc_plan* plan, ce_ldpc_info* info);

/*
 * Decodes n_blocks code blocks (slots x C) in ONE launch on `stream` (a hipStream_t; NULL = the default stream).
 * Asynchronous; n_blocks == 0 launches nothing.
 *  in      [n_blocks][n_in] int8 or float32 (the plan's in_format), dense: ce_rm_recover's out, seen as slots x C rows
 *  hard    [n_blocks][row_bytes] uint8: bit i < k_out is h_i, MSB first; the padding bits are 0
 *  status  [n_blocks][2] int32: {iterations executed, parity holds ? 1 : 0}
 *  post    [n_blocks][n_cols zc] int16: the final L; NULL skips it
 * in, hard, status and post must be 16-byte aligned (CE_ERR_INVALID otherwise); the rows of `in` and `post` need not be
 * (N_cb = 350 in int8).  Inputs and outputs must not overlap.  No atomics, no scratch, no workspace; every address comes
 * from the block index, the thread index and host-derived plan values, tensor values enter arithmetic only.
 */
int ce_ldpc_decode(const ce_ldpc_plan* plan, const void* in, int64_t n_blocks, uint8_t* hard, int32_t* status, int16_t* post,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_LDPC_H */

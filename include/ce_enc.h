/*
 * ce_enc.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: the PUSCH transport-block encoder, the forward
 * counterpart of ce_rm_recover, ce_ldpc_decode and ce_tb_assemble in one stage.  It turns the row ce_tb_assemble writes,
 * `tb[slot][tb_row_bytes]`, into the rate-matched bit row `g[slot][G]` a modulator takes, under the caller's LdpcGraph.
 * All section numbers are TS 38.212.
 *
 * The reference (pjookim/srsran-ce-pytorch) stops at the channel estimate.  The operator is pinned by tests/enc_oracle.py,
 * which composes tests/tb_oracle.py (segment), a numpy encoder and tests/rm_oracle.py (slot_map); everything is bits and
 * results are compared by value, without a tolerance.
 *
 * Operator, per slot.  Bit i < A of the transport block is bit 7 - (i mod 8) of byte floor(i / 8) of tb[slot][.] (MSB first);
 * bits from A on are ignored, whatever they hold.
 *   5.1      s = tb bits | L_tb parity bits (CRC24A for A > 3824, else CRC16), the CRC convention of ce_tb.h;  B = A + L_tb
 *   5.2.2    block r takes s[r P .. (r + 1) P), P = B / C; for C > 1 the CRC24B of these P bits follows; then zero filler
 *            bits from K' to K.  A filler bit is 0 in the encoder and is never transmitted.
 *   5.3.2    the codeword c_r[0 .. n_cols Zc): the K information bits, then the parity columns, with H c = 0 for the lifted
 *            graph: row (r, z) sums c[col Zc + (z + shift) mod Zc] over the row's (col, shift) edges, as ce_ldpc.h reads it
 *   5.4.2.1, 5.4.2.2, 5.5   bit i of g[slot] belongs to block r, buffer position n, under the slot's rv, exactly as element i
 *            of ce_rm_recover's llr row does (ce_rm.h):  g_i = c_r[n + 2 Zc].  Repetition wraps round N_cb, the filler
 *            positions are skipped.
 * Outputs: g[slot][g_row_bytes], MSB first, zeros behind bit G;  on request cw[slot][C][cw_row_bytes], the whole codeword
 * (punctured columns included, fillers 0), MSB first, zeros behind bit n_cols Zc.
 *
 * Integers.  Segmentation and rate matching (B, C, K', Zc, K, N_cb, f0, f1, P_rm, E_r, k0, s) are ce_rm_derive_host's: the
 * encoder calls that function, so the two stages cannot disagree, and whatever it refuses is refused here in its words.
 * L_tb, L_cb, the payload P and the polynomials are ce_tb.h's.
 *
 * Which graphs are accepted (ce_enc_derive_host).  n_sys = n_cols - n_rows must be 22 (base graph 1) / 10 (2), n_cols at
 * most 68 / 52, n_rows >= 4, a row has at most CE_LDPC_MAX_ROW_DEGREE edges, and (n_cols - 2) Zc >= N_cb (a prefix of rows --
 * LdpcGraph.truncated -- is a graph like any other where n_ref makes N_cb fit).  Every row r >= 4 holds its own column
 * n_sys + r exactly once, at shift 0; that column appears in no other row; the row's other edges lie in columns
 * < n_sys + 4.  The core -- rows 0-3 against columns n_sys .. n_sys + 3 -- has one of two forms:
 *   triangular  row i holds (n_sys + i, 0) and of the core columns otherwise only those < n_sys + i: forward substitution.
 *   NR core     column n_sys + j (j = 1, 2, 3) appears in exactly rows j - 1 and j, both at shift 0; column n_sys appears
 *               in exactly three of the four rows, with shifts of which at least two are equal.  With lambda_i the XOR of
 *               row i's rotated systematic columns, lambda_0 ^ lambda_1 ^ lambda_2 ^ lambda_3 is the first parity column
 *               rotated by the remaining shift (the three shifts XOR-cancel in pairs); the other three parity columns
 *               follow from rows 0, 1, 2 in turn and row 3 holds by construction.
 * The NR-core form is THIS PROJECT'S READING of the shape of Tables 5.3.2-2 / 5.3.2-3.  The tables are not in this
 * repository and nothing is tested against them; the tests use seeded random graphs of both forms.
 * Anything else is CE_ERR_INVALID with a text naming the row or column that breaks the form.
 */
#ifndef CE_ENC_H
#define CE_ENC_H

#include "ce_ldpc.h"
#include "ce_rm.h"
#include "ce_tb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_ENC_THREADS 256     /* one workgroup per (slot, code block) */
#define CE_ENC_CORE_TRIANGULAR 0
#define CE_ENC_CORE_NR 1
#define CE_ENC_CRC_CHUNK 1024  /* dwords of a bit string one pass of the workgroup runs through a CRC: 4 per thread */

typedef struct ce_enc_desc {
  int32_t abi_version; /* = CE_ABI_VERSION */
  int32_t device;      /* HIP device ordinal the plan lives on */
  int32_t base_graph;  /* 1 or 2, as in ce_rm_desc */
  int32_t tbs;         /* A >= 1 */
  int32_t qm;          /* 2, 4, 6 or 8 */
  int32_t n_layers;    /* 1 .. 4 */
  int32_t g_bits;      /* G */
  int32_t n_ref;       /* 0, or N_ref >= K - 2 Zc */
  int32_t n_rows;      /* base rows of the graph */
  int32_t n_cols;      /* base columns; n_sys = n_cols - n_rows */
  const int32_t* row_start; /* [n_rows + 1], host memory, copied: the graph in the form ce_ldpc_desc takes */
  const int32_t* col;       /* [n_edges] */
  const int32_t* shift;     /* [n_edges], 0 .. Zc - 1 */
} ce_enc_desc;

typedef struct ce_enc_plan ce_enc_plan; /* opaque */

typedef struct ce_enc_info {
  int32_t n_code_blocks;  /* C */
  int32_t tb_row_bytes;   /* bytes per slot of `tb` */
  int32_t g_row_bytes;    /* bytes per slot of `g` */
  int32_t cw_row_bytes;   /* bytes per code block of `cw` */
  int32_t cw_required;    /* 1: ce_enc_encode needs `cw` (see there) */
  int32_t reserved0;
  int64_t bytes_per_slot; /* tb_row_bytes in; g_row_bytes (+ C cw_row_bytes) out */
} ce_enc_info;

/* What ce_enc_plan_create derives on the host. */
typedef struct ce_enc_host_view {
  int32_t b, k_cb, c, b_prime, k_prime, k_b, zc, k, n, n_cb; /* as ce_rm_host_view */
  int32_t f0, f1;         /* filler positions [f0, f1) of the circular buffer */
  int32_t p_rm;           /* ce_rm_host_view.p: non-filler positions of one turn */
  int32_t n_lo, e_lo, e_hi;
  int32_t k0[4];
  int32_t s[4];
  int32_t l_tb, l_cb;     /* as ce_tb_host_view */
  int32_t p;              /* payload bits per block, B / C */
  int32_t g_tb, g_cb;
  int32_t tb_row_bytes;   /* 16 ceil(A / 128) */
  int32_t g_row_bytes;    /* 16 ceil(G / 128) */
  int32_t cw_row_bytes;   /* 16 ceil(n_cols Zc / 128) */
  int32_t n_sys;
  int32_t n_edges;
  int32_t core_form;      /* CE_ENC_CORE_TRIANGULAR or CE_ENC_CORE_NR */
  int32_t core_rows;      /* NR core: bit i set = row i holds column n_sys; triangular: 0 */
  int32_t core_shift;     /* NR core: the shift that remains when the two equal ones cancel; triangular: 0 */
  int32_t rows_needed;    /* rows whose parity column starts below 2 Zc + N_cb: the others are computed for `cw` only */
  int32_t col_dwords;     /* ceil(Zc / 32): dwords of a column */
  int32_t ext_dwords;     /* dwords of a column's periodic image in LDS (2 Zc + 32 bits and one to spare) */
  int32_t cw_required;    /* 1 where two code blocks meet inside a dword of g (an E_r prefix sum is no multiple of 32) */
  int32_t threads;        /* CE_ENC_THREADS */
  int32_t lds_bytes;      /* static LDS of the encode kernel */
  int32_t table_bytes;    /* the plan's device buffer: edges, powers of x */
} ce_enc_host_view;

/* Validation and integer derivation of ce_enc_plan_create without touching a GPU: usable on a CPU-only host.  Refuses what
 * ce_rm_derive_host refuses (same text), and the graphs described above. */
int ce_enc_derive_host(const ce_enc_desc* desc, ce_enc_host_view* view);

/* Validates the descriptor and uploads the edge list and the powers of x (table_bytes of device memory). */
int ce_enc_plan_create(const ce_enc_desc* desc, ce_enc_plan** out);
void ce_enc_plan_destroy(ce_enc_plan* plan);
int ce_enc_plan_get_info(const ce_enc_plan* plan, ce_enc_info* info);

/*
 * Encodes n_slots transport blocks on `stream` (a hipStream_t; NULL = the default stream).  Asynchronous; n_slots == 0
 * launches nothing.
 *  tb   [slot][tb_row_bytes] uint8, dense: the row ce_tb_assemble writes
 *  rv   int32 device array; slot b reads element b * rv_stride (in elements, >= 0; 0 = one value for the whole batch).  Only
 *       rv & 3 is used, so an out-of-range value cannot address memory.
 *  g    [slot][g_row_bytes] uint8
 *  cw   [slot][C][cw_row_bytes] uint8, or NULL
 * One launch of one workgroup per (slot, code block) computes the codeword in LDS, stores it to `cw` where given, and
 * gathers the block's bits of g straight from LDS.  Where cw_required is set -- C > 1 and two blocks' bits share a dword of
 * g -- no workgroup holds all 32 bits of such a dword: the first launch then only stores the codewords and a second one
 * gathers g from `cw`, so `cw` must be given (CE_ERR_INVALID otherwise; the Python wrapper allocates it).
 * tb, g and cw must be 16-byte aligned (CE_ERR_INVALID otherwise) and must not overlap.  No atomics, no scratch; every byte
 * of g and cw has one writer, and no kernel reads what it wrote.  Every address comes from the block index, the thread index,
 * host-derived plan values and rv & 3; the one data-dependent address is an index into a CRC table in LDS, masked to the
 * table's size.
 */
int ce_enc_encode(const ce_enc_plan* plan, const uint8_t* tb, const int32_t* rv, int64_t rv_stride, int64_t n_slots, uint8_t* g,
                  uint8_t* cw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_ENC_H */

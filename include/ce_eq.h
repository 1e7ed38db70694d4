/*
 * ce_eq.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: a noise-whitened, unbiased LMMSE equalizer
 * over the PUSCH data REs, the consumer of ce_estimate_batch's `ch_est` and `noise`.
 *
 * The reference (pjookim/srsran-ce-pytorch) stops at the channel estimate.  The operator is pinned by the float64
 * restatement in tests/eq_oracle.py (np.linalg.inv, no Cholesky) and the tolerance rule stated there.
 *
 * Operator, per data RE (k, s) of slot b, with R Rx ports and L layers; h_r = ch_est[b, r, k, s, :] (a 1 x L row),
 * y_r = rx[b, r, k, s], n_r = noise[b, r]:
 *     w_r     = 1 / n_r  if n_r, rounded to float32, is finite and > 0, else 0    (a bad port drops out)
 *     A       = I_L + sum_r w_r h_r^H h_r                                          (Hermitian, A >= I)
 *     z       = sum_r w_r h_r^H y_r
 *     d_l     = [A^-1]_ll,  b_l = 1 - d_l                                          (b_l: the LMMSE bias, diag of W H)
 *     x_hat_l = [A^-1 z]_l / b_l,   nvar_l = d_l / b_l                             (unbiased estimate, 1 / SINR_l)
 *     where b_l <= 0 (every port dropped, or h = 0):  x_hat_l = 0, nvar_l = +inf
 * float32 throughout; A is factored by an unpivoted Cholesky decomposition.  L = 1 is computed as g = sum_r w_r |h_r|^2,
 * x_hat = z / g, nvar = 1 / g (no 1 - d cancellation).  `ch_est` is used as given: a data / DM-RS power offset is the
 * caller's to fold in.  A noise variance below the smallest normal float32 is outside the operator's range.
 *
 * Data REs: the REs of PRBs prb_start .. prb_start + n_prbs - 1 on symbols start_symbol .. start_symbol +
 * n_alloc_symbols - 1 of each hop (the rectangle the estimator fills); on the hop's DM-RS symbols inside that
 * rectangle, RE r of every PRB is left out where bit r of reserved_re_mask is set.  Two hops must not share a symbol.
 * Output order: symbol ascending over the slot, subcarrier ascending within a symbol, layer fastest (TS 38.211
 * 6.3.1.6 frequency-first mapping with the layers interleaved as in 6.3.1.3):
 *     x_hat[slot][n_data_re][L] complex64,  nvar[slot][n_data_re][L] float32,  both dense.
 */
#ifndef CE_EQ_H
#define CE_EQ_H

#include "ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_EQ_MAX_PORTS 8
#define CE_EQ_CHUNK_SC 36 /* subcarriers one workgroup handles (3 PRB): 36 * 14 = 504 REs on 256 threads, two each */

typedef struct ce_eq_hop_desc {
  uint8_t dmrs_symbols[CE_MAX_SYMBOLS]; /* 1 where the OFDM symbol carries DM-RS (ignored outside the hop's symbols) */
  uint16_t reserved_re_mask;            /* bit r set <=> RE r of each PRB carries no data on the hop's DM-RS symbols:
                                           0xFFF none; 0x555 type 1, one CDM group without data; 0x3CF type 2, two */
  int32_t prb_start;
  int32_t n_prbs;
  int32_t start_symbol;
  int32_t n_alloc_symbols;
} ce_eq_hop_desc;

typedef struct ce_eq_desc {
  int32_t abi_version; /* = CE_ABI_VERSION */
  int32_t device;      /* HIP device ordinal the plan lives on */
  int32_t n_prb_grid;  /* 12 * n_prb_grid <= CE_FFT_SIZE, as for ce_plan_desc */
  int32_t n_sym;       /* OFDM symbols in the grid, 1..CE_MAX_SYMBOLS */
  int32_t n_layers;    /* 1..CE_MAX_LAYERS */
  int32_t n_hops;      /* 1 or 2 */
  ce_eq_hop_desc hop[CE_MAX_HOPS];
} ce_eq_desc;

typedef struct ce_eq_plan ce_eq_plan; /* opaque: the per-symbol table on the device */

typedef struct ce_eq_info {
  int32_t n_data_re;      /* rows of x_hat / nvar per slot */
  int32_t reserved0;
  int64_t bytes_per_slot; /* n_data_re * n_layers * (8 + 4) */
} ce_eq_info;

/* What ce_eq_plan_create derives on the host.  Data RE `re` of PRB q (q counted over the grid) on symbol s has the
 * output row  first_row[s] + (q - prb_start of sym_hop[s]) * data_res_per_prb[s] + popcount(data_mask[s] & ((1 << re) - 1)). */
typedef struct ce_eq_host_view {
  int32_t sym_hop[CE_MAX_SYMBOLS];          /* the hop whose rectangle holds the symbol, or -1 */
  int32_t data_mask[CE_MAX_SYMBOLS];        /* 12-bit mask of the data REs of each of its PRBs (0 where sym_hop = -1) */
  int32_t data_res_per_prb[CE_MAX_SYMBOLS]; /* its set bits */
  int32_t first_row[CE_MAX_SYMBOLS];        /* output row of the symbol's first data RE (the running count where it has none) */
  int32_t n_data_re;
} ce_eq_host_view;

/* Validation and derivation of ce_eq_plan_create without touching a GPU: usable on a CPU-only host. */
int ce_eq_derive_host(const ce_eq_desc* desc, ce_eq_host_view* view);

/* Validates the descriptor, derives the table and uploads it.  Synchronous; not for the per-slot loop. */
int ce_eq_plan_create(const ce_eq_desc* desc, ce_eq_plan** out);
void ce_eq_plan_destroy(ce_eq_plan* plan);
int ce_eq_plan_get_info(const ce_eq_plan* plan, ce_eq_info* info);

/*
 * Equalizes n_slots slots in ONE launch on `stream` (a hipStream_t; NULL = the default stream).  Asynchronous;
 * n_slots == 0 launches nothing.
 *  rx        complex64, element (slot b, port r, subcarrier k, symbol s) at rx[b*rx_strides[0] + r*rx_strides[1] +
 *            k*rx_strides[2] + s*rx_strides[3]] (strides in complex elements, >= 0), exactly as in ce_estimate_batch
 *  ch_est    complex64, dense [slot][port][subcarrier][symbol][layer] as ce_estimate_batch writes it
 *  noise     float64 [slot][port] as ce_estimate_batch writes it
 *  n_ports   1..CE_EQ_MAX_PORTS
 *  x_hat     out, complex64 [slot][n_data_re][n_layers];  nvar  out, float32, the same shape
 * ch_est, x_hat and nvar must be 16-byte aligned (CE_ERR_INVALID otherwise).  Only the data REs of rx and ch_est are
 * read; noise and the tensor values enter arithmetic only, every address comes from the plan's host-derived table.
 */
int ce_eq_equalize(const ce_eq_plan* plan, const void* rx, const int64_t rx_strides[4], const void* ch_est,
                   const double* noise, int64_t n_slots, int32_t n_ports, void* x_hat, float* nvar, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_EQ_H */

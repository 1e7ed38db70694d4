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

/*
 * LOW-PAPR DM-RS, the PUSCH pilots with transform precoding ON (38.211 6.4.1.1.1.2 and 5.2.2): a Zadoff-Chu base sequence
 * with group or sequence hopping, cyclic shift alpha = 0.  One layer, configuration type 1, single-symbol DM-RS.  The entry
 * points take scalars and pointers only; the host view is handed out through caller-provided arrays.  Pinned by
 * tests/dmrs_lp_oracle.py, which runs the formulas below literally; every comparison is bit for bit.
 *
 * Plan values:
 *     n_prb_grid, n_sym, n_symb_slot, n_layers, n_hops      as in ce_dmrs_desc; n_layers must be 1
 *     dmrs_symbols[n_hops][CE_MAX_SYMBOLS]                  1 where the OFDM symbol carries DM-RS
 *     re_mask[n_hops]                                       0x555 or 0xAAA
 *     mask_prbs[n_hops][n_prb_grid]                         0/1; the active PRBs of a hop are ONE contiguous run of n_prb
 *                                                           PRBs, the same n_prb in both hops
 *     hopping                                               CE_DMRS_LP_HOP_NEITHER / _GROUP / _SEQUENCE
 *     slots_per_frame                                       10, 20, 40, 80 or 160
 *     phi[30][M_ZC]                                         int8 in {-3, -1, 1, 3}: the table phi_u(n) of 38.211 5.2.2.2 for this
 *                                                           M_ZC, needed where M_ZC <= 24 and ignored elsewhere (NULL: none).  The
 *                                                           tables are data of the caller's, as the LDPC base graphs are.
 * Operator, per slot b with parameters (slot, n_id) and per DM-RS column s (hop 1's DM-RS symbols ascending, then hop 2's)
 * at OFDM symbol l, with M_ZC = 6 n_prb and p = n_symb_slot (slot mod slots_per_frame) + l:
 *     u = (f_gh + n_id) mod 30, c(.) the Gold sequence of 5.2.1
 *         neither     f_gh = 0, v = 0
 *         group       f_gh = (sum_{m<8} 2^m c(8 p + m)) mod 30 with c_init = floor(n_id / 30); v = 0
 *         sequence    f_gh = 0; v = c(p) with c_init = n_id where M_ZC >= 72, else 0
 *     M_ZC >= 36      N_ZC = the largest prime < M_ZC; q = floor((2 N_ZC (u + 1) + 31) / 62), plus v where
 *                     floor(2 N_ZC (u + 1) / 31) is even, minus v where it is odd (q_bar = N_ZC (u + 1) / 31 in integers);
 *                     r(n) = W_N[e], N = N_ZC, e = (q (t (t + 1) / 2 mod N)) mod N, t = n mod N
 *     M_ZC = 30       r(n) = W_31[e], e = ((u + 1) ((n + 1) (n + 2) / 2 mod 31)) mod 31
 *     M_ZC <= 24      r(n) = exp(j phi_u(n) pi / 4) = (+-a, +-a), a = float32 0x3f3504f3
 *     W_N[e] = (float32(cos th), float32(-sin th)), th = 2 pi e / N evaluated in double on the host at plan creation;
 *     W_N[0] = (1, +0).  The device only gathers from the table: the result is defined to the bit.
 * Output pilots[slot][n_re][n_dmrs_total][1] complex64, dense, n_re = M_ZC: row k is r(k), counted from the allocation's
 * first pilot (not from CRB 0 as the Gold sequence of ce_dmrs_generate is).  Every element is written exactly once.
 */
#define CE_DMRS_LP_HOP_NEITHER 0
#define CE_DMRS_LP_HOP_GROUP 1
#define CE_DMRS_LP_HOP_SEQUENCE 2
#define CE_DMRS_LP_MAX_WORDS 560 /* 32-bit words of c the hopping reads: 8 bits per symbol of a frame, 8 * 14 * 160 / 32 */
#define CE_DMRS_LP_FORM_ZC 0     /* M_ZC >= 36 */
#define CE_DMRS_LP_FORM_30 1     /* M_ZC = 30 */
#define CE_DMRS_LP_FORM_PHI 2    /* M_ZC <= 24 */
#define CE_DMRS_LP_INFO_LEN 8

typedef struct ce_dmrs_lp_plan ce_dmrs_lp_plan; /* opaque */

/*
 * Host only: validation and integer derivation of ce_dmrs_lp_plan_create without touching a GPU.  Every output array may
 * be NULL (not wanted):
 *     info[CE_DMRS_LP_INFO_LEN]        n_re, n_dmrs_total, form (CE_DMRS_LP_FORM_*), N (N_ZC, 31 or 0), n_words, v_live (1:
 *                                      sequence hopping with M_ZC >= 72), n_prb, 0
 *     col_sym[CE_MAX_SYMBOLS]          per column: its OFDM symbol index l
 *     q[30][2]                         [u][v]: q of the Zadoff-Chu form, u + 1 of the length-30 form, 0 of the table form
 *     tri[CE_DMRS_MAX_RE]              per row k < n_re: t (t + 1) / 2 mod N with t = k mod N; (k + 1) (k + 2) / 2 mod 31 of
 *                                      the length-30 form; 0 of the table form.  So e = (q[u][v] tri[k]) mod N in both.
 *     hop_words[32][n_words]           the hopping bits, linear in c_init as the tables of ce_dmrs_host_view: word w of c (bit
 *                                      n of c in bit n % 32 of word n / 32) is row 0 XOR the rows 1 + i of the set bits i of
 *                                      c_init; n_words = ceil(n_symb_slot slots_per_frame / 4) with group hopping,
 *                                      ceil(n_symb_slot slots_per_frame / 32) with sequence hopping, 0 with neither
 * CE_ERR_INVALID: a null pointer among dmrs_symbols, re_mask, mask_prbs; n_hops outside 1..2; n_symb_slot not 14 or 12;
 * n_sym outside 1..n_symb_slot; a re_mask other than 0x555 / 0xAAA; hops that share a symbol or have none; hops of unequal
 * n_prb; an unknown hopping mode; a slots_per_frame outside the five values; a phi value outside {-3, -1, 1, 3}.
 * CE_ERR_UNSUPPORTED: n_layers != 1; a grid outside 1..341 PRB; active PRBs that are not one contiguous run;
 * M_ZC <= 24 without a phi table.
 */
int ce_dmrs_lp_derive_host(int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot, int32_t n_layers, int32_t n_hops,
                           const uint8_t* dmrs_symbols, const uint16_t* re_mask, const uint8_t* mask_prbs, int32_t hopping,
                           int32_t slots_per_frame, const int8_t* phi, int32_t* info, int32_t* col_sym, int32_t* q, int32_t* tri,
                           uint32_t* hop_words);

/* Host only: W_N[e], e < n, as n (re, im) float32 pairs into `twiddles`; 2 <= n <= CE_DMRS_MAX_RE. */
int ce_dmrs_lp_copy_twiddles(int32_t n, float* twiddles);

/* Validates the values, derives the tables once and uploads them to `device`; abi_version = CE_ABI_VERSION.  Synchronous. */
int ce_dmrs_lp_plan_create(int32_t abi_version, int32_t device, int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot,
                           int32_t n_layers, int32_t n_hops, const uint8_t* dmrs_symbols, const uint16_t* re_mask,
                           const uint8_t* mask_prbs, int32_t hopping, int32_t slots_per_frame, const int8_t* phi,
                           ce_dmrs_lp_plan** out);
void ce_dmrs_lp_plan_destroy(ce_dmrs_lp_plan* plan);

/*
 * Writes pilots_out[n_slots][n_re][n_dmrs_total][1] (complex64, dense, 8-byte aligned, on the plan's device) in ONE launch
 * on `stream` (NULL = the default stream).  Asynchronous; n_slots == 0 launches nothing.
 *  slot, n_id    int32 device arrays, 4-byte aligned; slot b reads element b * slot_stride / b * n_id_stride (strides in
 *                elements, >= 0; 0 = one value for the whole batch).  Neither can address memory.  Both are taken as
 *                UNSIGNED 32-bit values: the kernel uses slot only as slot mod slots_per_frame, which bounds every index
 *                into the hopping table; n_id enters u as n_id mod 30 and c_init as floor(n_id / 30) (group) or n_id
 *                (sequence), masked to 31 bits.  An out-of-range value therefore yields the pilots of
 *                (slot mod slots_per_frame, that u, that c_init) -- for a negative int32 those of its value + 2^32.
 * CE_ERR_INVALID: a null plan or pointer; n_slots < 0; a negative stride; slot or n_id not 4-byte or pilots_out not 8-byte
 * aligned.  CE_ERR_UNSUPPORTED: more than 2^31 - 1 slots in one launch.
 */
int ce_dmrs_lp_generate(const ce_dmrs_lp_plan* plan, const int32_t* slot, int64_t slot_stride, const int32_t* n_id,
                        int64_t n_id_stride, int64_t n_slots, void* pilots_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_DMRS_H */

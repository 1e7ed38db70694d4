/*
 * ce_mod.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: the PUSCH modulator, the forward counterpart of
 * ce_demod_demap and of the data-RE walk of ce_eq_equalize in one stage.  It turns the rate-matched bit row ce_enc_encode
 * writes, `g[slot][g_row_bytes]`, and the pilots ce_dmrs_generate writes into the resource grid of every layer,
 * `tx[slot][layer][n_sym][n_sc]`.  All section numbers are TS 38.211.
 *
 * The reference (pjookim/srsran-ce-pytorch) stops at the channel estimate.  The operator is pinned by tests/mod_oracle.py,
 * which composes demod_oracle (scrambling, c_init, the level tables of the constellations), eq_oracle.data_re_ref and the
 * pilot row rule of dmrs_oracle.pilots_ref; every result is one float32 multiply or +0, so results are compared by value,
 * without a tolerance.
 *
 * Operator, per slot b with (rnti, n_id), a scalar beta_dmrs, L layers and G = n_data_re L Qm bits.  Bit n < G of g[b] is bit
 * 7 - (n mod 8) of byte floor(n / 8) (MSB first); bits from G on are ignored, whatever they hold.
 *   6.3.1.1  b~(n) = g(n) ^ c(n), n < G (plan flag), c the Gold sequence of 5.2.1 with c_init = (n_RNTI 2^15 + n_ID) mod 2^31
 *            in unsigned 32-bit arithmetic: the demapper's convention exactly (ce_demod.h).  UCI placeholder bits are out
 *            of scope, as there.
 *   6.3.1.2  symbol i takes b~(i Qm .. i Qm + Qm - 1) under the Gray maps of 5.1.3 - 5.1.6 (ce_demod.h).  With s_j = 1 - 2 b~_j
 *            the real part has the odd integer level
 *                QPSK s0;  16QAM s0 (2 - s2);  64QAM s0 (4 - s2 (2 - s4));  256QAM s0 (8 - s2 (4 - s4 (2 - s6)))
 *            and the imaginary part the same of the odd bits.  Each part is float32(level) * A_qm, ONE float32 multiply,
 *            A_qm the float32 nearest to 1 / sqrt(2, 10, 42, 170) (CE_MOD_A_* below): the result is defined to the bit.
 *   6.3.1.3  symbol i goes to layer i mod L, data RE row floor(i / L): layer fastest, the order of ce_eq_equalize's x_hat.
 *   6.3.1.6  data RE row -> (symbol, subcarrier) exactly as ce_eq_derive_host defines it (ce_eq.h): symbol ascending,
 *            subcarrier ascending; on a hop's DM-RS symbols the REs in reserved_re_mask are skipped.  The plan calls
 *            ce_eq_derive_host, so modulator and equalizer cannot disagree, and whatever it refuses is refused here in
 *            its words.  Precoding is the identity: layer l is antenna port l.
 *   6.4.1.1.3  on DM-RS symbol s of hop h -- pilot column `col` as in ce_dmrs.h: hop 1's DM-RS symbols ascending, then hop
 *            2's -- layer l carries beta_dmrs * pilots[b][k][col][l] (each part one float32 multiply) on the k-th set RE of
 *            re_mask[l / 2] repeated over PRBs prb_start .. prb_start + n_prbs - 1.
 *   Everything else is +0: REs outside both hops' rectangles, REs of another layer's CDM group, reserved REs that carry no
 *   pilot of this layer.
 *
 * What a transmitter does not do is refused (CE_ERR_INVALID): a scattered mask_prbs (a quirk of the reference's extractor);
 * a re_mask[c] in use that is empty, not inside reserved_re_mask (an RE would be pilot and data), or of another size than
 * re_mask[0] (the pilot rows of the layers would differ); a DM-RS symbol outside its hop's symbols; hops of unequal n_prbs.
 * Limits: G <= CE_DEMOD_MAX_BITS (CE_ERR_UNSUPPORTED, the demapper's text), L <= CE_MAX_LAYERS, two hops share no symbol
 * (both ce_eq_derive_host's).
 *
 * Output tx[slot][layer][n_sym][n_sc] complex64, dense, subcarrier fastest.  Every element has exactly one writer in one
 * launch: the caller need not clear it.  The Python wrapper returns the [B, L, n_sc, n_sym] permuted view, the
 * subcarrier-contiguous layout the estimator's pilot loads coalesce on: with an identity channel, tx of an L = R slot can be
 * handed to ce_estimate_batch as it is.
 */
#ifndef CE_MOD_H
#define CE_MOD_H

#include "ce_demod.h"
#include "ce_eq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_MOD_THREADS 256     /* one workgroup per (slot, group of CE_MOD_GROUP_SYMBOLS OFDM symbols, tile of CE_MOD_TILE_SC
                                  subcarriers), all layers */
#define CE_MOD_TILE_SC 256     /* subcarriers of a tile: 128 lanes x 16 bytes per layer row, two (symbol, layer) rows per pass */
#define CE_MOD_GROUP_SYMBOLS 7 /* OFDM symbols of a group: 7 x CE_MOD_MAX_TILE_BLOCKS <= 256, one thread per (symbol, Gold block) */
#define CE_MOD_MAX_TILE_BLOCKS 34 /* Gold blocks (CE_DEMOD_BLOCK_WORDS words) a tile's bit range can touch: 256 subcarriers x 4
                                     layers x 8 bits = 8192 bits = 32 blocks, + 1 for a start inside a block, + 1 to spare */

/* A_qm as float32 bit patterns: the float32 nearest to 1 / sqrt(2), 1 / sqrt(10), 1 / sqrt(42), 1 / sqrt(170).
 * CE_MOD_A_QPSK is the DM-RS amplitude of ce_dmrs.h. */
#define CE_MOD_A_QPSK 0x3f3504f3u   /* 0.70710677  */
#define CE_MOD_A_16QAM 0x3ea1e89bu  /* 0.31622776  */
#define CE_MOD_A_64QAM 0x3e1e01b3u  /* 0.15430336  */
#define CE_MOD_A_256QAM 0x3d9d130eu /* 0.07669650  */

typedef struct ce_mod_hop_desc {
  uint8_t dmrs_symbols[CE_MAX_SYMBOLS]; /* 1 where the OFDM symbol carries DM-RS; every one inside the hop's symbols */
  uint16_t re_mask[CE_MAX_CDM];         /* bit r set <=> RE r of each PRB is a pilot of CDM group c (layers 2c, 2c + 1) */
  uint16_t reserved_re_mask;            /* as ce_eq_hop_desc: REs without data on the hop's DM-RS symbols */
  int32_t prb_start;
  int32_t n_prbs;
  int32_t start_symbol;
  int32_t n_alloc_symbols;
  const uint8_t* mask_prbs;             /* NULL, or n_prb_grid bytes (0/1) that must equal the run prb_start .. + n_prbs - 1;
                                           host memory, read during derivation only */
} ce_mod_hop_desc;

typedef struct ce_mod_desc {
  int32_t abi_version; /* = CE_ABI_VERSION */
  int32_t device;      /* HIP device ordinal the plan lives on */
  int32_t n_prb_grid;  /* 12 * n_prb_grid <= CE_FFT_SIZE, as for ce_eq_desc */
  int32_t n_sym;       /* OFDM symbols in the grid, 1..CE_MAX_SYMBOLS */
  int32_t n_layers;    /* 1..CE_MAX_LAYERS; layer l reads re_mask[l / 2] */
  int32_t qm;          /* 2, 4, 6 or 8 */
  int32_t scramble;    /* 0 or 1 */
  int32_t n_hops;      /* 1 or 2 */
  ce_mod_hop_desc hop[CE_MAX_HOPS];
} ce_mod_desc;

typedef struct ce_mod_plan ce_mod_plan; /* opaque: the Gold tables on the device */

typedef struct ce_mod_info {
  int32_t n_bits;         /* G = n_data_re * n_layers * qm */
  int32_t n_symbols;      /* n_data_re * n_layers */
  int32_t n_data_re;
  int32_t g_row_bytes;    /* bytes per slot of `g` */
  int32_t n_re;           /* pilots per column (= pilots.shape[1]) */
  int32_t n_dmrs_total;   /* pilot columns over both hops (= pilots.shape[2]) */
  int64_t bytes_per_slot; /* g_row_bytes + n_re n_dmrs_total L 8 in; L n_sym n_sc 8 out */
} ce_mod_info;

/* What ce_mod_plan_create derives on the host.  The per-symbol table is ce_eq_host_view's plus the pilot column. */
typedef struct ce_mod_host_view {
  int32_t n_bits;       /* G */
  int32_t g_row_bytes;  /* 16 ceil(G / 128) */
  int32_t n_data_re;
  int32_t n_symbols;    /* n_data_re * n_layers */
  int32_t n_re;         /* n_prbs * set bits of re_mask[0] */
  int32_t n_dmrs_total;
  int32_t sym_hop[CE_MAX_SYMBOLS];          /* as ce_eq_host_view */
  int32_t data_mask[CE_MAX_SYMBOLS];
  int32_t data_res_per_prb[CE_MAX_SYMBOLS];
  int32_t first_row[CE_MAX_SYMBOLS];
  int32_t dmrs_col[CE_MAX_SYMBOLS];         /* pilot column of the symbol, or -1 */
  int32_t n_words;      /* ceil(G / 32): words of c (0 without scrambling, as the three below) */
  int32_t block_words;  /* CE_DEMOD_BLOCK_WORDS */
  int32_t n_blocks;     /* ceil(n_words / block_words): jump entry sets kept */
  int32_t table_bytes;  /* the device tables, as ce_demod_host_view.table_bytes */
  int32_t tile_sc;      /* CE_MOD_TILE_SC */
  int32_t tiles_per_symbol;      /* ceil(n_sc / tile_sc) */
  int32_t group_symbols;         /* CE_MOD_GROUP_SYMBOLS */
  int32_t n_groups;              /* ceil(n_sym / group_symbols) */
  int32_t workgroups_per_slot;   /* n_groups * tiles_per_symbol */
  int32_t max_tile_blocks;       /* the most Gold blocks one tile of this plan touches (<= CE_MOD_MAX_TILE_BLOCKS) */
  int32_t threads;      /* CE_MOD_THREADS */
  int32_t lds_bytes;    /* static LDS of the kernel */
} ce_mod_host_view;

/* Validation and integer derivation of ce_mod_plan_create without touching a GPU: usable on a CPU-only host.  Refuses what
 * ce_eq_derive_host refuses (same text), and what is listed above. */
int ce_mod_derive_host(const ce_mod_desc* desc, ce_mod_host_view* view);

/* Validates the descriptor; a scrambling plan derives the Gold tables (the demapper's, ce_demod.h) and uploads them.
 * Synchronous; not for the per-slot loop. */
int ce_mod_plan_create(const ce_mod_desc* desc, ce_mod_plan** out);
void ce_mod_plan_destroy(ce_mod_plan* plan);
int ce_mod_plan_get_info(const ce_mod_plan* plan, ce_mod_info* info);

/*
 * Modulates n_slots slots in ONE launch on `stream` (a hipStream_t; NULL = the default stream).  Asynchronous; n_slots == 0
 * launches nothing.
 *  g          [slot][g_row_bytes] uint8, dense: the row ce_enc_encode writes
 *  pilots     complex64 [n_re][n_dmrs_total][n_layers], dense, the layout ce_dmrs_generate writes; slot b reads the tensor at
 *             element b * pilot_slot_stride (in complex elements, >= 0; 0 = one tensor for the whole batch).  8-byte aligned.
 *             Not read (may be NULL) where the plan has no DM-RS symbol.
 *  beta_dmrs  finite (CE_ERR_INVALID otherwise)
 *  rnti, n_id int32 device arrays; slot b reads element b * strides[0] / [1] of them (strides in elements, >= 0; 0 = one
 *             value for the whole batch).  They enter only the unsigned 32-bit arithmetic of c_init: an out-of-range value
 *             gives the sequence of the wrapped c_init and cannot address memory.  Not read (may be NULL, as may `strides`)
 *             by a plan without scrambling.
 *  tx         [slot][n_layers][n_sym][n_sc] complex64, dense
 * g and tx must be 16-byte aligned (CE_ERR_INVALID otherwise) and must not overlap.  No atomics, no scratch, plain vector
 * stores; every element of tx has one writer and nothing written is read.  Every address comes from the block index, the
 * thread index and host-derived plan values; the bits of g select a constellation level by arithmetic only.
 */
int ce_mod_modulate(const ce_mod_plan* plan, const uint8_t* g, const void* pilots, int64_t pilot_slot_stride, float beta_dmrs,
                    const int32_t* rnti, const int32_t* n_id, const int64_t strides[2], int64_t n_slots, void* tx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_MOD_H */

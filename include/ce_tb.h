/*
 * ce_tb.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: CRC checks and transport-block assembly
 * behind ce_ldpc_decode, the inverse of TS 38.212 5.1 (CRC attachment) and 5.2.2 (code-block segmentation).  It turns the
 * decoder's `hard[slot][C][row_bytes]` into what a MAC layer takes from PUSCH: the transport block and the residue of its
 * CRC.  All section numbers are TS 38.212.
 *
 * The reference (pjookim/srsran-ce-pytorch) stops at the channel estimate.  The operator is pinned by the literal
 * restatement of the specification's loops in tests/tb_oracle.py; all arithmetic is integer and results are compared by
 * value, without a tolerance.
 *
 * CRCs (5.1): zero initial state, MSB first, no final XOR.  Generator polynomials without the leading term:
 *     g24A = 0x864CFB   g24B = 0x800063   g16 = 0x1021
 * crc_g(bits) is the remainder of bits(x) x^L divided by g, so a bit string that carries its own CRC at its end has
 * residue 0.
 *
 * Host derivation (ce_tb_derive_host, integers only; A = tbs):
 *     L_tb = 24, g_tb = g24A if A > 3824, else L_tb = 16, g_tb = g16;  B = A + L_tb                         (5.1, 6.2.1)
 *     K_cb, C, B', K' exactly as in ce_rm.h (one function computes them for both stages)                      (5.2.2)
 *     L_cb = 24 if C > 1, else 0;  P = K' - L_cb = B / C, the payload bits of a code block
 * Any A >= 1 with B mod C = 0 is a plan; K' and P need not be multiples of 8.
 *
 * Operator, per slot.  Bit i < K' of block r is bit 7 - (i mod 8) of byte floor(i / 8) of hard[slot][r][.] (MSB first);
 * bits >= K' of a row are ignored, whatever they hold.  With p_r = bits [0, P) of block r:
 *     s = p_0 | p_1 | .. | p_{C-1}, B bits;  the transport block is s[0 .. A), the last L_tb bits of s are its CRC
 *     tb[slot][.]            bit i < A is s_i, MSB first; every bit from A to the end of the row is 0
 *     cb_status[slot][r][0]  C > 1: crc_24B(bits [0, K') of block r);  C = 1: crc_tb(s).  0 = the block is good
 *     cb_status[slot][r][1]  t_r = (p_r(x) x^(L_tb + (C - 1 - r) P)) mod g_tb: the block's share of crc_tb(s)
 *     tb_status[slot][0]     crc_tb(s) = XOR of t_r over r (the CRC is linear); 0 is the acknowledgement
 *     tb_status[slot][1]     the number of blocks whose cb_status[..][0] is nonzero
 * Residues are values, not pass bits, so corrupted inputs compare against the oracle too.
 */
#ifndef CE_TB_H
#define CE_TB_H

#include "ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_TB_G24A 8801531   /* 0x864CFB */
#define CE_TB_G24B 8388707   /* 0x800063 */
#define CE_TB_G16 4129       /* 0x1021 */
#define CE_TB_THREADS 256    /* one wave of 64 lanes per code block */
#define CE_TB_MAX_PIECE 5    /* dwords of a row per lane: ceil(in_row_bytes / 256), 5 at K' = 8448 */

typedef struct ce_tb_desc {
  int32_t abi_version; /* = CE_ABI_VERSION */
  int32_t device;      /* HIP device ordinal the plan lives on */
  int32_t base_graph;  /* 1 or 2, as in ce_rm_desc */
  int32_t tbs;         /* A >= 1: transport block size in bits */
} ce_tb_desc;

typedef struct ce_tb_plan ce_tb_plan; /* opaque */

typedef struct ce_tb_info {
  int32_t n_code_blocks;  /* C */
  int32_t in_row_bytes;   /* bytes per block of `hard` */
  int32_t tb_row_bytes;   /* bytes per slot of `tb` */
  int32_t reserved0;
  int64_t bytes_per_slot; /* C * in_row_bytes in; tb_row_bytes + 8 C + 8 out */
} ce_tb_info;

/* What ce_tb_plan_create derives on the host: every value of the derivation above, and the launch geometry. */
typedef struct ce_tb_host_view {
  int32_t b;            /* B */
  int32_t k_cb;         /* K_cb */
  int32_t c;            /* C */
  int32_t b_prime;      /* B' */
  int32_t k_prime;      /* K' */
  int32_t l_tb;         /* 24 or 16 */
  int32_t l_cb;         /* 24 or 0 */
  int32_t p;            /* P: payload bits per block */
  int32_t g_tb;         /* g24A or g16 */
  int32_t g_cb;         /* g24B (not used when C = 1) */
  int32_t in_row_bytes; /* 16 ceil(K' / 128): ce_ldpc_decode's row_bytes at k_out = K' */
  int32_t tb_row_bytes; /* 16 ceil(A / 128) */
  int32_t piece_dwords; /* ceil(in_row_bytes / 256) <= CE_TB_MAX_PIECE: the dwords of a row one lane runs through the CRCs */
  int32_t threads;      /* CE_TB_THREADS */
  int32_t blocks_per_workgroup;  /* threads / 64: the assemble launch has ceil(n_slots C / blocks_per_workgroup) workgroups */
  int32_t lds_bytes;    /* the CRC tables of one workgroup */
  int32_t fold_slots_per_workgroup; /* C > 1: the fold launch has ceil(n_slots / this) workgroups; 0 when C = 1 (no fold launch) */
  int32_t power_bytes;  /* the plan's device buffer: 256 (C + 1), host-derived powers of x modulo the two polynomials */
} ce_tb_host_view;

/* Validation and integer derivation of ce_tb_plan_create without touching a GPU: usable on a CPU-only host.
 * CE_ERR_INVALID with a text naming the field: ABI version; base_graph neither 1 nor 2; tbs < 1; B mod C != 0; K' > K_b 384
 * -- whatever ce_rm_derive_host refuses for a (base_graph, tbs) pair is refused here with the same text. */
int ce_tb_derive_host(const ce_tb_desc* desc, ce_tb_host_view* view);

/* Validates the descriptor and uploads the powers of x (power_bytes of device memory). */
int ce_tb_plan_create(const ce_tb_desc* desc, ce_tb_plan** out);
void ce_tb_plan_destroy(ce_tb_plan* plan);
int ce_tb_plan_get_info(const ce_tb_plan* plan, ce_tb_info* info);

/*
 * CRC checks and assembly of n_slots slots on `stream` (a hipStream_t; NULL = the default stream): one launch over all
 * n_slots * C code blocks and, for C > 1, one small launch behind it that folds cb_status into tb_status.  Asynchronous;
 * n_slots == 0 launches nothing.
 *  hard       [slot][C][in_row_bytes] uint8, dense: ce_ldpc_decode's output at k_out = K'
 *  tb         [slot][tb_row_bytes] uint8
 *  tb_status  [slot][2] int32
 *  cb_status  [slot][C][2] int32
 * All four must be 16-byte aligned (CE_ERR_INVALID otherwise) and must not overlap.  No atomics, no scratch, no workspace
 * beyond these outputs, no read-modify-write of output memory: every byte of tb, cb_status and tb_status is written by
 * exactly one thread.  Global addresses come from the block index, the thread index and host-derived plan values only; the
 * one data-dependent address is an index into a CRC table in LDS, masked to the table's size.
 */
int ce_tb_assemble(const ce_tb_plan* plan, const uint8_t* hard, int64_t n_slots, uint8_t* tb, int32_t* tb_status, int32_t* cb_status,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_TB_H */

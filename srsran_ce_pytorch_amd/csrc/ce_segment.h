// Code-block segmentation of TS 38.212 5.2.2, the lifting size of 5.3.2 and the choice of CRCs as integers on the host:
// what rate recovery (ce_rm), transport-block assembly (ce_tb) and the encoder (ce_enc) derive from (base graph, A) alike.
// One definition, so the stages cannot disagree on C, K', the polynomials or which sizes they refuse.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "ce_plan.h"
#include "ce_tb.h"

struct CeSegment {
  int64_t b;        // B = A + L_tb
  int64_t k_cb;     // K_cb
  int64_t c;        // C
  int64_t b_prime;  // B'
  int64_t k_prime;  // K'
  int64_t k_b;      // K_b
  int64_t zc;       // Zc
  int64_t k;        // K
  int64_t n;        // N
};

// base_graph is 1 or 2 and tbs >= 1 (the caller has checked both).  CE_ERR_INVALID: B mod C != 0; K' > K_b 384.
inline int ce_segment_derive(int32_t base_graph, int32_t tbs, CeSegment* s) {
  const bool bg1 = base_graph == 1;
  const int64_t A = tbs, B = A + (A > 3824 ? 24 : 16), K_cb = bg1 ? 8448 : 3840;
  const int64_t C = B <= K_cb ? 1 : (B + K_cb - 25) / (K_cb - 24);
  const int64_t Bp = C == 1 ? B : B + 24 * C;
  if (B % C != 0) return ce_fail(CE_ERR_INVALID, "tbs=%d: B=%lld is no multiple of C=%lld code blocks", tbs, (long long)B, (long long)C);
  const int64_t Kp = Bp / C;
  const int64_t K_b = bg1 ? 22 : B > 640 ? 10 : B > 560 ? 9 : B > 192 ? 8 : 6;
  if (Kp > K_b * 384) return ce_fail(CE_ERR_INVALID, "K'=%lld exceeds K_b * 384 = %lld", (long long)Kp, (long long)(K_b * 384));
  int64_t Zc = 0;
  for (int a : {2, 3, 5, 7, 9, 11, 13, 15})
    for (int64_t z = a; z <= 384; z *= 2)
      if (K_b * z >= Kp && (Zc == 0 || z < Zc)) Zc = z;
  s->b = B;
  s->k_cb = K_cb;
  s->c = C;
  s->b_prime = Bp;
  s->k_prime = Kp;
  s->k_b = K_b;
  s->zc = Zc;
  s->k = (bg1 ? 22 : 10) * Zc;
  s->n = (bg1 ? 66 : 50) * Zc;
  return CE_OK;
}

// The CRCs of 5.1 and 5.2.2 that go with a segmentation of C blocks of K' bits: what transport-block assembly checks and
// the encoder attaches.
struct CeCrcSelect {
  int32_t l_tb, l_cb;     // L_tb: 24 for A > 3824, else 16; the code blocks' L: 24 for C > 1, else 0 (no CRC24B)
  int32_t p;              // payload bits of a code block, K' - l_cb
  int32_t g_tb, g_cb;     // the polynomials without their leading term (CE_TB_G24A or CE_TB_G16; CE_TB_G24B)
  int32_t tb_row_bytes;   // the A bits of a transport block in whole 16-byte pieces
};

inline CeCrcSelect ce_crc_select(int32_t tbs, int64_t c, int64_t k_prime) {
  const bool crc24 = tbs > 3824;
  CeCrcSelect s;
  s.l_tb = crc24 ? 24 : 16;
  s.l_cb = c > 1 ? 24 : 0;
  s.p = (int32_t)k_prime - s.l_cb;
  s.g_tb = crc24 ? CE_TB_G24A : CE_TB_G16;
  s.g_cb = CE_TB_G24B;
  s.tb_row_bytes = 16 * (int32_t)(((int64_t)tbs + 127) / 128);
  return s;
}

// floor(a / d) and a - d floor(a / d) for a < 2^24 and d >= 1, inv = float32(1 / d): the product is within one of the
// quotient, one correction step either way makes it exact.  The index arithmetic of bit selection and interleaving in
// rate recovery (ce_rm.hip) and the encoder (ce_enc.hip).
__host__ __device__ __forceinline__ void ce_divmod(uint32_t a, uint32_t d, float inv, uint32_t& quo, uint32_t& rem) {
  uint32_t q = (uint32_t)((float)a * inv);
  int32_t m = (int32_t)a - (int32_t)(q * d);
  if (m < 0) {
    --q;
    m += (int32_t)d;
  } else if (m >= (int32_t)d) {
    ++q;
    m -= (int32_t)d;
  }
  quo = q;
  rem = (uint32_t)m;
}

// Code-block segmentation of TS 38.212 5.2.2 and the lifting size of 5.3.2 as integers on the host: what rate recovery
// (ce_rm) and transport-block assembly (ce_tb) derive from (base graph, A) alike.  One definition, so the two stages
// cannot disagree on C, K' or which sizes they refuse.
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "ce_plan.h"

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

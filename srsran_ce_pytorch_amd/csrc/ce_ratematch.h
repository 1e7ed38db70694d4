// Rate matching of TS 38.212 5.4.2 and 5.5 as integers on the host, and the words of it a kernel walks: how the G bits of
// a slot are split into the code blocks' E_r, and how a block's E_r bits walk its circular buffer of N_cb positions round
// the fillers from the redundancy version's k0.  Rate recovery (ce_rm) walks it backwards and the encoder (ce_enc)
// forwards.  One definition, so the two cannot disagree on a position or on what they refuse.
#pragma once
#include "ce_rm.h"
#include "ce_segment.h"

struct CeRateMatch {
  CeSegment seg;
  int32_t n_cb;          // N_cb
  int32_t f0, f1;        // filler positions [f0, f1) of the circular buffer
  int32_t p;             // P = N_cb - (f1 - f0): non-filler positions of one turn
  int32_t n_lo;          // blocks r < n_lo have E_r = e_lo, the others e_hi
  int32_t e_lo, e_hi;
  int32_t k0[4], s[4];   // per rv: k0, and its rank among the non-filler positions (f0 where k0 is a filler position)
};

// The checks and values that depend on these six inputs alone; a refused input leaves *m undefined.
__attribute__((visibility("hidden")))   // one copy in the library, no exported symbol
inline int ce_ratematch_derive(int32_t base_graph, int32_t tbs, int32_t qm, int32_t n_layers, int32_t g_bits, int32_t n_ref, CeRateMatch* m) {
  if (base_graph != 1 && base_graph != 2) return ce_fail(CE_ERR_INVALID, "base_graph=%d is neither 1 nor 2", base_graph);
  if (qm != 2 && qm != 4 && qm != 6 && qm != 8) return ce_fail(CE_ERR_INVALID, "qm=%d: modulation orders 2, 4, 6 and 8 are supported", qm);
  if (n_layers < 1 || n_layers > 4) return ce_fail(CE_ERR_INVALID, "n_layers=%d outside 1..4", n_layers);
  if (tbs < 1) return ce_fail(CE_ERR_INVALID, "tbs=%d must be positive", tbs);
  if (n_ref < 0) return ce_fail(CE_ERR_INVALID, "n_ref=%d is negative", n_ref);
  const bool bg1 = base_graph == 1;
  CeSegment& seg = m->seg;   // 5.2.2 and the lifting size: shared with ce_tb
  if (const int rc = ce_segment_derive(base_graph, tbs, &seg); rc != CE_OK) return rc;
  const int64_t C = seg.c, Zc = seg.zc;
  if (n_ref != 0 && n_ref < seg.k - 2 * Zc) return ce_fail(CE_ERR_INVALID, "n_ref=%d is below K - 2 Zc = %lld", n_ref, (long long)(seg.k - 2 * Zc));
  const int64_t N_cb = n_ref == 0 ? seg.n : (seg.n < n_ref ? seg.n : (int64_t)n_ref);
  const int64_t f0 = seg.k_prime - 2 * Zc, f1 = seg.k - 2 * Zc, P = N_cb - (f1 - f0);
  if (f0 < 0 || P < 1) return ce_fail(CE_ERR_INVALID, "tbs=%d: no transmittable position in the circular buffer", tbs);
  const int64_t lq = (int64_t)n_layers * qm, G = g_bits;
  if (G < 1 || G % lq != 0) return ce_fail(CE_ERR_INVALID, "g_bits=%d is no positive multiple of n_layers * qm = %lld", g_bits, (long long)lq);
  if (G > CE_DEMOD_MAX_BITS) return ce_fail(CE_ERR_INVALID, "g_bits=%d: more than %d bits per slot", g_bits, CE_DEMOD_MAX_BITS);
  const int64_t q = G / lq;
  if (q < C) return ce_fail(CE_ERR_INVALID, "g_bits=%d: %lld symbols per layer for %lld code blocks", g_bits, (long long)q, (long long)C);
  if (C * N_cb > CE_RM_MAX_SLOT_ELEMS) return ce_fail(CE_ERR_UNSUPPORTED, "%lld code blocks of %lld positions: more than %d outputs per slot", (long long)C, (long long)N_cb, CE_RM_MAX_SLOT_ELEMS);
  m->n_cb = (int32_t)N_cb;
  m->f0 = (int32_t)f0;
  m->f1 = (int32_t)f1;
  m->p = (int32_t)P;
  m->n_lo = (int32_t)(C - q % C);
  m->e_lo = (int32_t)(lq * (q / C));
  m->e_hi = (int32_t)(lq * ((q + C - 1) / C));
  const int num1[4] = {0, 17, 33, 56}, num2[4] = {0, 13, 25, 43};
  for (int i = 0; i < 4; ++i) {
    const int64_t k0 = (bg1 ? num1[i] : num2[i]) * N_cb / ((bg1 ? 66 : 50) * Zc) * Zc;
    m->k0[i] = (int32_t)k0;
    m->s[i] = (int32_t)(k0 < f0 ? k0 : k0 < f1 ? f0 : k0 - (f1 - f0));
  }
  return CE_OK;
}

// Into a public host view (ce_rm_host_view, ce_enc_host_view): the members the two name alike, which is all but P.
template <class View>
void ce_ratematch_view(const CeRateMatch& m, View* v) {
  v->b = (int32_t)m.seg.b, v->k_cb = (int32_t)m.seg.k_cb, v->c = (int32_t)m.seg.c, v->b_prime = (int32_t)m.seg.b_prime;
  v->k_prime = (int32_t)m.seg.k_prime, v->k_b = (int32_t)m.seg.k_b, v->zc = (int32_t)m.seg.zc, v->k = (int32_t)m.seg.k, v->n = (int32_t)m.seg.n;
  v->n_cb = m.n_cb, v->f0 = m.f0, v->f1 = m.f1, v->n_lo = m.n_lo, v->e_lo = m.e_lo, v->e_hi = m.e_hi;
  for (int i = 0; i < 4; ++i) v->k0[i] = m.k0[i], v->s[i] = m.s[i];
}

// What a kernel reads of the walk.  Block r holds E_r = e_lo (r < n_lo) or e_hi bits of the slot's row, from bit r e_lo or
// base_hi + (r - n_lo) e_hi on; bit k of them is f_{i Qm + j} with j = floor(k / (E_r / Qm)), i = k mod (E_r / Qm), and
// stands at the non-filler position of rank (s + k) mod P, position rank + nf from f0 on.
struct RmWalkDev {
  uint32_t qm, g, f0, nf, p;        // Qm, G, fillers [f0, f0 + nf), P
  uint32_t s0, s1, s2, s3;          // per rv: the rank the walk starts at
  uint32_t n_lo, e_lo, e_hi;
  uint32_t eq_lo, eq_hi, base_hi;   // E_r / Qm; base_hi = n_lo * e_lo, the first bit of block n_lo
};

inline RmWalkDev ce_rm_walk_dev(const CeRateMatch& m, int32_t qm, int32_t g_bits) {
  RmWalkDev W;
  W.qm = (uint32_t)qm, W.g = (uint32_t)g_bits, W.f0 = (uint32_t)m.f0, W.nf = (uint32_t)(m.f1 - m.f0), W.p = (uint32_t)m.p;
  W.s0 = (uint32_t)m.s[0], W.s1 = (uint32_t)m.s[1], W.s2 = (uint32_t)m.s[2], W.s3 = (uint32_t)m.s[3];
  W.n_lo = (uint32_t)m.n_lo, W.e_lo = (uint32_t)m.e_lo, W.e_hi = (uint32_t)m.e_hi;
  W.eq_lo = W.e_lo / W.qm, W.eq_hi = W.e_hi / W.qm, W.base_hi = W.n_lo * W.e_lo;
  return W;
}

// The rank the walk of redundancy version rv & 3 starts at.  P is the kernel's argument block, which embeds the words as
// `rm`: handed P.rm alone, the compiler loads the encoder's kernel arguments in another order and schedules differently.
template <class Dev>
__device__ __forceinline__ uint32_t ce_rm_walk_start(const Dev& P, uint32_t rv) {
  const uint32_t b = rv & 3u;
  return b == 0u ? P.rm.s0 : b == 1u ? P.rm.s1 : b == 2u ? P.rm.s2 : P.rm.s3;
}

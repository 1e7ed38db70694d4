// EXTENSION (no reference counterpart, see include/ce_dmrs.h): the low-PAPR PUSCH DM-RS of DFT-s-OFDM, a Zadoff-Chu base
// sequence with group or sequence hopping (TS 38.211 6.4.1.1.1.2, 5.2.2), in the [slot][n_re][n_dmrs_total][1] layout
// ce_estimate_batch consumes.
//
// Everything but a gather is integer work derived on the host.  A pilot is W_N[e] with e = (q tri[k]) mod N:
//     W_N     the N-th roots of unity, evaluated in double on the host and rounded once (the phase pi q t (t + 1) / N
//             formed in float32 would be off by 0.63 at 273 PRB; the index never leaves the integers)
//     tri[k]  t (t + 1) / 2 mod N, t = k mod N -- per row, host-derived
//     q       q[u][v], 60 values -- host-derived; (u, v) come from the hopping bits of the Gold sequence, which is linear
//             over GF(2) in c_init: word w of c is row 0 of the table XOR the rows 1 + i of the set bits i of c_init, the
//             construction of ce_dmrs.hip
// The length-30 form is the same gather with N = 31, q = u + 1 and tri[k] = (k + 1) (k + 2) / 2 mod 31; the table form
// (M_ZC <= 24) gathers one of four values by the caller's phi_u(k).
//
// Kernel: one 256-thread workgroup per slot.
//   1. the workgroup copies W_N into the LDS (<= 16 KB, consecutive threads consecutive entries) -- the gather that follows is
//      element-granular and would cost a cache line per lane from L2; from the LDS it costs bank conflicts only;
//   2. 32 threads per DM-RS column load the 32 table rows of the column's hopping word (row i + 1 only where bit i of
//      c_init is set); barrier; one thread per column folds them and derives (u, v, q); barrier;
//   3. the workgroup walks the slot's output in memory order (k, s), one 16-byte store per thread and step where the
//      slot's element count is even.
// The per-slot parameters enter as slot mod slots_per_frame, n_id mod 30 and the bits of c_init: the one index they form,
// the hopping word's, is below the table's row length for every value.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ce_dmrs.h"
#include "ce_gold.h"
#include "ce_stage.h"

namespace {

constexpr int LP_NT = 256;
constexpr int LP_MAX_N = CE_DMRS_MAX_RE;   // N_ZC < M_ZC <= CE_DMRS_MAX_RE
constexpr uint32_t LP_A = 0x3f3504f3u;     // float32 0.70710677

struct LpDev {
  uint32_t n_re, n_cols, n_elem;    // pilots per column; columns; elements per slot
  uint32_t col_magic;               // floor(2^32 / n_cols) + 1 (n_cols > 1): e / n_cols = umulhi(e, col_magic), e n_cols < 2^32
  uint32_t form, n, n_magic;        // CE_DMRS_LP_FORM_*; N; floor(2^32 / N)
  uint32_t n_w;                     // entries of the gather table (N, or 4 in the table form)
  uint32_t hopping, v_live, n_symb_slot, slots_per_frame, nw;   // nw: words per row of the hopping table
  uint32_t sym[CE_MAX_SYMBOLS];     // per column: OFDM symbol index
};

// Everything a plan holds, as the host derives it.
struct LpHost {
  LpDev dev{};
  int n_prb = 0;
  int col_sym[CE_MAX_SYMBOLS] = {0};
  std::vector<int32_t> q;           // [30][2]
  std::vector<uint16_t> tri;        // [n_re]
  std::vector<uint8_t> code;        // table form: [30][n_re], index into the four values
  std::vector<uint32_t> hop;        // [32][nw]
};

}  // namespace

struct ce_dmrs_lp_plan {
  int device = 0;
  LpDev dev{};
  float2* w = nullptr;       // [n_w]
  uint16_t* qtab = nullptr;  // [60]
  uint16_t* tri = nullptr;   // [n_re]
  uint8_t* code = nullptr;   // [30][n_re] (table form)
  uint32_t* hop = nullptr;   // [32][nw]
};

namespace {

// x mod n for any 32-bit x: the quotient estimate umulhi(x, floor(2^32 / n)) is the true one or one less
// (x / n - x / 2^32 - 1 < estimate <= x / n), so one conditional subtraction finishes it.
__device__ __forceinline__ uint32_t lp_mod(uint32_t x, uint32_t n, uint32_t n_magic) {
  const uint32_t r = x - __umulhi(x, n_magic) * n;
  return r >= n ? r - n : r;
}

__device__ __forceinline__ float2 lp_value(const LpDev& P, const float2* w, const uint32_t* qs, const uint16_t* __restrict__ tri,
                                           const uint8_t* __restrict__ code, uint32_t k, uint32_t s) {
  if (P.form == CE_DMRS_LP_FORM_PHI) return w[code[qs[s] * P.n_re + k] & 3u];   // qs = u < 30
  return w[lp_mod(qs[s] * (uint32_t)tri[k], P.n, P.n_magic)];                   // q <= N, tri < N: the product is below 2^22
}

template <bool VEC2>
__global__ __launch_bounds__(LP_NT) void ce_dmrs_lp_kernel(LpDev P, const float2* __restrict__ wtab, const uint16_t* __restrict__ qtab,
                                                           const uint16_t* __restrict__ tri, const uint8_t* __restrict__ code,
                                                           const uint32_t* __restrict__ hop, const int32_t* __restrict__ slot,
                                                           const int32_t* __restrict__ n_id, int64_t st_slot, int64_t st_id,
                                                           float2* __restrict__ out) {
  __shared__ float2 w[LP_MAX_N];
  __shared__ uint32_t hw[CE_MAX_SYMBOLS * 32];
  __shared__ uint32_t qs[CE_MAX_SYMBOLS];
  const uint32_t tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const uint32_t u_slot = (uint32_t)slot[b * st_slot] % P.slots_per_frame, u_id = (uint32_t)n_id[b * st_id];
  for (uint32_t i = tid; i < P.n_w; i += LP_NT) w[i] = wtab[i];
  if (P.hopping != CE_DMRS_LP_HOP_NEITHER) {
    const bool group = P.hopping == CE_DMRS_LP_HOP_GROUP;
    const uint32_t c_init = (group ? u_id / 30u : u_id) & 0x7FFFFFFFu;
    for (uint32_t j = tid; j < P.n_cols * 32u; j += LP_NT) {
      const uint32_t col = j >> 5, i = j & 31u;
      const uint32_t p = P.n_symb_slot * u_slot + P.sym[col];   // < n_symb_slot * slots_per_frame
      const uint32_t wi = group ? p >> 2 : p >> 5;              // < nw (host: nw = ceil of that bound / 4 or / 32)
      hw[j] = i == 0 ? hop[wi] : (((c_init >> (i - 1u)) & 1u) ? hop[i * P.nw + wi] : 0u);
    }
  }
  __syncthreads();
  if (tid < P.n_cols) {
    uint32_t f_gh = 0, v = 0;
    if (P.hopping != CE_DMRS_LP_HOP_NEITHER) {
      uint32_t x = 0;
      for (uint32_t i = 0; i < 32; ++i) x ^= hw[tid * 32u + i];
      const uint32_t p = P.n_symb_slot * u_slot + P.sym[tid];
      if (P.hopping == CE_DMRS_LP_HOP_GROUP)
        f_gh = ((x >> (8u * (p & 3u))) & 0xFFu) % 30u;
      else
        v = P.v_live ? (x >> (p & 31u)) & 1u : 0u;
    }
    const uint32_t u = (f_gh + u_id % 30u) % 30u;
    qs[tid] = P.form == CE_DMRS_LP_FORM_PHI ? u : qtab[2u * u + v];
  }
  __syncthreads();
  float2* __restrict__ o = out + b * (int64_t)P.n_elem;
  if (VEC2) {   // n_elem even and `out` 16-byte aligned (host)
    float4* __restrict__ o4 = reinterpret_cast<float4*>(o);
    for (uint32_t pr = tid; pr < P.n_elem / 2; pr += LP_NT) {
      const uint32_t e = 2 * pr;
      const uint32_t k0 = P.n_cols > 1 ? __umulhi(e, P.col_magic) : e;
      const uint32_t s0 = e - k0 * P.n_cols;
      const bool wrap = s0 + 1 == P.n_cols;          // n_elem is even: k0 + 1 < n_re where the pair wraps
      const uint32_t k1 = wrap ? k0 + 1 : k0, s1 = wrap ? 0u : s0 + 1;
      const float2 v0 = lp_value(P, w, qs, tri, code, k0, s0), v1 = lp_value(P, w, qs, tri, code, k1, s1);
      o4[pr] = make_float4(v0.x, v0.y, v1.x, v1.y);
    }
  } else {
    for (uint32_t e = tid; e < P.n_elem; e += LP_NT) {
      const uint32_t k = P.n_cols > 1 ? __umulhi(e, P.col_magic) : e;
      o[e] = lp_value(P, w, qs, tri, code, k, e - k * P.n_cols);
    }
  }
}

// ---- host derivation: integers only ----

int lp_largest_prime_below(int m) {
  for (int n = m - 1; n >= 2; --n) {
    bool prime = true;
    for (int d = 2; d * d <= n && prime; ++d) prime = n % d != 0;
    if (prime) return n;
  }
  return 0;
}

int lp_derive(int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot, int32_t n_layers, int32_t n_hops, const uint8_t* dmrs_symbols,
              const uint16_t* re_mask, const uint8_t* mask_prbs, int32_t hopping, int32_t slots_per_frame, const int8_t* phi, LpHost* H) {
  if (!dmrs_symbols || !re_mask || !mask_prbs) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_layers != 1) return ce_fail(CE_ERR_UNSUPPORTED, "n_layers=%d: low-PAPR DM-RS is single-layer (transform precoding)", n_layers);
  if (n_hops < 1 || n_hops > CE_MAX_HOPS) return ce_fail(CE_ERR_INVALID, "n_hops=%d outside 1..2", n_hops);
  if (n_prb_grid < 1 || 12 * n_prb_grid > CE_FFT_SIZE) return ce_fail(CE_ERR_UNSUPPORTED, "grid of %d PRB: 12*n_prb must be in 12..%d", n_prb_grid, CE_FFT_SIZE);
  if (n_symb_slot != 12 && n_symb_slot != 14) return ce_fail(CE_ERR_INVALID, "n_symb_slot=%d, expected 14 or 12", n_symb_slot);
  if (n_sym < 1 || n_sym > n_symb_slot) return ce_fail(CE_ERR_INVALID, "n_sym=%d outside 1..n_symb_slot=%d", n_sym, n_symb_slot);
  if (hopping != CE_DMRS_LP_HOP_NEITHER && hopping != CE_DMRS_LP_HOP_GROUP && hopping != CE_DMRS_LP_HOP_SEQUENCE)
    return ce_fail(CE_ERR_INVALID, "hopping=%d is not one of neither (0), group (1), sequence (2)", hopping);
  if (slots_per_frame != 10 && slots_per_frame != 20 && slots_per_frame != 40 && slots_per_frame != 80 && slots_per_frame != 160)
    return ce_fail(CE_ERR_INVALID, "slots_per_frame=%d, expected 10, 20, 40, 80 or 160", slots_per_frame);
  LpDev& P = H->dev;
  int n_cols = 0, n_prb0 = 0;
  uint8_t seen_sym[CE_MAX_SYMBOLS] = {0};
  for (int h = 0; h < n_hops; ++h) {
    if (re_mask[h] != 0x555u && re_mask[h] != 0xAAAu)
      return ce_fail(CE_ERR_INVALID, "hop %d: re_mask=0x%03x is not a configuration type 1 mask (0x555 0xAAA)", h, re_mask[h]);
    const int col0 = n_cols;
    for (int s = 0; s < n_sym; ++s)
      if (dmrs_symbols[h * CE_MAX_SYMBOLS + s]) {
        if (seen_sym[s]) return ce_fail(CE_ERR_INVALID, "Hops should not overlap.");
        seen_sym[s] = 1;
        H->col_sym[n_cols] = s;
        P.sym[n_cols] = (uint32_t)s;
        ++n_cols;
      }
    if (n_cols == col0) return ce_fail(CE_ERR_INVALID, "hop %d has no DM-RS symbol", h);
    const uint8_t* mp = mask_prbs + (size_t)h * n_prb_grid;
    int n_active = 0, first = -1, last = -1;
    for (int p = 0; p < n_prb_grid; ++p)
      if (mp[p]) {
        if (first < 0) first = p;
        last = p;
        ++n_active;
      }
    if (n_active < 1) return ce_fail(CE_ERR_INVALID, "hop %d: mask_prbs has no active PRB", h);
    if (last - first + 1 != n_active)
      return ce_fail(CE_ERR_UNSUPPORTED, "hop %d: the %d active PRBs are not one contiguous run (the sequence length is that of a contiguous allocation)", h, n_active);
    if (h == 0) n_prb0 = n_active;
    if (n_active != n_prb0) return ce_fail(CE_ERR_INVALID, "hop %d has %d active PRBs, hop 0 has %d (one sequence length M_ZC for both)", h, n_active, n_prb0);
  }
  const int m_zc = 6 * n_prb0;   // <= 6 * 341 = 2046 <= CE_DMRS_MAX_RE
  H->n_prb = n_prb0;
  P.n_re = (uint32_t)m_zc;
  P.n_cols = (uint32_t)n_cols;
  P.n_elem = P.n_re * P.n_cols;
  P.col_magic = n_cols > 1 ? (uint32_t)(0x100000000ull / (uint32_t)n_cols) + 1u : 0u;   // exact for e n_cols < 2^32: e < 2^15, n_cols <= 14
  P.hopping = (uint32_t)hopping;
  P.n_symb_slot = (uint32_t)n_symb_slot;
  P.slots_per_frame = (uint32_t)slots_per_frame;
  P.v_live = hopping == CE_DMRS_LP_HOP_SEQUENCE && m_zc >= 72 ? 1u : 0u;
  H->q.assign(60, 0);
  H->tri.assign((size_t)m_zc, 0);
  if (m_zc >= 36) {
    const int n = lp_largest_prime_below(m_zc);   // > m_zc / 2: a row index wraps at most once
    P.form = CE_DMRS_LP_FORM_ZC;
    P.n = (uint32_t)n;
    for (int u = 0; u < 30; ++u)
      for (int v = 0; v < 2; ++v) {
        const int two_qbar = 2 * n * (u + 1);   // 31 * 2 q_bar
        H->q[2 * u + v] = (two_qbar + 31) / 62 + ((two_qbar / 31) % 2 == 0 ? v : -v);
      }
    for (int k = 0; k < m_zc; ++k) {
      const int64_t t = k % n;
      H->tri[k] = (uint16_t)((t * (t + 1) / 2) % n);
    }
  } else if (m_zc == 30) {
    P.form = CE_DMRS_LP_FORM_30;
    P.n = 31;
    for (int u = 0; u < 30; ++u) H->q[2 * u] = H->q[2 * u + 1] = u + 1;
    for (int k = 0; k < 30; ++k) H->tri[k] = (uint16_t)(((k + 1) * (k + 2) / 2) % 31);
  } else {
    if (!phi) return ce_fail(CE_ERR_UNSUPPORTED, "M_ZC=%d (%d PRB) needs the phi table of 38.211 5.2.2.2, which the caller provides", m_zc, n_prb0);
    P.form = CE_DMRS_LP_FORM_PHI;
    P.n = 0;
    H->code.assign((size_t)30 * m_zc, 0);
    for (int i = 0; i < 30 * m_zc; ++i) {
      const int f = phi[i];
      if (f != -3 && f != -1 && f != 1 && f != 3) return ce_fail(CE_ERR_INVALID, "phi[%d][%d]=%d is not one of -3, -1, 1, 3", i / m_zc, i % m_zc, f);
      H->code[i] = (uint8_t)((f + 3) / 2);   // -3, -1, 1, 3 -> 0 .. 3
    }
  }
  P.n_magic = P.n ? (uint32_t)(0x100000000ull / P.n) : 0u;
  P.n_w = P.form == CE_DMRS_LP_FORM_PHI ? 4u : P.n;
  const int n_pos = n_symb_slot * slots_per_frame;
  const int nw = hopping == CE_DMRS_LP_HOP_GROUP ? (n_pos + 3) / 4 : hopping == CE_DMRS_LP_HOP_SEQUENCE ? (n_pos + 31) / 32 : 0;   // <= CE_DMRS_LP_MAX_WORDS
  P.nw = (uint32_t)nw;
  H->hop.assign((size_t)32 * nw, 0u);
  if (nw) {
    ce_gold_words<false>(1u, 0, nw - 1, H->hop.data());
    for (int i = 0; i < 31; ++i) ce_gold_words<true>(1u << i, 0, nw - 1, H->hop.data() + (size_t)(1 + i) * nw);
  }
  return CE_OK;
}

// W_n[e] = (float32(cos th), float32(-sin th)), th = 2 pi e / n in double; W_n[0] = (1, +0).
void lp_twiddles(int n, float* w) {
  for (int e = 0; e < n; ++e) {
    const double th = 2.0 * M_PI * (double)e / (double)n;
    w[2 * e] = (float)cos(th);
    w[2 * e + 1] = e ? (float)-sin(th) : 0.0f;
  }
}

}  // namespace

extern "C" int ce_dmrs_lp_derive_host(int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot, int32_t n_layers, int32_t n_hops,
                                      const uint8_t* dmrs_symbols, const uint16_t* re_mask, const uint8_t* mask_prbs, int32_t hopping,
                                      int32_t slots_per_frame, const int8_t* phi, int32_t* info, int32_t* col_sym, int32_t* q, int32_t* tri,
                                      uint32_t* hop_words) {
  LpHost H;
  if (const int rc = lp_derive(n_prb_grid, n_sym, n_symb_slot, n_layers, n_hops, dmrs_symbols, re_mask, mask_prbs, hopping, slots_per_frame, phi, &H); rc != CE_OK) return rc;
  const LpDev& P = H.dev;
  if (info) {
    const int32_t v[CE_DMRS_LP_INFO_LEN] = {(int32_t)P.n_re, (int32_t)P.n_cols, (int32_t)P.form, (int32_t)P.n, (int32_t)P.nw, (int32_t)P.v_live, H.n_prb, 0};
    memcpy(info, v, sizeof(v));
  }
  if (col_sym) memcpy(col_sym, H.col_sym, sizeof(H.col_sym));
  if (q) memcpy(q, H.q.data(), 60 * sizeof(int32_t));
  if (tri) {
    memset(tri, 0, CE_DMRS_MAX_RE * sizeof(int32_t));
    for (uint32_t k = 0; k < P.n_re; ++k) tri[k] = H.tri[k];
  }
  if (hop_words && !H.hop.empty()) memcpy(hop_words, H.hop.data(), H.hop.size() * sizeof(uint32_t));
  return CE_OK;
}

extern "C" int ce_dmrs_lp_copy_twiddles(int32_t n, float* twiddles) {
  if (!twiddles) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n < 2 || n > LP_MAX_N) return ce_fail(CE_ERR_INVALID, "n=%d outside 2..%d", n, LP_MAX_N);
  lp_twiddles(n, twiddles);
  return CE_OK;
}

extern "C" int ce_dmrs_lp_plan_create(int32_t abi_version, int32_t device, int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot,
                                      int32_t n_layers, int32_t n_hops, const uint8_t* dmrs_symbols, const uint16_t* re_mask,
                                      const uint8_t* mask_prbs, int32_t hopping, int32_t slots_per_frame, const int8_t* phi,
                                      ce_dmrs_lp_plan** out) {
  if (!out) return ce_fail(CE_ERR_INVALID, "null argument");
  if (abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", abi_version, CE_ABI_VERSION);
  LpHost H;
  if (const int rc = lp_derive(n_prb_grid, n_sym, n_symb_slot, n_layers, n_hops, dmrs_symbols, re_mask, mask_prbs, hopping, slots_per_frame, phi, &H); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_dmrs_lp_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->device = device;
  p->dev = H.dev;
  const LpDev& P = H.dev;
  std::vector<float> w(2 * (size_t)P.n_w);
  if (P.form == CE_DMRS_LP_FORM_PHI) {   // code c <-> phi = 2 c - 3: exp(j phi pi / 4) = (+-a, +-a)
    const uint32_t neg = LP_A | 0x80000000u, re[4] = {neg, LP_A, LP_A, neg}, im[4] = {neg, neg, LP_A, LP_A};
    for (int c = 0; c < 4; ++c) {
      memcpy(&w[2 * c], &re[c], 4);
      memcpy(&w[2 * c + 1], &im[c], 4);
    }
  } else {
    lp_twiddles((int)P.n, w.data());
  }
  std::vector<uint16_t> qtab(60);
  for (int i = 0; i < 60; ++i) qtab[i] = (uint16_t)H.q[i];   // 0 <= q <= N
  if (H.code.empty()) H.code.assign(1, 0);                    // every table has an allocation behind its pointer
  if (H.hop.empty()) H.hop.assign(1, 0u);
  CeDeviceScope scope(device);
  hipError_t e = ce_upload(scope.err, &p->w, w.data(), w.size() * sizeof(float));
  e = ce_upload(e, &p->qtab, qtab.data(), qtab.size() * sizeof(uint16_t));
  e = ce_upload(e, &p->tri, H.tri.data(), H.tri.size() * sizeof(uint16_t));
  e = ce_upload(e, &p->code, H.code.data(), H.code.size());
  e = ce_upload(e, &p->hop, H.hop.data(), H.hop.size() * sizeof(uint32_t));
  if (e != hipSuccess) {
    ce_dmrs_lp_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "low-PAPR DM-RS plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_dmrs_lp_plan_destroy(ce_dmrs_lp_plan* p) {
  if (!p) return;
  if (p->w) (void)hipFree(p->w);
  if (p->qtab) (void)hipFree(p->qtab);
  if (p->tri) (void)hipFree(p->tri);
  if (p->code) (void)hipFree(p->code);
  if (p->hop) (void)hipFree(p->hop);
  delete p;
}

extern "C" int ce_dmrs_lp_generate(const ce_dmrs_lp_plan* p, const int32_t* slot, int64_t slot_stride, const int32_t* n_id,
                                   int64_t n_id_stride, int64_t n_slots, void* pilots_out, void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  if (!slot || !n_id || !pilots_out) return ce_fail(CE_ERR_INVALID, "null argument");
  if (slot_stride < 0 || n_id_stride < 0) return ce_fail(CE_ERR_INVALID, "negative strides are not supported");
  if ((reinterpret_cast<uintptr_t>(slot) & 3u) || (reinterpret_cast<uintptr_t>(n_id) & 3u)) return ce_fail(CE_ERR_INVALID, "slot and n_id must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(pilots_out) & 7u) return ce_fail(CE_ERR_INVALID, "pilots_out must be 8-byte aligned");
  if (n_slots > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "more than 2^31-1 slots in one launch");
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  const bool vec2 = p->dev.n_elem % 2 == 0 && (reinterpret_cast<uintptr_t>(pilots_out) & 15u) == 0;
  float2* out = reinterpret_cast<float2*>(pilots_out);
  const hipStream_t st = (hipStream_t)stream;
  if (vec2)
    hipLaunchKernelGGL((ce_dmrs_lp_kernel<true>), dim3((unsigned)n_slots), dim3(LP_NT), 0, st, p->dev, p->w, p->qtab, p->tri, p->code, p->hop, slot, n_id, slot_stride, n_id_stride, out);
  else
    hipLaunchKernelGGL((ce_dmrs_lp_kernel<false>), dim3((unsigned)n_slots), dim3(LP_NT), 0, st, p->dev, p->w, p->qtab, p->tri, p->code, p->hop, slot, n_id, slot_stride, n_id_stride, out);
  return ce_launch_status("low-PAPR DM-RS");
}

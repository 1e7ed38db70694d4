// What the row transforms (ce_tp.hip: transform de-precoding and precoding; ce_ofdm.hip: OFDM demodulation and modulation)
// share: on the device the row frame of a workgroup and the Stockham passes of one row in LDS, on the host the radix
// sequence, stride constants, launch geometry and twiddle table of a transform of any length 2^a 3^b 5^c and the part of a
// plan that holds them.  The loads and stores differ per kernel and stay there.  Internal; everything here has internal
// linkage.
//
//   frame  one 256-thread workgroup handles rows_per_workgroup rows of one item (a slot, or a (slot, port)),
//          threads_per_row = 64, 128 or 256 threads each: whole waves, so everything that depends on the row is
//          wave-uniform.  A row lives in two LDS buffers of M complex64 from the load to the store.
//   passes Stockham autosort, decimation in frequency, radix sequence r_0 r_1 .. from the host: at stride s (the product
//          of the radices before) butterfly i < M / r reads src[i + k M / r], k < r, takes the r-point inverse DFT,
//          multiplies output j by W[p j s] with p = floor(i / s) (one table of M twiddles for every pass, since the
//          pass's own root of unity is W^s; p j s < M) and writes dst[(i - p s) + s (r p + j)].  The reads are contiguous
//          over the lanes; the division is one v_mul_hi with a host-derived constant.  One barrier per pass.  The last
//          pass has p = 0 (no twiddles), applies the caller's scale and leaves the row in natural order.
// The transform is the INVERSE one, y_i = sum_k x_k exp(+j 2 pi i k / M); a forward transform runs it between two
// conjugations.  DESIGN 6i.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ce_stage.h"
#include "ce_tp.h"

namespace {

constexpr int TP_NT = 256;   // threads of a workgroup: 1, 2 or 4 rows of 256, 128 or 64 threads

// The plan values of the frame and the passes: the first member of every kernel's own argument block.
struct FftDev {
  uint32_t m;             // transform length M (N in ce_ofdm.hip)
  uint32_t n_rows;        // rows per item
  uint32_t tpr_log2;      // log2(threads_per_row)
  uint32_t rpw;           // rows per workgroup
  uint32_t wg_per_item;   // workgroups per item
  uint32_t n_passes;
  uint32_t radix[CE_TP_MAX_PASSES];
  uint32_t magic[CE_TP_MAX_PASSES];
};

// What a thread works on: row `row` of item `item` as thread `lane` of the row's `tpr`, between `buf0` and `buf1`.
struct FftRow {
  uint32_t item, row, lane, tpr;
  bool active;   // row < n_rows: the item's last workgroup may hold fewer rows
  float2 *buf0, *buf1;
};

// `lds`: the workgroup's dynamic LDS, rows_per_workgroup * 2 * M complex64.
__device__ __forceinline__ FftRow fft_row(const FftDev& P, float4* lds) {
  const uint32_t tpr = 1u << P.tpr_log2, item = blockIdx.x / P.wg_per_item, wg = blockIdx.x - item * P.wg_per_item;
  const uint32_t rl = threadIdx.x >> P.tpr_log2, row = wg * P.rpw + rl;   // rl: row of the workgroup (wave-uniform)
  float2* buf0 = reinterpret_cast<float2*>(lds) + (size_t)rl * 2u * P.m;
  return {item, row, threadIdx.x & (tpr - 1u), tpr, row < P.n_rows, buf0, buf0 + P.m};
}

__device__ __forceinline__ float2 operator+(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 operator-(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 operator*(float c, float2 a) { return make_float2(c * a.x, c * a.y); }
__device__ __forceinline__ float2 tp_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
// a + j b and a - j b
__device__ __forceinline__ float2 tp_add_j(float2 a, float2 b) { return make_float2(a.x - b.y, a.y + b.x); }
__device__ __forceinline__ float2 tp_sub_j(float2 a, float2 b) { return make_float2(a.x + b.y, a.y - b.x); }

// y_j = sum_k x_k exp(+j 2 pi j k / R)
template <int R>
__device__ __forceinline__ void tp_butterfly(const float2 (&x)[R], float2 (&y)[R]) {
  if constexpr (R == 2) {
    y[0] = x[0] + x[1];
    y[1] = x[0] - x[1];
  } else if constexpr (R == 4) {
    const float2 t0 = x[0] + x[2], t1 = x[0] - x[2], t2 = x[1] + x[3], t3 = x[1] - x[3];
    y[0] = t0 + t2;
    y[1] = tp_add_j(t1, t3);
    y[2] = t0 - t2;
    y[3] = tp_sub_j(t1, t3);
  } else if constexpr (R == 3) {
    const float2 t = x[1] + x[2], u = x[1] - x[2];
    const float2 m = x[0] - 0.5f * t, v = 0.8660254037844386f * u;
    y[0] = x[0] + t;
    y[1] = tp_add_j(m, v);
    y[2] = tp_sub_j(m, v);
  } else {
    static_assert(R == 5, "radices 2, 3, 4 and 5");
    constexpr float c1 = 0.30901699437494745f, c2 = -0.8090169943749475f, s1 = 0.9510565162951535f, s2 = 0.5877852522924731f;
    const float2 t1 = x[1] + x[4], t2 = x[2] + x[3], u1 = x[1] - x[4], u2 = x[2] - x[3];
    const float2 m1 = (x[0] + c1 * t1) + c2 * t2, m2 = (x[0] + c2 * t1) + c1 * t2;
    const float2 n1 = s1 * u1 + s2 * u2, n2 = s2 * u1 - s1 * u2;
    y[0] = (x[0] + t1) + t2;
    y[1] = tp_add_j(m1, n1);
    y[2] = tp_add_j(m2, n2);
    y[3] = tp_sub_j(m2, n2);
    y[4] = tp_sub_j(m1, n1);
  }
}

// One pass over one row: `nb` = M / R butterflies at stride `s`; magic = floor(2^32 / s) + 1, or 0 where s = 1.
template <int R, bool LAST>
__device__ __forceinline__ void tp_pass(const float2* src, float2* dst, const float2* __restrict__ tw, uint32_t nb, uint32_t s, uint32_t magic,
                                        uint32_t lane, uint32_t tpr, float scale) {
  for (uint32_t i = lane; i < nb; i += tpr) {
    float2 x[R], y[R];
#pragma unroll
    for (int k = 0; k < R; ++k) x[k] = src[i + k * nb];
    tp_butterfly<R>(x, y);
    if constexpr (LAST) {   // s = nb, p = 0: no twiddles, natural order
#pragma unroll
      for (int j = 0; j < R; ++j) dst[i + j * nb] = scale * y[j];
    } else {
      const uint32_t p = magic ? __umulhi(i, magic) : i;   // floor(i / s)
      const uint32_t ps = p * s;
      const uint32_t o = (i - ps) + ps * R;
      dst[o] = y[0];
#pragma unroll
      for (int j = 1; j < R; ++j) dst[o + s * j] = tp_cmul(y[j], tw[ps * j]);
    }
  }
}

template <bool LAST>
__device__ __forceinline__ void tp_pass_any(uint32_t r, const float2* src, float2* dst, const float2* __restrict__ tw, uint32_t nb, uint32_t s,
                                            uint32_t magic, uint32_t lane, uint32_t tpr, float scale) {
  switch (r) {   // uniform
    case 4: tp_pass<4, LAST>(src, dst, tw, nb, s, magic, lane, tpr, scale); break;
    case 2: tp_pass<2, LAST>(src, dst, tw, nb, s, magic, lane, tpr, scale); break;
    case 3: tp_pass<3, LAST>(src, dst, tw, nb, s, magic, lane, tpr, scale); break;
    default: tp_pass<5, LAST>(src, dst, tw, nb, s, magic, lane, tpr, scale); break;
  }
}

// Every pass of the workgroup's rows, the row in `buf0` (written before the workgroup's last barrier) with `buf1` as the
// other half of the ping-pong pair; returns the buffer that holds the result, in natural order, after a barrier.
// Every thread of the workgroup calls it.
__device__ __forceinline__ float2* tp_passes(const FftDev& P, float2* buf0, float2* buf1, const float2* __restrict__ tw, uint32_t lane, uint32_t tpr,
                                             float scale) {
  float2* src = buf0;
  float2* dst = buf1;
  uint32_t s = 1u;
  for (uint32_t pass = 0; pass + 1u < P.n_passes; ++pass) {
    const uint32_t r = P.radix[pass];
    tp_pass_any<false>(r, src, dst, tw, P.m / r, s, P.magic[pass], lane, tpr, 1.0f);
    s *= r;
    __syncthreads();
    float2* t = src;
    src = dst;
    dst = t;
  }
  const uint32_t r = P.radix[P.n_passes - 1u];
  tp_pass_any<true>(r, src, dst, tw, s, s, 0u, lane, tpr, scale);   // M / r = s: the last radix closes the product
  __syncthreads();
  return dst;
}

// ---- host ----

// Radix sequence, stride constants and launch geometry of a transform of length `len` over `n_rows` rows per slot (or per
// (slot, port)) into `v`; false, with `v` untouched, unless len = 2^a 3^b 5^c with at most CE_TP_MAX_PASSES radices.
inline bool fft_derive(int len, int n_rows, ce_tp_host_view* v) {
  int rest = len, e[3] = {0, 0, 0};   // exponents of 2, 3, 5
  const int primes[3] = {2, 3, 5};
  if (len < 1) return false;
  for (int i = 0; i < 3; ++i)
    while (rest % primes[i] == 0) {
      rest /= primes[i];
      ++e[i];
    }
  if (rest != 1 || e[0] / 2 + (e[0] & 1) + e[1] + e[2] > CE_TP_MAX_PASSES) return false;
  int n = 0;
  for (int i = 0; i < e[0] / 2; ++i) v->radix[n++] = 4;
  if (e[0] & 1) v->radix[n++] = 2;
  for (int i = 0; i < e[1]; ++i) v->radix[n++] = 3;
  for (int i = 0; i < e[2]; ++i) v->radix[n++] = 5;   // at most 7 entries for len <= 4096
  v->n_passes = n;
  uint32_t s = 1;
  for (int i = 0; i < n; ++i) {
    v->stride_magic[i] = s == 1 ? 0u : (uint32_t)(0x100000000ull / s) + 1u;   // exact for i s < 2^32 (i < len <= 4096, s <= len)
    s *= (uint32_t)v->radix[i];
  }
  v->m_sc = len;
  // a row's threads: about one radix-4 butterfly each in the small rows, where lanes would idle otherwise
  v->threads_per_row = len <= 384 ? 64 : len <= 1152 ? 128 : 256;
  v->threads = TP_NT;
  v->rows_per_workgroup = TP_NT / v->threads_per_row;
  v->lds_bytes = v->rows_per_workgroup * 2 * 8 * len;
  v->twiddle_bytes = 8 * len;
  v->n_workgroups_per_slot = (n_rows + v->rows_per_workgroup - 1) / v->rows_per_workgroup;
  return true;
}

// W[n] = exp(+j 2 pi n / len), n < len, in double, rounded once: len (re, im) pairs
inline void fft_twiddles(int len, float* out) {
  const double two_pi = 6.283185307179586476925286766559;
  for (int n = 0; n < len; ++n) {
    const double a = two_pi * (double)n / (double)len;
    out[2 * n] = (float)cos(a);
    out[2 * n + 1] = (float)sin(a);
  }
}

// The kernels' plan values of a derived view with `n_rows` rows per item.
inline FftDev fft_dev(const ce_tp_host_view& v, int n_rows) {
  FftDev D{};
  D.m = (uint32_t)v.m_sc;
  D.n_rows = (uint32_t)n_rows;
  D.tpr_log2 = v.threads_per_row == 64 ? 6u : v.threads_per_row == 128 ? 7u : 8u;
  D.rpw = (uint32_t)v.rows_per_workgroup;
  D.wg_per_item = (uint32_t)v.n_workgroups_per_slot;
  D.n_passes = (uint32_t)v.n_passes;
  for (int i = 0; i < CE_TP_MAX_PASSES; ++i) {
    D.radix[i] = (uint32_t)v.radix[i];
    D.magic[i] = v.stride_magic[i];
  }
  return D;
}

// What a plan holds besides its kernel's argument block.
struct FftPlan {
  int device = 0;
  int lds_bytes = 0;
  float2* tw = nullptr;   // M twiddles on `device`
};

// *_plan_destroy of a plan that keeps its FftPlan in `core`.
template <class Plan>
void fft_plan_destroy(Plan* p) {
  if (!p) return;
  if (p->core.tw) (void)hipFree(p->core.tw);
  delete p;
}

// Fills `c` for the view's transform on `device`: the twiddle table, generated and uploaded.  Whatever the result, c->tw
// stays the plan's to free.
inline hipError_t fft_plan_upload(FftPlan* c, int device, const ce_tp_host_view& v) {
  c->device = device;
  c->lds_bytes = v.lds_bytes;
  std::vector<float> tw(2 * (size_t)v.m_sc);
  fft_twiddles(v.m_sc, tw.data());
  CeDeviceScope scope(device);
  return ce_upload(scope.err, &c->tw, tw.data(), tw.size() * sizeof(float));
}

}  // namespace

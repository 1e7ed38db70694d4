// EXTENSION (no reference counterpart, see include/ce_tp.h): PRACH preamble detection over frequency-domain rows -- per
// (occasion, root) the product of every row with the root's table, the inverse transform of length N = 2^n scaled by 1 / L,
// the power delay profile summed over the terms, and per cyclic-shift window its maximum and the first index that attains it.
//
// Operator (include/ce_tp.h has the derivation of the windows and the table):
//     Z[k] = Y[b][r][s][k] T_i[k]  (combine = 0: a term is (r, s))   or   (sum_s Y[b][r][s][k]) T_i[k]  (combine = 1: a term is r)
//     z[n] = (1 / L) sum_{k<L} Z[k] exp(+j 2 pi k n / N), n < N          P[b][i][n] = sum over the terms of |z[n]|^2
//     mean[b][i] = (1 / N) sum_n P[b][i][n]
//     peak[b][i][v] = max_{d < win_len} P[b][i][(win_start[v] + d) mod N],  delay[b][i][v] = the smallest d that attains it
//
// Kernel: one 256-thread workgroup per (occasion, root), the row frame of ce_fft.h with a row being a TERM: rows_per_workgroup
// (4, 2 or 1 by N) terms at a time, row q taking the terms q, q + rows_per_workgroup, ..
//   load   thread t of the row takes k = t, t + threads_per_row, .. < N: for k < L one 8-byte load of Y (combine = 1: n_reps of
//          them, added in ascending order) and one of T_i, contiguous over the lanes, and the complex product; zero for
//          k >= L and for a row without a term.  8-byte LDS writes in natural order: lanes on consecutive dword pairs.
//   passes the Stockham passes of ce_fft.h over the host's radix sequence, one barrier per pass; the last pass applies
//          float32(1 / L).  The passes are the inverse transform natively: no conjugation.
//   power  thread t adds re^2 + im^2 of the outputs n = t + j threads_per_row, j < N / threads_per_row <= 16, to the
//          registers it keeps for them (8-byte LDS reads, consecutive over the lanes).  One barrier, then the next terms.
//   fold   every row writes its sums to LDS (float32 [row][N], over the transform buffers, behind a barrier); thread t adds the
//          rows in ascending order for n = t, t + 256, .. and leaves P in row 0's place.
//   mean   per thread the sum of its P[n] in ascending n, a butterfly of __shfl_xor per wave, the four waves through LDS.
//   peak   wave w takes the windows v = w, w + 4, ..: lane l scans d = l, l + 64, .. < win_len (consecutive dwords over the
//          lanes: no bank conflicts) keeping the first largest value, then the butterfly on (value, d) pairs, the smaller d
//          winning a tie.  Lane 0 stores.
// 64-bit addressing; no atomics, no scratch; tensor values enter arithmetic only.  DESIGN 6t.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "ce_fft.h"
#include "ce_stage.h"
#include "ce_tp.h"

namespace {

constexpr int PRACH_MAX_ROOTS = 64, PRACH_MAX_SHIFTS = 64, PRACH_MAX_PORTS = 64, PRACH_MAX_REPS = 12;
constexpr int PRACH_MAX_PER_THREAD = 16;   // N / threads_per_row: 4 (N = 256, 512), 8 (1024, 2048), 16 (4096)

struct PrachDev {
  FftDev f;               // m = N, n_rows = 1, wg_per_item = 1; an item is an (occasion, root)
  uint32_t l_ra;          // L
  uint32_t n_roots;
  uint32_t n_shifts;
  uint32_t win_len;
  uint32_t combine;
  float scale;            // float32(1 / L)
  float inv_n;            // 1 / N
  int32_t win_start[PRACH_MAX_SHIFTS];   // entries >= n_shifts are 0
};

// (value, index): the larger value, of equal values the smaller index.  A value of -1 stands for "nothing yet" (P >= 0).
__device__ __forceinline__ void prach_take(float& best, uint32_t& best_d, float v, uint32_t d) {
  if (v > best || (v == best && d < best_d)) {
    best = v;
    best_d = d;
  }
}

__global__ __launch_bounds__(TP_NT) void ce_prach_kernel(PrachDev P, const float2* __restrict__ tw, const float2* __restrict__ table,
                                                         const float2* __restrict__ y, int64_t occ_stride, int64_t port_stride, int64_t rep_stride,
                                                         uint32_t n_ports, uint32_t n_reps, float* __restrict__ peak, int32_t* __restrict__ delay,
                                                         float* __restrict__ mean, float* __restrict__ profile) {
  extern __shared__ float4 prach_lds[];
  const uint32_t N = P.f.m, L = P.l_ra, mask = N - 1u;
  const uint32_t tpr = 1u << P.f.tpr_log2, rpw = P.f.rpw;
  const uint32_t rl = threadIdx.x >> P.f.tpr_log2, lane = threadIdx.x & (tpr - 1u);   // rl: row of the workgroup (wave-uniform)
  const uint32_t occ = blockIdx.x / P.n_roots, root = blockIdx.x - occ * P.n_roots;
  float2* buf0 = reinterpret_cast<float2*>(prach_lds) + (size_t)rl * 2u * N;
  float2* buf1 = buf0 + N;
  const float2* t_row = table + (size_t)root * L;
  const float2* y_occ = y + (int64_t)occ * occ_stride;
  const uint32_t n_terms = P.combine ? n_ports : n_ports * n_reps;
  const uint32_t per_thread = N >> P.f.tpr_log2;

  float acc[PRACH_MAX_PER_THREAD];
#pragma unroll
  for (int j = 0; j < PRACH_MAX_PER_THREAD; ++j) acc[j] = 0.0f;

  for (uint32_t t0 = 0; t0 < n_terms; t0 += rpw) {   // uniform over the workgroup
    const uint32_t term = t0 + rl;
    const bool active = term < n_terms;
    // ---- load: Y T_i onto the bins 0 .. L - 1, zeros behind (a row without a term: zeros) ----
    {
      uint32_t r = term, s = 0u;
      if (!P.combine) {
        r = term / n_reps;
        s = term - r * n_reps;
      }
      const float2* row = y_occ + ((int64_t)r * port_stride + (int64_t)s * rep_stride);
      for (uint32_t k = lane; k < N; k += tpr) {
        float2 z = make_float2(0.0f, 0.0f);
        if (active && k < L) {
          float2 v = row[k];
          if (P.combine)
            for (uint32_t q = 1; q < n_reps; ++q) v = v + row[(int64_t)q * rep_stride + k];
          z = tp_cmul(v, t_row[k]);
        }
        buf0[k] = z;
      }
    }
    __syncthreads();

    const float2* res = tp_passes(P.f, buf0, buf1, tw, lane, tpr, P.scale);

    // ---- power: this term's |z[n]|^2 onto the row's sums ----
    if (active) {
#pragma unroll
      for (int j = 0; j < PRACH_MAX_PER_THREAD; ++j)
        if ((uint32_t)j < per_thread) {
          const float2 v = res[lane + (uint32_t)j * tpr];
          acc[j] += v.x * v.x + v.y * v.y;
        }
    }
    __syncthreads();   // the next load writes buf0, which may be `res`
  }

  // ---- fold: the rows' sums, in ascending row order, into P (row 0's place) ----
  float* rows = reinterpret_cast<float*>(prach_lds);   // [rpw][N]; the loop's last barrier is behind every read of the buffers
  float* wave_sum = rows + rpw * N;                    // [4], behind them: the buffers hold 4 rpw N floats, all of the 64 KiB at N = 4096
#pragma unroll
  for (int j = 0; j < PRACH_MAX_PER_THREAD; ++j)
    if ((uint32_t)j < per_thread) rows[rl * N + lane + (uint32_t)j * tpr] = acc[j];
  __syncthreads();
  float part = 0.0f;
  float* prof = profile ? profile + (int64_t)blockIdx.x * N : nullptr;
  for (uint32_t n = threadIdx.x; n < N; n += TP_NT) {   // thread t alone touches the index n = t + 256 j of any row here
    float p = rows[n];
    for (uint32_t q = 1; q < rpw; ++q) p += rows[q * N + n];
    rows[n] = p;
    part += p;
    if (prof) prof[n] = p;
  }
  // ---- mean ----
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
  if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = part;
  __syncthreads();   // also: P is complete
  if (threadIdx.x == 0u) mean[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3])) * P.inv_n;

  // ---- peak: one wave per window ----
  const uint32_t wave = threadIdx.x >> 6, wl = threadIdx.x & 63u;
  for (uint32_t v = wave; v < P.n_shifts; v += TP_NT / 64) {
    const uint32_t start = (uint32_t)P.win_start[v];
    float best = -1.0f;
    uint32_t best_d = 0x7FFFFFFFu;
    for (uint32_t d = wl; d < P.win_len; d += 64u) {
      const float p = rows[(start + d) & mask];
      if (p > best) {   // ascending d: the first of equal values stays
        best = p;
        best_d = d;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(best, off);
      const uint32_t od = (uint32_t)__shfl_xor((int)best_d, off);
      prach_take(best, best_d, ov, od);
    }
    if (wl == 0u) {
      const bool none = best < 0.0f;   // every value of the window unordered (NaN)
      const int64_t o = (int64_t)blockIdx.x * P.n_shifts + v;
      peak[o] = none ? __builtin_nanf("") : best;
      delay[o] = none ? 0 : (int32_t)best_d;
    }
  }
}

// ---- host derivation ----

// Validation of the plan values; the view, the window starts into `win_start` (n_shifts entries) and *win_len.
int prach_derive(int32_t l_ra, int32_t n_fft, int32_t n_roots, const int32_t* roots, int32_t n_cs, int32_t n_shifts, int32_t combine,
                 ce_tp_host_view* v, int32_t* win_start, int32_t* win_len) {
  memset(v, 0, sizeof(*v));
  if (l_ra != 139 && l_ra != 571 && l_ra != 839 && l_ra != 1151) return ce_fail(CE_ERR_INVALID, "l_ra=%d is not 139, 571, 839 or 1151", l_ra);
  if (n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048 && n_fft != 4096)
    return ce_fail(CE_ERR_INVALID, "n_fft=%d is not 256, 512, 1024, 2048 or 4096", n_fft);
  if (n_fft <= l_ra) return ce_fail(CE_ERR_INVALID, "n_fft=%d must exceed l_ra=%d", n_fft, l_ra);
  if (n_roots < 1 || n_roots > PRACH_MAX_ROOTS) return ce_fail(CE_ERR_INVALID, "n_roots=%d outside 1..%d", n_roots, PRACH_MAX_ROOTS);
  if (!roots) return ce_fail(CE_ERR_INVALID, "null argument");
  for (int i = 0; i < n_roots; ++i) {
    if (roots[i] < 1 || roots[i] >= l_ra) return ce_fail(CE_ERR_INVALID, "roots[%d]=%d outside 1..%d", i, roots[i], l_ra - 1);
    for (int j = 0; j < i; ++j)
      if (roots[j] == roots[i]) return ce_fail(CE_ERR_INVALID, "roots[%d]=%d repeats roots[%d]", i, roots[i], j);
  }
  if (n_cs < 0 || n_cs >= l_ra) return ce_fail(CE_ERR_INVALID, "n_cs=%d outside 0..%d", n_cs, l_ra - 1);
  if (n_shifts < 1 || n_shifts > PRACH_MAX_SHIFTS) return ce_fail(CE_ERR_INVALID, "n_shifts=%d outside 1..%d", n_shifts, PRACH_MAX_SHIFTS);
  if (n_cs == 0 && n_shifts != 1) return ce_fail(CE_ERR_INVALID, "n_cs=0 (one window round the circle) with n_shifts=%d", n_shifts);
  if ((int64_t)n_shifts * n_cs > l_ra) return ce_fail(CE_ERR_INVALID, "n_shifts=%d x n_cs=%d exceeds l_ra=%d", n_shifts, n_cs, l_ra);
  if (combine != 0 && combine != 1) return ce_fail(CE_ERR_INVALID, "combine=%d is neither 0 (non-coherent) nor 1 (coherent)", combine);
  if (!fft_derive(n_fft, 1, v)) return ce_fail(CE_ERR_INVALID, "n_fft=%d has no radix sequence", n_fft);   // (not reached: powers of two)
  if (n_cs == 0) {
    win_start[0] = 0;
    *win_len = n_fft;
  } else {
    const int32_t g = (n_fft + l_ra - 1) / l_ra;
    for (int s = 0; s < n_shifts; ++s) {
      const int64_t c = (int64_t)((l_ra - s * n_cs) % l_ra);   // (L - C_v) mod L; C_v <= L
      win_start[s] = (int32_t)(((c * n_fft) / l_ra - g + n_fft) % n_fft);
    }
    *win_len = (int32_t)(((int64_t)n_cs * n_fft) / l_ra);
  }
  return CE_OK;
}

// T_i[k] = conj(X_u[k]) / |X_u[k]| of root u into `out`, L (re, im) pairs.  For an odd prime L completing the square gives
// X_u[k] = X_u[0] conj(x_u(m)), m = u^-1 k mod L, so T_i[k] = (conj(X_u[0]) / |X_u[0]|) x_u(m): one sum of L terms per root.
void prach_root_table(int32_t l_ra, int32_t u, float* out) {
  const double two_pi = 6.283185307179586476925286766559;
  const int64_t L = l_ra;
  auto x_u = [&](int64_t n, double* re, double* im) {   // exp(-j 2 pi ((u n (n + 1) / 2) mod L) / L)
    const int64_t q = (((n * (n + 1)) / 2) % L * u) % L;
    const double a = -two_pi * (double)q / (double)L;
    *re = cos(a);
    *im = sin(a);
  };
  double sr = 0.0, si = 0.0;   // X_u[0]
  for (int64_t n = 0; n < L; ++n) {
    double re, im;
    x_u(n, &re, &im);
    sr += re;
    si += im;
  }
  const double mag = sqrt(sr * sr + si * si), cr = sr / mag, ci = -si / mag;   // conj(X_u[0]) / |X_u[0]|
  int64_t u_inv = 1;
  while ((u_inv * u) % L != 1) ++u_inv;
  for (int64_t k = 0; k < L; ++k) {
    double re, im;
    x_u((u_inv * k) % L, &re, &im);
    out[2 * k] = (float)(cr * re - ci * im);
    out[2 * k + 1] = (float)(cr * im + ci * re);
  }
}

}  // namespace

struct ce_prach_plan {
  FftPlan core;
  PrachDev dev{};
  float2* table = nullptr;   // n_roots x L on core.device
};

extern "C" int ce_prach_derive_host(int32_t l_ra, int32_t n_fft, int32_t n_roots, const int32_t* roots, int32_t n_cs, int32_t n_shifts,
                                    int32_t combine, ce_tp_host_view* view, int32_t* win_start, int32_t* win_len) {
  if (!view || !win_start || !win_len) return ce_fail(CE_ERR_INVALID, "null argument");
  int32_t ws[PRACH_MAX_SHIFTS], wl;
  ce_tp_host_view v;
  if (const int rc = prach_derive(l_ra, n_fft, n_roots, roots, n_cs, n_shifts, combine, &v, ws, &wl); rc != CE_OK) return rc;
  *view = v;
  memcpy(win_start, ws, sizeof(int32_t) * (size_t)n_shifts);
  *win_len = wl;
  return CE_OK;
}

extern "C" int ce_prach_copy_tables(int32_t l_ra, int32_t n_fft, int32_t n_roots, const int32_t* roots, float* twiddles, float* table) {
  int32_t ws[PRACH_MAX_SHIFTS], wl;
  ce_tp_host_view v;
  if (const int rc = prach_derive(l_ra, n_fft, n_roots, roots, 0, 1, 0, &v, ws, &wl); rc != CE_OK) return rc;
  if (twiddles) fft_twiddles(n_fft, twiddles);
  if (table)
    for (int i = 0; i < n_roots; ++i) prach_root_table(l_ra, roots[i], table + 2 * (size_t)i * (size_t)l_ra);
  return CE_OK;
}

extern "C" void ce_prach_plan_destroy(ce_prach_plan* p) {
  if (p && p->table) (void)hipFree(p->table);
  fft_plan_destroy(p);
}

extern "C" int ce_prach_plan_create(int32_t abi_version, int32_t device, int32_t l_ra, int32_t n_fft, int32_t n_roots, const int32_t* roots,
                                    int32_t n_cs, int32_t n_shifts, int32_t combine, ce_prach_plan** out) {
  if (!out) return ce_fail(CE_ERR_INVALID, "null argument");
  if (abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", abi_version, CE_ABI_VERSION);
  auto p = ce_new_plan<ce_prach_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  ce_tp_host_view v;
  PrachDev& D = p->dev;
  int32_t wl;
  if (const int rc = prach_derive(l_ra, n_fft, n_roots, roots, n_cs, n_shifts, combine, &v, D.win_start, &wl); rc != CE_OK) return rc;
  D.f = fft_dev(v, 1);
  D.l_ra = (uint32_t)l_ra;
  D.n_roots = (uint32_t)n_roots;
  D.n_shifts = (uint32_t)n_shifts;
  D.win_len = (uint32_t)wl;
  D.combine = (uint32_t)combine;
  D.scale = (float)(1.0 / (double)l_ra);
  D.inv_n = 1.0f / (float)n_fft;
  std::vector<float> table(2 * (size_t)n_roots * (size_t)l_ra);
  for (int i = 0; i < n_roots; ++i) prach_root_table(l_ra, roots[i], table.data() + 2 * (size_t)i * (size_t)l_ra);
  hipError_t e = fft_plan_upload(&p->core, device, v);
  {
    CeDeviceScope scope(device);
    if (e == hipSuccess) e = scope.err;
    e = ce_upload(e, &p->table, table.data(), table.size() * sizeof(float));
  }
  if (e != hipSuccess) {
    ce_prach_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "PRACH detector plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" int ce_prach_detect(const ce_prach_plan* p, const void* y, int64_t occasion_stride, int64_t port_stride, int64_t rep_stride,
                               int64_t n_occasions, int32_t n_ports, int32_t n_reps, float* peak, int32_t* delay, float* mean, float* profile,
                               void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_occasions < 0) return ce_fail(CE_ERR_INVALID, "n_occasions=%lld", (long long)n_occasions);
  if (n_ports < 1 || n_ports > PRACH_MAX_PORTS) return ce_fail(CE_ERR_INVALID, "n_ports=%d outside 1..%d", n_ports, PRACH_MAX_PORTS);
  if (n_reps < 1 || n_reps > PRACH_MAX_REPS) return ce_fail(CE_ERR_INVALID, "n_reps=%d outside 1..%d", n_reps, PRACH_MAX_REPS);
  if (n_occasions == 0) return CE_OK;
  if (!y || !peak || !delay || !mean) return ce_fail(CE_ERR_INVALID, "null argument");
  if (occasion_stride < 0 || port_stride < 0 || rep_stride < 0)
    return ce_fail(CE_ERR_INVALID, "occasion_stride=%lld, port_stride=%lld and rep_stride=%lld must be >= 0", (long long)occasion_stride,
                   (long long)port_stride, (long long)rep_stride);
  if (reinterpret_cast<uintptr_t>(y) & 7u) return ce_fail(CE_ERR_INVALID, "y must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(peak) | reinterpret_cast<uintptr_t>(delay) | reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(profile)) & 3u)
    return ce_fail(CE_ERR_INVALID, "peak, delay, mean and profile must be 4-byte aligned");
  const PrachDev& D = p->dev;
  int64_t n_wg;
  if (const int rc = ce_rows_workgroups(n_occasions, (int64_t)D.n_roots, 1, &n_wg); rc != CE_OK) return rc;
  const int64_t room = INT64_MAX >> 6;
  if (occasion_stride > room / n_occasions || port_stride > room / n_ports || rep_stride > room / n_reps)
    return ce_fail(CE_ERR_INVALID, "occasion_stride=%lld, port_stride=%lld, rep_stride=%lld: the extent of y exceeds the address space",
                   (long long)occasion_stride, (long long)port_stride, (long long)rep_stride);
  const uintptr_t y0 = reinterpret_cast<uintptr_t>(y);
  const uintptr_t y1 = y0 + 8u * (uintptr_t)((n_occasions - 1) * occasion_stride + (n_ports - 1) * port_stride + (n_reps - 1) * rep_stride + D.l_ra);
  const struct {
    const void* ptr;
    uintptr_t elems;
    const char* name;
  } outs[4] = {{peak, (uintptr_t)n_wg * D.n_shifts, "peak"}, {delay, (uintptr_t)n_wg * D.n_shifts, "delay"}, {mean, (uintptr_t)n_wg, "mean"},
               {profile, (uintptr_t)n_wg * D.f.m, "profile"}};
  for (const auto& o : outs) {
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(o.ptr), o1 = o0 + 4u * o.elems;
    if (o.ptr && y0 < o1 && o0 < y1) return ce_fail(CE_ERR_INVALID, "%s overlaps y", o.name);
  }
  CeDeviceScope scope(p->core.device);
  if (scope.err != hipSuccess) return ce_device_fail(p->core.device, scope.err);
  hipLaunchKernelGGL(ce_prach_kernel, dim3((unsigned)n_wg), dim3(TP_NT), (size_t)p->core.lds_bytes, (hipStream_t)stream, D, p->core.tw, p->table,
                     reinterpret_cast<const float2*>(y), occasion_stride, port_stride, rep_stride, (uint32_t)n_ports, (uint32_t)n_reps, peak, delay, mean,
                     profile);
  return ce_launch_status("PRACH detection");
}

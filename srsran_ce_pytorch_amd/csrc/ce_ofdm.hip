// EXTENSION (no reference counterpart, see include/ce_tp.h): OFDM demodulation -- per (slot, port, symbol) the window of N
// time-domain samples behind the cyclic prefix, its DFT of length N = 2^n scaled by 1 / sqrt(N), and the n_sc bins around
// DC onto the subcarriers of the resource grid, with the window advance and the per-symbol phase compensated at the store.
// Behind it, on the same plan, the transmit direction: OFDM modulation (ce_ofdmtx_kernel).
//
// Kernel: the row frame of ce_fft.h, a row being a window (symbol) of one (slot, port): 64 KiB of LDS at N = 4096, two
// workgroups per CU.
//   load   thread t of the row takes the samples n = t, t + threads_per_row, .. of the window with 8-byte loads (a window
//          may start at an odd sample), contiguous over the lanes, and writes conj(s_n) into buffer 0 in natural order.
//          An inactive row of a (slot, port)'s last workgroup writes zeros.
//   passes the Stockham passes of ce_fft.h (shared with ce_tp.hip) over the host's radix sequence, one barrier per pass;
//          the last pass applies float32(1 / sqrt(N)) and leaves the bins in natural order.  DFT(s) = conj(IDFT(conj(s))).
//   store  thread t takes the pairs of subcarriers k = 2 h, 2 h + 1, h = t, t + threads_per_row, ..: one 16-byte LDS read
//          at bin (k - n_sc / 2) mod N (n_sc / 2 is even, so a pair never straddles DC and the read is aligned), the
//          conjugation, the product with W[(q_k a) mod N] where a != 0, the product with phi_l where phasors were given,
//          one 16-byte store, contiguous over the lanes.  Bins N - n_sc / 2 .. N - 1 go to k = 0 .. n_sc / 2 - 1, bins
//          0 .. n_sc / 2 - 1 to k = n_sc / 2 .. n_sc - 1; the other N - n_sc bins are dropped.
// 64-bit addressing; no atomics, no scratch; tensor values enter arithmetic only.  DESIGN 6p.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>

#include "ce_fft.h"
#include "ce_stage.h"
#include "ce_tp.h"

namespace {

struct OfdmDev {
  FftDev f;               // m = N, n_rows = n_sym; an item is a (slot, port)
  uint32_t n_sc;
  uint32_t adv;           // a
  uint32_t has_phasor;
  float scale;            // float32(1 / sqrt(N))
  int32_t win[CE_MAX_SYMBOLS];      // w_l, samples from the start of the slot; entries >= n_sym are 0
  float2 phasor[CE_MAX_SYMBOLS];    // phi_l
};

__global__ __launch_bounds__(TP_NT) void ce_ofdm_kernel(OfdmDev P, const float2* __restrict__ tw, const float2* __restrict__ samples, int64_t slot_stride,
                                                        int64_t port_stride, uint32_t n_ports, float4* __restrict__ out) {
  extern __shared__ float4 ofdm_lds[];
  const auto [item, row, lane, tpr, active, buf0, buf1] = fft_row(P.f, ofdm_lds);   // item = slot n_ports + port
  const uint32_t N = P.f.m;
  const uint32_t slot = item / n_ports, port = item - slot * n_ports;
  const uint32_t ri = active ? row : 0u;

  // ---- load: conj(s) into buf0 (an inactive row: zeros) ----
  {
    const float2* s = samples + ((int64_t)slot * slot_stride + (int64_t)port * port_stride + (int64_t)P.win[ri]);
    for (uint32_t n = lane; n < N; n += tpr) {
      float2 v = make_float2(0.0f, 0.0f);
      if (active) v = s[n];
      buf0[n] = make_float2(v.x, -v.y);
    }
  }
  __syncthreads();

  const float2* res = tp_passes(P.f, buf0, buf1, tw, lane, tpr, P.scale);

  // ---- store: conj, advance, phasor ----
  if (active) {
    const uint32_t n_half = P.n_sc >> 1, mask = N - 1u;
    const float2 phi = P.phasor[ri];
    float4* o = out + ((((int64_t)item * P.f.n_rows + row) * (int64_t)P.n_sc) >> 1);
    for (uint32_t h = lane; h < n_half; h += tpr) {
      const uint32_t q = 2u * h - n_half;   // q_k of k = 2 h in two's complement: N divides 2^32, so `& mask` is mod N
      const float4 v = *reinterpret_cast<const float4*>(res + (q & mask));
      float2 y0 = make_float2(v.x, -v.y), y1 = make_float2(v.z, -v.w);
      if (P.adv) {
        y0 = tp_cmul(y0, tw[(q * P.adv) & mask]);
        y1 = tp_cmul(y1, tw[((q + 1u) * P.adv) & mask]);
      }
      if (P.has_phasor) {
        y0 = tp_cmul(y0, phi);
        y1 = tp_cmul(y1, phi);
      }
      o[h] = make_float4(y0.x, y0.y, y1.x, y1.y);
    }
  }
}

// OFDM MODULATION, the transmit direction on the same plan: per (slot, port, symbol) the n_sc subcarriers of the grid onto
// the bins around DC, the transform of length N -- the passes are the inverse transform natively, so there is no
// conjugation -- scaled by 1 / sqrt(N), and the cp_l + N samples of the symbol with its cyclic prefix in front.
//   load   thread t of the row takes the pairs of subcarriers k = 2 h, 2 h + 1, h = t, t + threads_per_row, ..: one 16-byte
//          global load, contiguous over the lanes, the product with conj(phi_l) where phasors were given, one 16-byte LDS
//          write at bin (k - n_sc / 2) mod N; the N - n_sc bins n_sc / 2 .. N - n_sc / 2 - 1 in between are written with
//          zeros, 16 bytes at a time (n_sc / 2 and N - n_sc are even).  An inactive row writes zeros and loads nothing.
//   passes as above, without the conjugations.
//   store  thread t takes the samples j = t, t + threads_per_row, .. < cp_l + N of the symbol: sample j is the result's
//          element (j - cp_l) mod N, so the prefix is the symbol's tail stored a second time; 8-byte stores (a symbol may
//          start at an odd sample), contiguous over the lanes.  Every sample of [0, T) of a (slot, port) exactly once.
struct OfdmTxDev {
  FftDev f;               // the demodulator's
  uint32_t n_sc;
  uint32_t has_phasor;
  float scale;            // float32(1 / sqrt(N))
  int32_t start[CE_MAX_SYMBOLS];    // t_l, samples from the start of the slot; entries >= n_sym are 0
  int32_t cp[CE_MAX_SYMBOLS];       // cp_l
  float2 phasor[CE_MAX_SYMBOLS];    // phi_l, the demodulator's: applied conjugated
};

__global__ __launch_bounds__(TP_NT) void ce_ofdmtx_kernel(OfdmTxDev P, const float2* __restrict__ tw, const float4* __restrict__ grid, uint32_t n_ports,
                                                          float2* __restrict__ samples, int64_t slot_stride, int64_t port_stride) {
  extern __shared__ float4 ofdm_lds[];
  const auto [item, row, lane, tpr, active, buf0, buf1] = fft_row(P.f, ofdm_lds);   // item = slot n_ports + port
  const uint32_t N = P.f.m, mask = N - 1u, n_half = P.n_sc >> 1;
  const uint32_t slot = item / n_ports, port = item - slot * n_ports;
  const uint32_t ri = active ? row : 0u;

  // ---- load: conj(phi) X onto the bins around DC, zeros in between (an inactive row: zeros) ----
  {
    const float2 phi = make_float2(P.phasor[ri].x, -P.phasor[ri].y);
    const float4* x = grid + ((((int64_t)item * P.f.n_rows + ri) * (int64_t)P.n_sc) >> 1);
    for (uint32_t h = lane; h < n_half; h += tpr) {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (active) v = x[h];
      float2 y0 = make_float2(v.x, v.y), y1 = make_float2(v.z, v.w);
      if (P.has_phasor) {
        y0 = tp_cmul(y0, phi);
        y1 = tp_cmul(y1, phi);
      }
      const uint32_t q = 2u * h - n_half;   // q_k of k = 2 h in two's complement: N divides 2^32, so `& mask` is mod N
      *reinterpret_cast<float4*>(buf0 + (q & mask)) = make_float4(y0.x, y0.y, y1.x, y1.y);
    }
    const uint32_t n_guard = (N - P.n_sc) >> 1;   // pairs of unused bins
    for (uint32_t g = lane; g < n_guard; g += tpr) *reinterpret_cast<float4*>(buf0 + (n_half + 2u * g)) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  __syncthreads();

  const float2* res = tp_passes(P.f, buf0, buf1, tw, lane, tpr, P.scale);

  // ---- store: the cyclic prefix and the symbol ----
  if (active) {
    const uint32_t cp = (uint32_t)P.cp[ri], len = cp + N;
    float2* s = samples + ((int64_t)slot * slot_stride + (int64_t)port * port_stride + (int64_t)P.start[ri]);
    for (uint32_t j = lane; j < len; j += tpr) s[j] = res[(j - cp) & mask];
  }
}

// ---- host derivation ----

// Validation of the plan values (all but the phasors); the view, the window starts w_l into `win` (CE_MAX_SYMBOLS
// entries) and the slot length T into *n_samples.
int ofdm_derive(int32_t n_fft, int32_t n_prb_grid, int32_t n_sym, const int32_t* cp_len, int32_t adv, ce_tp_host_view* v, int32_t* win,
                int32_t* n_samples) {
  memset(v, 0, sizeof(*v));
  if (n_fft != 128 && n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048 && n_fft != 4096)
    return ce_fail(CE_ERR_INVALID, "n_fft=%d is not 128, 256, 512, 1024, 2048 or 4096", n_fft);
  if (n_prb_grid < 1 || (int64_t)12 * n_prb_grid > n_fft)
    return ce_fail(CE_ERR_INVALID, "n_prb_grid=%d: n_sc = 12 n_prb_grid must lie in 12..n_fft=%d", n_prb_grid, n_fft);
  if (n_sym < 1 || n_sym > CE_MAX_SYMBOLS) return ce_fail(CE_ERR_INVALID, "n_sym=%d outside 1..%d", n_sym, CE_MAX_SYMBOLS);
  if (!cp_len) return ce_fail(CE_ERR_INVALID, "null argument");
  int32_t cp_min = INT32_MAX;
  for (int l = 0; l < n_sym; ++l) {
    if (cp_len[l] < 0) return ce_fail(CE_ERR_INVALID, "cp_len[%d]=%d is negative", l, cp_len[l]);
    if (cp_len[l] > n_fft) return ce_fail(CE_ERR_INVALID, "cp_len[%d]=%d is longer than the symbol, n_fft=%d", l, cp_len[l], n_fft);
    if (cp_len[l] < cp_min) cp_min = cp_len[l];
  }
  if (adv < 0 || adv > cp_min) return ce_fail(CE_ERR_INVALID, "window_advance=%d outside 0..%d (the shortest cyclic prefix)", adv, cp_min);
  int32_t t = 0;   // <= 14 * 2 * 4096
  for (int l = 0; l < CE_MAX_SYMBOLS; ++l) {
    win[l] = l < n_sym ? t + cp_len[l] - adv : 0;
    if (l < n_sym) t += cp_len[l] + n_fft;
  }
  *n_samples = t;
  if (!fft_derive(n_fft, n_sym, v)) return ce_fail(CE_ERR_INVALID, "n_fft=%d has no radix sequence", n_fft);   // (not reached: powers of two)
  return CE_OK;
}

// What both launches check about a non-empty batch behind their pointers: the workgroup count, into *n_wg, and that the
// extent of the strided tensor, in bytes, stays inside 64 bits.
int ofdm_batch(const FftDev& f, int64_t n_slots, int64_t n_ports, int64_t slot_stride, int64_t port_stride, int64_t* n_wg) {
  if (const int rc = ce_rows_workgroups(n_slots, n_ports, (int64_t)f.wg_per_item, n_wg); rc != CE_OK) return rc;
  return ce_rows_extent(n_slots, n_ports, slot_stride, port_stride);   // n_slots, n_ports < 2^31 here
}

}  // namespace

struct ce_ofdm_plan {
  FftPlan core;
  OfdmDev dev{};
  OfdmTxDev tx{};          // the modulator's argument block of the same values
  int32_t n_samples = 0;   // T
};

extern "C" int ce_ofdm_derive_host(int32_t n_fft, int32_t n_prb_grid, int32_t n_sym, const int32_t* cp_len, int32_t window_advance,
                                   ce_tp_host_view* view) {
  if (!view) return ce_fail(CE_ERR_INVALID, "null argument");
  int32_t win[CE_MAX_SYMBOLS], t;
  return ofdm_derive(n_fft, n_prb_grid, n_sym, cp_len, window_advance, view, win, &t);
}

extern "C" int ce_ofdm_copy_twiddles(int32_t n_fft, float* twiddles) {
  if (!twiddles) return ce_fail(CE_ERR_INVALID, "null argument");
  const int32_t cp = 0;
  ce_tp_host_view v;
  int32_t win[CE_MAX_SYMBOLS], t;
  if (const int rc = ofdm_derive(n_fft, 1, 1, &cp, 0, &v, win, &t); rc != CE_OK) return rc;
  fft_twiddles(n_fft, twiddles);
  return CE_OK;
}

extern "C" int ce_ofdm_plan_create(int32_t abi_version, int32_t device, int32_t n_fft, int32_t n_prb_grid, int32_t n_sym, const int32_t* cp_len,
                                   int32_t window_advance, const float* sym_phasor, ce_ofdm_plan** out) {
  if (!out) return ce_fail(CE_ERR_INVALID, "null argument");
  if (abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", abi_version, CE_ABI_VERSION);
  auto p = ce_new_plan<ce_ofdm_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  ce_tp_host_view v;
  OfdmDev& D = p->dev;
  if (const int rc = ofdm_derive(n_fft, n_prb_grid, n_sym, cp_len, window_advance, &v, D.win, &p->n_samples); rc != CE_OK) return rc;
  if (sym_phasor)
    for (int l = 0; l < n_sym; ++l) {
      if (!isfinite(sym_phasor[2 * l]) || !isfinite(sym_phasor[2 * l + 1])) return ce_fail(CE_ERR_INVALID, "sym_phasor[%d] is not finite", l);
      D.phasor[l] = make_float2(sym_phasor[2 * l], sym_phasor[2 * l + 1]);
    }
  D.f = fft_dev(v, n_sym);
  D.n_sc = 12u * (uint32_t)n_prb_grid;
  D.adv = (uint32_t)window_advance;
  D.has_phasor = sym_phasor ? 1u : 0u;
  D.scale = (float)(1.0 / sqrt((double)n_fft));
  OfdmTxDev& X = p->tx;
  X.f = D.f;
  X.n_sc = D.n_sc;
  X.has_phasor = D.has_phasor;
  X.scale = D.scale;
  for (int l = 0, t = 0; l < n_sym; t += cp_len[l] + n_fft, ++l) {
    X.start[l] = t;
    X.cp[l] = cp_len[l];
    X.phasor[l] = D.phasor[l];
  }
  const hipError_t e = fft_plan_upload(&p->core, device, v);
  if (e != hipSuccess) {
    ce_ofdm_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "OFDM demodulator plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_ofdm_plan_destroy(ce_ofdm_plan* p) { fft_plan_destroy(p); }

extern "C" int ce_ofdm_demodulate(const ce_ofdm_plan* p, const void* samples, int64_t slot_stride, int64_t port_stride, int64_t n_slots,
                                  int64_t n_ports, void* out, void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0 || n_ports < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld, n_ports=%lld", (long long)n_slots, (long long)n_ports);
  if (n_slots == 0 || n_ports == 0) return CE_OK;
  if (!samples || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  if (slot_stride < 0 || port_stride < 0)
    return ce_fail(CE_ERR_INVALID, "slot_stride=%lld and port_stride=%lld must be >= 0", (long long)slot_stride, (long long)port_stride);
  if (reinterpret_cast<uintptr_t>(samples) & 7u) return ce_fail(CE_ERR_INVALID, "samples must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(out) & 15u) return ce_fail(CE_ERR_INVALID, "out must be 16-byte aligned");
  const OfdmDev& D = p->dev;
  int64_t n_wg;
  if (const int rc = ofdm_batch(D.f, n_slots, n_ports, slot_stride, port_stride, &n_wg); rc != CE_OK) return rc;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(samples), o0 = reinterpret_cast<uintptr_t>(out);
  const uintptr_t s1 = s0 + 8u * (uintptr_t)((n_slots - 1) * slot_stride + (n_ports - 1) * port_stride + p->n_samples);
  const uintptr_t o1 = o0 + 8u * (uintptr_t)(n_slots * n_ports) * D.f.n_rows * D.n_sc;
  if (s0 < o1 && o0 < s1) return ce_fail(CE_ERR_INVALID, "out overlaps samples");
  CeDeviceScope scope(p->core.device);
  if (scope.err != hipSuccess) return ce_device_fail(p->core.device, scope.err);
  hipLaunchKernelGGL(ce_ofdm_kernel, dim3((unsigned)n_wg), dim3(TP_NT), (size_t)p->core.lds_bytes, (hipStream_t)stream, D, p->core.tw,
                     reinterpret_cast<const float2*>(samples), slot_stride, port_stride, (uint32_t)n_ports, reinterpret_cast<float4*>(out));
  return ce_launch_status("OFDM demodulation");
}

extern "C" int ce_ofdmtx_modulate(const ce_ofdm_plan* p, const void* grid, int64_t n_slots, int64_t n_ports, void* samples, int64_t slot_stride,
                                  int64_t port_stride, void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0 || n_ports < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld, n_ports=%lld", (long long)n_slots, (long long)n_ports);
  if (n_slots == 0 || n_ports == 0) return CE_OK;
  if (!grid || !samples) return ce_fail(CE_ERR_INVALID, "null argument");
  if (slot_stride < 0 || port_stride < 0)
    return ce_fail(CE_ERR_INVALID, "slot_stride=%lld and port_stride=%lld must be >= 0", (long long)slot_stride, (long long)port_stride);
  if (reinterpret_cast<uintptr_t>(grid) & 15u) return ce_fail(CE_ERR_INVALID, "grid must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(samples) & 7u) return ce_fail(CE_ERR_INVALID, "samples must be 8-byte aligned");
  const OfdmTxDev& D = p->tx;
  int64_t n_wg;
  if (const int rc = ofdm_batch(D.f, n_slots, n_ports, slot_stride, port_stride, &n_wg); rc != CE_OK) return rc;
  // every sample is written by one workgroup only: the rows of T samples pairwise disjoint, the ports inside a slot or the
  // slots inside a port (one continuous stream per port)
  const int64_t T = p->n_samples;
  if (const int rc = ce_rows_disjoint(n_slots, n_ports, slot_stride, port_stride, T); rc != CE_OK) return rc;
  const uintptr_t g0 = reinterpret_cast<uintptr_t>(grid), s0 = reinterpret_cast<uintptr_t>(samples);
  const uintptr_t g1 = g0 + 8u * (uintptr_t)(n_slots * n_ports) * D.f.n_rows * D.n_sc;
  const uintptr_t s1 = s0 + 8u * (uintptr_t)((n_slots - 1) * slot_stride + (n_ports - 1) * port_stride + T);
  if (g0 < s1 && s0 < g1) return ce_fail(CE_ERR_INVALID, "samples overlaps grid");
  CeDeviceScope scope(p->core.device);
  if (scope.err != hipSuccess) return ce_device_fail(p->core.device, scope.err);
  hipLaunchKernelGGL(ce_ofdmtx_kernel, dim3((unsigned)n_wg), dim3(TP_NT), (size_t)p->core.lds_bytes, (hipStream_t)stream, D, p->core.tw,
                     reinterpret_cast<const float4*>(grid), (uint32_t)n_ports, reinterpret_cast<float2*>(samples), slot_stride, port_stride);
  return ce_launch_status("OFDM modulation");
}

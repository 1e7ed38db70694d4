// EXTENSION (no reference counterpart, see include/ce_tp.h): transform de-precoding -- per data symbol the MMSE-weighted
// inverse DFT of length M = 12 n_prbs of the equalizer's x_hat, and the per-symbol noise variance the demapper needs.
//
// Kernel: the row frame of ce_fft.h, a row being a data symbol of one slot.
//   load   thread t of the row takes the groups g = t, t + threads_per_row, .. of 4 REs (two 16-byte loads of x_hat,
//          one of nvar), forms u_k, beta_k, gamma_k, adds beta and gamma to its own two partial sums in ascending k and
//          writes u into buffer 0 in natural order.  The partial sums are reduced by a butterfly of lane exchanges
//          inside the wave (offsets 32 .. 1: a balanced tree, every lane ends with the same bits) and, for rows of two or
//          four waves, (w0 + w1) + (w2 + w3) through LDS: the longest addition chain is
//          4 ceil(M / 4 / threads_per_row) + log2(threads_per_row), and nothing depends on the batch.
//   passes the Stockham passes of ce_fft.h (shared with ce_ofdm.hip) over the host's radix sequence, one barrier per pass;
//          the last pass applies sqrt(M) / sum beta and leaves the row in natural order.
//   store  16-byte stores of the row from LDS and of the broadcast nvar_out, contiguous over the lanes.
// In place is safe: the stores come after the last barrier, the loads before the first.  DESIGN 6i.
//
// The forward transform (ce_tp_precode, the transmit side) is ce_tp_precode_kernel: the same launch geometry
// and the same passes between a conjugating load and a conjugating store, rows at host-given offsets (dense rows, or
// the data symbols of a resource grid), no weights and no sums.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>

#include "ce_fft.h"
#include "ce_stage.h"
#include "ce_tp.h"

namespace {

struct TpDev {
  FftDev f;       // m = M, n_rows = S; an item is a slot
  float sqrt_m;   // float32(sqrt(M))
};

// beta, gamma and u of one RE (include/ce_tp.h); an unusable RE is selected away, never multiplied
__device__ __forceinline__ float2 tp_weigh(float xr, float xi, float nv, float& sb, float& sg) {
  const bool ok = nv > 0.0f && nv < INFINITY && fabsf(xr) < INFINITY && fabsf(xi) < INFINITY;   // a NaN fails its comparison
  const float d = 1.0f + nv;
  const float beta = ok ? 1.0f / d : 0.0f;
  const float gamma = ok ? nv / d : 1.0f;
  sb += beta;
  sg += gamma;
  return make_float2(ok ? beta * xr : 0.0f, ok ? beta * xi : 0.0f);
}

__global__ __launch_bounds__(TP_NT) void ce_tp_kernel(TpDev P, const float2* __restrict__ tw, const float4* x_in, const float4* nv_in, float4* x_out,
                                                      float4* nv_out) {
  // x_in / x_out and nv_in / nv_out may be the same buffers: no __restrict__; every load of the workgroup's rows comes
  // before the first barrier, every store after the last
  extern __shared__ float4 tp_lds[];
  __shared__ float red[TP_NT / 64][2];
  const auto [slot, row, lane, tpr, active, buf0, buf1] = fft_row(P.f, tp_lds);
  const uint32_t M = P.f.m;
  const int64_t grow = (int64_t)slot * P.f.n_rows + row;
  const uint32_t n_grp = M >> 2;   // groups of 4 REs

  // ---- load: u into buf0, the two sums ----
  float sb = 0.0f, sg = 0.0f;
  {
    const float4* xr = x_in + grow * (int64_t)(M >> 1);
    const float4* nr = nv_in + grow * (int64_t)n_grp;
    float4* u4 = reinterpret_cast<float4*>(buf0);
    for (uint32_t g = lane; g < n_grp; g += tpr) {
      float4 nv = make_float4(-1.0f, -1.0f, -1.0f, -1.0f), xa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), xb = xa;
      if (active) {
        nv = nr[g];
        xa = xr[2u * g];
        xb = xr[2u * g + 1u];
      }
      const float2 u0 = tp_weigh(xa.x, xa.y, nv.x, sb, sg);
      const float2 u1 = tp_weigh(xa.z, xa.w, nv.y, sb, sg);
      const float2 u2 = tp_weigh(xb.x, xb.y, nv.z, sb, sg);
      const float2 u3 = tp_weigh(xb.z, xb.w, nv.w, sb, sg);
      u4[2u * g] = make_float4(u0.x, u0.y, u1.x, u1.y);
      u4[2u * g + 1u] = make_float4(u2.x, u2.y, u3.x, u3.y);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {   // a + b = b + a: both partners of an exchange get the same bits
    sb += __shfl_xor(sb, off);
    sg += __shfl_xor(sg, off);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    red[wave][0] = sb;
    red[wave][1] = sg;
  }
  __syncthreads();
  if (P.f.tpr_log2 == 7u) {
    const uint32_t w0 = wave & ~1u;
    sb = red[w0][0] + red[w0 + 1u][0];
    sg = red[w0][1] + red[w0 + 1u][1];
  } else if (P.f.tpr_log2 == 8u) {
    sb = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    sg = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  }
  const bool any = sb > 0.0f;
  const float scale = any ? P.sqrt_m / sb : 0.0f;        // 1 / (sqrt(M) mu)
  const float nvo = any ? sg / sb : INFINITY;

  // ---- passes ----
  const float2* dst = tp_passes(P.f, buf0, buf1, tw, lane, tpr, scale);

  // ---- store ----
  if (active) {
    const float4* res = reinterpret_cast<const float4*>(dst);
    float4* xo = x_out + grow * (int64_t)(M >> 1);
    float4* no = nv_out + grow * (int64_t)n_grp;
    for (uint32_t h = lane; h < (M >> 1); h += tpr) xo[h] = res[h];
    const float4 nv4 = make_float4(nvo, nvo, nvo, nvo);
    for (uint32_t g = lane; g < n_grp; g += tpr) no[g] = nv4;
  }
}

// The row geometry of one ce_tp_precode call, by value in the kernel arguments; complex elements.
struct TpRows {
  int64_t x_slot, y_slot;            // slot strides
  int32_t x_off[CE_MAX_SYMBOLS];     // row offsets inside a slot; entries >= S are 0
  int32_t y_off[CE_MAX_SYMBOLS];
  float scale;                       // float32(1 / sqrt(M))
};

// Transform precoding, DFT(x) = conj(IDFT(conj(x))): the passes above between a conjugating load and a conjugating store.
__global__ __launch_bounds__(TP_NT) void ce_tp_precode_kernel(TpDev P, TpRows G, const float2* __restrict__ tw, const float4* x_in, float4* y_out) {
  // x_in and y_out may be the same rows: no __restrict__; every load of the workgroup's rows comes before the first
  // barrier, every store after the last
  extern __shared__ float4 tp_lds[];
  const auto [slot, row, lane, tpr, active, buf0, buf1] = fft_row(P.f, tp_lds);
  const uint32_t ri = active ? row : 0u;
  const uint32_t n_half = P.f.m >> 1;   // 16-byte pairs of REs

  // ---- load: conj(x) into buf0 (an inactive row: zeros) ----
  {
    const float4* xr = x_in + (((int64_t)slot * G.x_slot + (int64_t)G.x_off[ri]) >> 1);   // strides and offsets are even
    float4* u4 = reinterpret_cast<float4*>(buf0);
    for (uint32_t h = lane; h < n_half; h += tpr) {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (active) v = xr[h];
      u4[h] = make_float4(v.x, -v.y, v.z, -v.w);
    }
  }
  __syncthreads();

  // ---- passes ----
  const float2* dst = tp_passes(P.f, buf0, buf1, tw, lane, tpr, G.scale);

  // ---- store: conj ----
  if (active) {
    const float4* res = reinterpret_cast<const float4*>(dst);
    float4* yo = y_out + (((int64_t)slot * G.y_slot + (int64_t)G.y_off[ri]) >> 1);
    for (uint32_t h = lane; h < n_half; h += tpr) {
      const float4 v = res[h];
      yo[h] = make_float4(v.x, -v.y, v.z, -v.w);
    }
  }
}

// ---- host derivation ----

int tp_derive(const ce_tp_desc* d, ce_tp_host_view* v) {
  memset(v, 0, sizeof(*v));
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  if (d->n_prbs < 1 || d->n_prbs > CE_TP_MAX_PRBS) return ce_fail(CE_ERR_INVALID, "n_prbs=%d outside 1..%d", d->n_prbs, CE_TP_MAX_PRBS);
  if (d->n_symbols < 1 || d->n_symbols > CE_MAX_SYMBOLS) return ce_fail(CE_ERR_INVALID, "n_symbols=%d outside 1..%d", d->n_symbols, CE_MAX_SYMBOLS);
  if (!fft_derive(12 * d->n_prbs, d->n_symbols, v))
    return ce_fail(CE_ERR_INVALID, "n_prbs=%d has a prime factor above 5: transform precoding allocates 2^a 3^b 5^c PRBs", d->n_prbs);
  return CE_OK;
}

}  // namespace

struct ce_tp_plan {
  FftPlan core;
  ce_tp_info info{};
  TpDev dev{};
};

extern "C" int ce_tp_derive_host(const ce_tp_desc* d, ce_tp_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  return tp_derive(d, v);
}

extern "C" int ce_tp_copy_twiddles(const ce_tp_desc* d, float* twiddles) {
  if (!d || !twiddles) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_tp_host_view v;
  if (const int rc = tp_derive(d, &v); rc != CE_OK) return rc;
  fft_twiddles(v.m_sc, twiddles);
  return CE_OK;
}

extern "C" int ce_tp_plan_create(const ce_tp_desc* d, ce_tp_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_tp_host_view v;
  if (const int rc = tp_derive(d, &v); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_tp_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->info.m_sc = v.m_sc;
  p->info.n_symbols = d->n_symbols;
  p->info.bytes_per_slot = (int64_t)d->n_symbols * v.m_sc * 24;
  p->dev.f = fft_dev(v, d->n_symbols);
  p->dev.sqrt_m = (float)sqrt((double)v.m_sc);
  const hipError_t e = fft_plan_upload(&p->core, d->device, v);
  if (e != hipSuccess) {
    ce_tp_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "de-precoder plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_tp_plan_destroy(ce_tp_plan* p) { fft_plan_destroy(p); }

extern "C" int ce_tp_plan_get_info(const ce_tp_plan* p, ce_tp_info* info) { return ce_get_info(p, info); }

extern "C" int ce_tp_deprecode(const ce_tp_plan* p, const void* x_hat, const float* nvar, int64_t n_slots, void* x_out, float* nvar_out,
                               void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  if (!x_hat || !nvar || !x_out || !nvar_out) return ce_fail(CE_ERR_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(x_hat) | reinterpret_cast<uintptr_t>(nvar) | reinterpret_cast<uintptr_t>(x_out) | reinterpret_cast<uintptr_t>(nvar_out)) & 15u)
    return ce_fail(CE_ERR_INVALID, "x_hat, nvar, x_out and nvar_out must be 16-byte aligned");
  const int64_t n_wg = n_slots * (int64_t)p->dev.f.wg_per_item;
  if (n_wg > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "%lld slots of %u workgroups: more than 2^31-1 workgroups in one launch", (long long)n_slots, p->dev.f.wg_per_item);
  CeDeviceScope scope(p->core.device);
  if (scope.err != hipSuccess) return ce_device_fail(p->core.device, scope.err);
  hipLaunchKernelGGL(ce_tp_kernel, dim3((unsigned)n_wg), dim3(TP_NT), (size_t)p->core.lds_bytes, (hipStream_t)stream, p->dev, p->core.tw,
                     reinterpret_cast<const float4*>(x_hat), reinterpret_cast<const float4*>(nvar), reinterpret_cast<float4*>(x_out),
                     reinterpret_cast<float4*>(nvar_out));
  return ce_launch_status("transform de-precoding");
}

namespace {

// The row geometry of one tensor of ce_tp_precode (`name` = "x" or "y"): offsets (NULL = dense rows) into `off`, the
// largest into *max_off; CE_OK or the refusal.
int tp_rows(const char* name, int M, int S, int64_t stride, const int32_t* offsets, int32_t* off, int32_t* max_off) {
  if (stride < 0 || (stride & 1)) return ce_fail(CE_ERR_INVALID, "%s_slot_stride=%lld must be even and >= 0", name, (long long)stride);
  *max_off = 0;
  for (int r = 0; r < S; ++r) {
    const int32_t o = offsets ? offsets[r] : r * M;
    if (o < 0 || (o & 1)) return ce_fail(CE_ERR_INVALID, "%s_row_offset[%d]=%d must be even and >= 0", name, r, o);
    if ((int64_t)o + M > stride) return ce_fail(CE_ERR_INVALID, "%s_row_offset[%d]=%d + M=%d exceeds %s_slot_stride=%lld", name, r, o, M, name, (long long)stride);
    for (int q = 0; q < r; ++q)
      if ((int64_t)o < (int64_t)off[q] + M && (int64_t)off[q] < (int64_t)o + M)
        return ce_fail(CE_ERR_INVALID, "%s rows %d and %d overlap (offsets %d and %d, M=%d)", name, q, r, off[q], o, M);
    off[r] = o;
    if (o > *max_off) *max_off = o;
  }
  return CE_OK;
}

}  // namespace

extern "C" int ce_tp_precode(const ce_tp_plan* p, const void* x, int64_t x_slot_stride, const int32_t* x_row_offset, void* y, int64_t y_slot_stride,
                             const int32_t* y_row_offset, int64_t n_slots, void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  if (!x || !y) return ce_fail(CE_ERR_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) return ce_fail(CE_ERR_INVALID, "x and y must be 16-byte aligned");
  const int M = (int)p->dev.f.m, S = (int)p->dev.f.n_rows;
  TpRows G{};
  G.x_slot = x_slot_stride;
  G.y_slot = y_slot_stride;
  G.scale = (float)(1.0 / sqrt((double)M));
  int32_t x_max = 0, y_max = 0;
  if (const int rc = tp_rows("x", M, S, x_slot_stride, x_row_offset, G.x_off, &x_max); rc != CE_OK) return rc;
  if (const int rc = tp_rows("y", M, S, y_slot_stride, y_row_offset, G.y_off, &y_max); rc != CE_OK) return rc;
  const int64_t n_wg = n_slots * (int64_t)p->dev.f.wg_per_item;
  if (n_wg > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "%lld slots of %u workgroups: more than 2^31-1 workgroups in one launch", (long long)n_slots, p->dev.f.wg_per_item);
  // n_slots < 2^31 here; the extents below, in bytes, must stay inside 64 bits
  if (x_slot_stride > (INT64_MAX >> 4) / n_slots || y_slot_stride > (INT64_MAX >> 4) / n_slots)
    return ce_fail(CE_ERR_INVALID, "slot strides %lld and %lld: the extent of %lld slots exceeds the address space", (long long)x_slot_stride, (long long)y_slot_stride, (long long)n_slots);
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
  if (x0 == y0) {
    if (x_slot_stride != y_slot_stride || memcmp(G.x_off, G.y_off, sizeof(G.x_off)) != 0)
      return ce_fail(CE_ERR_INVALID, "y is x with another stride or other row offsets: the in-place form needs the identical geometry");
  } else {
    const uintptr_t x1 = x0 + 8u * (uintptr_t)((n_slots - 1) * x_slot_stride + x_max + M);
    const uintptr_t y1 = y0 + 8u * (uintptr_t)((n_slots - 1) * y_slot_stride + y_max + M);
    if (x0 < y1 && y0 < x1) return ce_fail(CE_ERR_INVALID, "y overlaps x: only y = x with the identical stride and row offsets is an in-place form");
  }
  CeDeviceScope scope(p->core.device);
  if (scope.err != hipSuccess) return ce_device_fail(p->core.device, scope.err);
  hipLaunchKernelGGL(ce_tp_precode_kernel, dim3((unsigned)n_wg), dim3(TP_NT), (size_t)p->core.lds_bytes, (hipStream_t)stream, p->dev, G, p->core.tw,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y));
  return ce_launch_status("transform precoding");
}

// EXTENSION (no reference counterpart, see include/ce_tp.h): the time-domain channel emulator between ce_ofdmtx_modulate and
// ce_ofdm_demodulate -- per (slot, rx port) the FIR sum over the tx ports' samples, the rotation by a numerically controlled
// oscillator (CFO) and seeded white Gaussian noise from Philox4x32-10, in ONE launch, without a plan.
//
// Kernel: one workgroup of 256 threads per (slot, rx port, tile of 1024 output samples).
//   stage  x[b][p][tile_start - halo .. tile_start + 1024) of every tx port p into LDS with 8-byte loads, halo = n_taps rounded
//          down to even (>= n_taps - 1, and even so that sample pairs stay 16-byte aligned in LDS); a sample before the row's
//          start or behind its end is a zero by a bound test, never a load.  The P K taps of (b, r) go behind them.
//          At most 4 (1024 + 128) 8 + 4 128 8 = 40 KiB: four workgroups per CU.
//   sum    thread i owns the sample pairs j = i and i + 256 of the tile, the samples 2 j and 2 j + 1: a sliding window over
//          16-byte LDS reads (one per two taps and pair, contiguous over the lanes: conflict-free) and one broadcast 8-byte
//          read per tap, shared by the thread's four outputs.  float32 FMAs in the fixed order p outer, k inner, per product
//          re += h.re x.re, re -= h.im x.im, im += h.re x.im, im += h.im x.re.
//   finish the phasor of w = phase0 + fcw t (uint32 arithmetic, t from the ROW's start) as sincospi(int32(w) 2^-31), the noise
//          of one Philox call per pair (words 0, 1 for the even sample, 2, 3 for the odd one), one 8-byte store per sample.
// 64-bit addressing; no atomics, no scratch; tensor values enter arithmetic only: every address and every bound comes from
// the block index, the thread index and the host's scalars.  DESIGN 6p.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ce_stage.h"
#include "ce_tp.h"

#define CHAN_NT 256
#define CHAN_TILE 1024
#define CHAN_MAX_TAPS 128
#define CHAN_MAX_TX 4

namespace {

struct ChanWords {
  uint32_t w[4];
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter c, the key k.
__host__ __device__ inline uint32_t chan_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

__host__ __device__ inline ChanWords chan_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = chan_mulhi(M0, c0), lo0 = M0 * c0, hi1 = chan_mulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return ChanWords{{c0, c1, c2, c3}};
}

// The noise words of the sample pair t_pair of (slot, port): counter (t_pair, port, slot low, slot high), key (seed low, seed high).
__host__ __device__ inline ChanWords chan_noise_words(uint32_t key0, uint32_t key1, uint64_t slot, uint32_t port, uint32_t t_pair) {
  return chan_philox(t_pair, port, (uint32_t)slot, (uint32_t)(slot >> 32), key0, key1);
}

struct ChanDev {
  const float2* x;        // [slot][tx port][>= T]
  int64_t x_ss, x_ps;
  const float2* h;        // [slot][rx port][tx port][tap], dense behind the slot stride
  int64_t h_ss;
  const int32_t* fcw;     // per slot, stride 0: one value for the batch
  int64_t fcw_s;
  const uint32_t* ph0;
  int64_t ph0_s;
  const float* sigma;
  int64_t sigma_s;
  float2* y;              // [slot][rx port][>= T]
  int64_t y_ss, y_ps;
  int64_t T;
  uint64_t first_slot;
  uint32_t key0, key1;
  uint32_t P, K, R, tiles, halo;
};

__device__ __forceinline__ void chan_mac(float2& a, const float2 h, const float2 v) {
  a.x = fmaf(h.x, v.x, a.x);
  a.x = fmaf(-h.y, v.y, a.x);
  a.y = fmaf(h.x, v.y, a.y);
  a.y = fmaf(h.y, v.x, a.y);
}

__device__ __forceinline__ float2 chan_lo(const float4 v) { return make_float2(v.x, v.y); }
__device__ __forceinline__ float2 chan_hi(const float4 v) { return make_float2(v.z, v.w); }

template <bool CFO>
__device__ __forceinline__ float2 chan_rotate(const float2 a, const uint32_t w) {
  if (!CFO) return a;
  float s, c;
  sincospif((float)(int32_t)w * 0x1p-31f, &s, &c);
  return make_float2(fmaf(a.x, c, -(a.y * s)), fmaf(a.x, s, a.y * c));
}

// sigma n added to v: n = sqrt(-ln u1) exp(j 2 pi u2), u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (c >> 8) 2^-24
__device__ __forceinline__ float2 chan_add_noise(const float2 v, const float sigma, const uint32_t a, const uint32_t c) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
  const float rad = sqrtf(-logf(u1));
  float sn, cs;
  sincospif((float)(c >> 8) * 0x1p-23f, &sn, &cs);
  return make_float2(fmaf(sigma, rad * cs, v.x), fmaf(sigma, rad * sn, v.y));
}

template <bool CFO, bool NOISE>
__global__ __launch_bounds__(CHAN_NT) void ce_chan_kernel(const ChanDev A) {
  extern __shared__ float4 chan_lds[];
  float2* const xs = reinterpret_cast<float2*>(chan_lds);
  const uint32_t P = A.P, K = A.K, halo = A.halo;
  const uint32_t W = CHAN_TILE + halo;                 // staged samples per tx port, even
  float2* const hs = xs + P * W;
  const uint32_t tid = threadIdx.x;
  const uint32_t tile = blockIdx.x % A.tiles, item = blockIdx.x / A.tiles;
  const uint32_t r = item % A.R, b = item / A.R;
  const int64_t t0 = (int64_t)tile * CHAN_TILE;

  // ---- stage: the tile and its halo of every tx port, zeros outside [0, T); the taps of (b, r) ----
  for (uint32_t p = 0; p < P; ++p) {
    const float2* xr = A.x + ((int64_t)b * A.x_ss + (int64_t)p * A.x_ps);
    for (uint32_t i = tid; i < W; i += CHAN_NT) {
      const int64_t t = t0 - (int64_t)halo + (int64_t)i;
      float2 v = make_float2(0.0f, 0.0f);
      if (t >= 0 && t < A.T) v = xr[t];
      xs[p * W + i] = v;
    }
  }
  {
    const float2* hr = A.h + ((int64_t)b * A.h_ss + (int64_t)r * (int64_t)(P * K));
    for (uint32_t i = tid; i < P * K; i += CHAN_NT) hs[i] = hr[i];
  }
  __syncthreads();

  // ---- sum: pairs j = tid and tid + 256, p outer, k inner ----
  float2 acc[2][2] = {{make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)}, {make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)}};
  for (uint32_t p = 0; p < P; ++p) {
    const float4* xp = reinterpret_cast<const float4*>(xs + p * W + halo);   // pair j of the tile at xp[j]; 16-byte aligned
    const float2* hp = hs + p * K;
    float4 cur[2] = {xp[tid], xp[tid + CHAN_NT]};
    uint32_t k = 0;
    for (; k + 1 < K; k += 2) {
      const float2 h0 = hp[k], h1 = hp[k + 1];
      const int32_t back = (int32_t)(k >> 1) + 1;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float4 prev = xp[(int32_t)(tid + q * CHAN_NT) - back];
        chan_mac(acc[q][0], h0, chan_lo(cur[q]));
        chan_mac(acc[q][1], h0, chan_hi(cur[q]));
        chan_mac(acc[q][0], h1, chan_hi(prev));
        chan_mac(acc[q][1], h1, chan_lo(cur[q]));
        cur[q] = prev;
      }
    }
    if (k < K) {
      const float2 h0 = hp[k];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        chan_mac(acc[q][0], h0, chan_lo(cur[q]));
        chan_mac(acc[q][1], h0, chan_hi(cur[q]));
      }
    }
  }

  // ---- finish: phasor, noise, store ----
  uint32_t fcw = 0u, ph0 = 0u;
  float sigma = 0.0f;
  if (CFO) {
    fcw = (uint32_t)A.fcw[(int64_t)b * A.fcw_s];
    ph0 = A.ph0[(int64_t)b * A.ph0_s];
  }
  if (NOISE) sigma = A.sigma[(int64_t)b * A.sigma_s];
  float2* yr = A.y + ((int64_t)b * A.y_ss + (int64_t)r * A.y_ps);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int64_t t = t0 + 2 * (int64_t)(tid + q * CHAN_NT);
    if (t >= A.T) continue;
    const uint32_t w = ph0 + fcw * (uint32_t)t;        // modulo 2^32: the phase counts from the row's start
    float2 v0 = chan_rotate<CFO>(acc[q][0], w), v1 = chan_rotate<CFO>(acc[q][1], w + fcw);
    if (NOISE) {
      const ChanWords n = chan_noise_words(A.key0, A.key1, A.first_slot + (uint64_t)b, r, (uint32_t)(t >> 1));
      v0 = chan_add_noise(v0, sigma, n.w[0], n.w[1]);
      v1 = chan_add_noise(v1, sigma, n.w[2], n.w[3]);
    }
    yr[t] = v0;
    if (t + 1 < A.T) yr[t + 1] = v1;
  }
}

template <bool CFO, bool NOISE>
void chan_launch(const ChanDev& A, unsigned n_wg, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL((ce_chan_kernel<CFO, NOISE>), dim3(n_wg), dim3(CHAN_NT), lds, stream, A);
}

}  // namespace

extern "C" int ce_chan_noise_words(uint64_t seed, int64_t slot, int32_t port, int64_t t_pair, uint32_t out[4]) {
  if (!out) return ce_fail(CE_ERR_INVALID, "null argument");
  const ChanWords n = chan_noise_words((uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)slot, (uint32_t)port, (uint32_t)t_pair);
  for (int i = 0; i < 4; ++i) out[i] = n.w[i];
  return CE_OK;
}

extern "C" int ce_chan_apply(int32_t abi_version, const void* x, int64_t x_slot_stride, int64_t x_port_stride, int64_t n_slots, int32_t n_tx,
                             int64_t n_rx, int64_t n_samples, const void* taps, int64_t taps_slot_stride, int32_t n_taps, const int32_t* fcw,
                             int64_t fcw_stride, const uint32_t* phase0, int64_t phase0_stride, const float* sigma, int64_t sigma_stride,
                             uint64_t seed, int64_t first_slot, void* y, int64_t y_slot_stride, int64_t y_port_stride, void* stream) {
  if (abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", abi_version, CE_ABI_VERSION);
  if (n_slots < 0 || n_rx < 0 || n_samples < 0)
    return ce_fail(CE_ERR_INVALID, "n_slots=%lld, n_rx=%lld, n_samples=%lld", (long long)n_slots, (long long)n_rx, (long long)n_samples);
  if (n_tx < 1 || n_tx > CHAN_MAX_TX) return ce_fail(CE_ERR_INVALID, "n_tx=%d outside 1..%d", n_tx, CHAN_MAX_TX);
  if (n_taps < 1 || n_taps > CHAN_MAX_TAPS) return ce_fail(CE_ERR_INVALID, "n_taps=%d outside 1..%d", n_taps, CHAN_MAX_TAPS);
  if (n_rx < 1) return ce_fail(CE_ERR_INVALID, "n_rx=%lld must be >= 1", (long long)n_rx);
  if (n_samples < 1) return ce_fail(CE_ERR_INVALID, "n_samples=%lld must be >= 1", (long long)n_samples);
  if (n_slots == 0) return CE_OK;
  if (!x || !y || !taps || (fcw && !phase0)) return ce_fail(CE_ERR_INVALID, "null argument");
  if (x_slot_stride < 0 || x_port_stride < 0 || y_slot_stride < 0 || y_port_stride < 0 || taps_slot_stride < 0 || fcw_stride < 0 ||
      phase0_stride < 0 || sigma_stride < 0)
    return ce_fail(CE_ERR_INVALID, "strides must be >= 0");
  if (reinterpret_cast<uintptr_t>(x) & 7u) return ce_fail(CE_ERR_INVALID, "x must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(y) & 7u) return ce_fail(CE_ERR_INVALID, "y must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(taps) & 7u) return ce_fail(CE_ERR_INVALID, "taps must be 8-byte aligned");
  const int64_t room = INT64_MAX >> 6;
  if (n_samples > room) return ce_fail(CE_ERR_INVALID, "n_samples=%lld exceeds the address space", (long long)n_samples);
  const int64_t tiles = (n_samples + CHAN_TILE - 1) / CHAN_TILE, pk = (int64_t)n_tx * n_taps;
  int64_t n_wg;
  if (const int rc = ce_rows_workgroups(n_slots, n_rx, tiles, &n_wg); rc != CE_OK) return rc;
  if (const int rc = ce_rows_extent(n_slots, n_rx, y_slot_stride, y_port_stride); rc != CE_OK) return rc;
  if (const int rc = ce_rows_extent(n_slots, n_tx, x_slot_stride, x_port_stride); rc != CE_OK) return rc;
  if (const int rc = ce_rows_extent(n_slots, 1, taps_slot_stride, 0); rc != CE_OK) return rc;
  if (taps_slot_stride != 0 && taps_slot_stride < n_rx * pk)
    return ce_fail(CE_ERR_INVALID, "taps_slot_stride=%lld is neither 0 nor >= n_rx n_tx n_taps = %lld", (long long)taps_slot_stride, (long long)(n_rx * pk));
  if (const int rc = ce_rows_disjoint(n_slots, n_rx, y_slot_stride, y_port_stride, n_samples); rc != CE_OK) return rc;
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y), h0 = reinterpret_cast<uintptr_t>(taps);
  const uintptr_t x1 = x0 + 8u * (uintptr_t)((n_slots - 1) * x_slot_stride + (n_tx - 1) * x_port_stride + n_samples);
  const uintptr_t y1 = y0 + 8u * (uintptr_t)((n_slots - 1) * y_slot_stride + (n_rx - 1) * y_port_stride + n_samples);
  const uintptr_t h1 = h0 + 8u * (uintptr_t)((n_slots - 1) * taps_slot_stride + n_rx * pk);
  if (x0 < y1 && y0 < x1) return ce_fail(CE_ERR_INVALID, "y overlaps x");
  if (h0 < y1 && y0 < h1) return ce_fail(CE_ERR_INVALID, "y overlaps taps");

  ChanDev A{};
  A.x = reinterpret_cast<const float2*>(x), A.x_ss = x_slot_stride, A.x_ps = x_port_stride;
  A.h = reinterpret_cast<const float2*>(taps), A.h_ss = taps_slot_stride;
  A.fcw = fcw, A.fcw_s = fcw_stride, A.ph0 = phase0, A.ph0_s = phase0_stride;
  A.sigma = sigma, A.sigma_s = sigma_stride;
  A.y = reinterpret_cast<float2*>(y), A.y_ss = y_slot_stride, A.y_ps = y_port_stride;
  A.T = n_samples, A.first_slot = (uint64_t)first_slot;
  A.key0 = (uint32_t)seed, A.key1 = (uint32_t)(seed >> 32);
  A.P = (uint32_t)n_tx, A.K = (uint32_t)n_taps, A.R = (uint32_t)n_rx, A.tiles = (uint32_t)tiles;
  A.halo = (uint32_t)n_taps & ~1u;
  const size_t lds = 8u * ((size_t)A.P * (CHAN_TILE + A.halo) + (size_t)pk);
  hipStream_t s = (hipStream_t)stream;
  if (fcw && sigma) chan_launch<true, true>(A, (unsigned)n_wg, lds, s);
  else if (fcw) chan_launch<true, false>(A, (unsigned)n_wg, lds, s);
  else if (sigma) chan_launch<false, true>(A, (unsigned)n_wg, lds, s);
  else chan_launch<false, false>(A, (unsigned)n_wg, lds, s);
  return ce_launch_status("channel emulator");
}

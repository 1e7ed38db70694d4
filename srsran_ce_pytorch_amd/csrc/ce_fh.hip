// EXTENSION (no reference counterpart, see include/ce_tp.h): fronthaul I/Q (de)compression, the O-RAN 7.2x wire format of
// frequency-domain samples -- block floating point with a 1..16 bit mantissa, or plain big-endian int16 -- to and from rows
// of the resource grid [slot][port][symbol][subcarrier], each direction in ONE launch, without a plan.
//
// Both kernels: one workgroup of 256 threads per (slot, port, symbol, tile of 64 PRBs); a tile is 768 REs (6 KiB of grid) and
// 64 (hdr + 3 W) <= 3136 payload bytes, a multiple of 4, so every tile starts on a dword of its row.
//   decompress  stage   the tile's payload in LDS with dword loads; the row's last row_bytes mod 4 bytes one by one
//               extract where every row starts on 16 bytes thread i owns the RE pairs i, i + 256 (of 384), otherwise the REs i,
//                       i + 256, i + 512: per RE the 2 W bits out of the 64-bit window of two byte-swapped LDS dwords, two
//                       signed bit-field extracts, << e, convert, one multiply
//               store   one 16-byte store per pair, or one 8-byte store per RE: neighbouring lanes, neighbouring subcarriers
//   compress    stage   thread i loads the same RE pairs (16-byte loads) or REs (8-byte loads), quantises (one multiply, rint,
//                       NaN -> 0, saturate) and keeps (I, Q) as two int16 in one LDS dword per RE
//               max     four lanes per PRB OR the magnitudes v >= 0 ? v : ~v of three REs each, combined over the quad
//                       (bit_length(max) = bit_length(OR)); e = max(L + 1 - W, 0) to LDS
//               pack    thread i owns the output dwords i, i + 256, .. of the tile: per dword the parameter byte where one
//                       falls into it and the mantissa bits of the one or two PRBs it covers, gathered MSB first
//               store   dwords; the bytes of the row's last, partial dword one by one
// 64-bit addressing; no atomics, no scratch; payload values enter arithmetic only: every address and every bound comes from
// the block index, the thread index and the host's scalars.  DESIGN 6s.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "ce_stage.h"
#include "ce_tp.h"

#define FH_NT 256
#define FH_TILE_PRB 64
#define FH_MAX_PRB_BYTES 49

namespace {

struct FhDev {
  uint8_t* pay;           // rows of row_bytes bytes at b p_ss + r p_ps + y p_ys
  int64_t p_ss, p_ps, p_ys;
  float2* grid;           // rows of 12 n_prb REs at b g_ss + r g_ps + y g_ys
  int64_t g_ss, g_ps, g_ys;
  uint32_t R, S, tiles, n_prb;
  uint32_t W, hdr, prb_bytes;       // hdr: 1 with a parameter byte (bfp), 0 without (none)
  uint32_t magic_prb, magic_w;      // floor(2^32 / d) + 1: x / d = (x magic) >> 32 for x d < 2^32; 0 where d = 1
  float scale;                      // scale (decompress) or inv_scale (compress)
};

struct FhTile {
  uint32_t b, r, y, prb0, np;
};

__device__ __forceinline__ FhTile fh_tile(const FhDev& A) {
  FhTile t;
  const uint32_t tile = blockIdx.x % A.tiles, row = blockIdx.x / A.tiles;
  t.y = row % A.S;
  const uint32_t item = row / A.S;
  t.r = item % A.R, t.b = item / A.R;
  t.prb0 = tile * FH_TILE_PRB;
  t.np = min((uint32_t)FH_TILE_PRB, A.n_prb - t.prb0);
  return t;
}

__device__ __forceinline__ uint32_t fh_div(const uint32_t x, const uint32_t magic) { return magic ? __umulhi(x, magic) : x; }

__device__ __forceinline__ float2 fh_expand(const uint32_t iq, const uint32_t W, const uint32_t e, const float scale) {
  const int32_t mi = (int32_t)iq >> (32u - W), mq = (int32_t)(iq << W) >> (32u - W);      // the top W bits, the next W bits
  const int32_t vi = (int32_t)((uint32_t)mi << e), vq = (int32_t)((uint32_t)mq << e);
  return make_float2((float)vi * scale, (float)vq * scale);
}

// N REs per lane and access: 2 where every row starts on 16 bytes (16-byte accesses), 1 otherwise (8-byte accesses)
template <uint32_t N>
__global__ __launch_bounds__(FH_NT) void ce_fh_decompress_kernel(const FhDev A) {
  __shared__ alignas(16) uint32_t pay[FH_TILE_PRB * FH_MAX_PRB_BYTES / 4 + 2];
  const uint32_t tid = threadIdx.x;
  const FhTile t = fh_tile(A);
  const uint32_t nb = t.np * A.prb_bytes, nfull = nb >> 2, ntail = nb & 3u;

  // ---- stage: nfull dwords, the row's last 1..3 bytes (only the last tile of a row has any), two zero dwords behind ----
  {
    const uint8_t* src = A.pay + ((int64_t)t.b * A.p_ss + (int64_t)t.r * A.p_ps + (int64_t)t.y * A.p_ys + (int64_t)t.prb0 * A.prb_bytes);
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>(src);
    for (uint32_t i = tid; i < nfull + 2u; i += FH_NT) {
      uint32_t v = 0u;
      if (i < nfull) {
        v = src32[i];
      } else if (i == nfull) {
        for (uint32_t k = 0; k < ntail; ++k) v |= (uint32_t)src[4u * nfull + k] << (8u * k);
      }
      pay[i] = v;
    }
  }
  __syncthreads();

  // ---- extract and store: item i holds the REs N i .. N i + N - 1 of the tile, all of PRB N i / 12 ----
  float2* const dst = A.grid + ((int64_t)t.b * A.g_ss + (int64_t)t.r * A.g_ps + (int64_t)t.y * A.g_ys + (int64_t)t.prb0 * 12);
  const uint32_t W = A.W, n_items = t.np * (12u / N);
  for (uint32_t i = tid; i < n_items; i += FH_NT) {
    const uint32_t re0 = i * N, prb = re0 / 12u, boff = prb * A.prb_bytes;
    const uint32_t e = A.hdr ? (pay[boff >> 2] >> ((boff & 3u) * 8u)) & 15u : 0u;
    const uint32_t bit = (boff + A.hdr) * 8u + (re0 - prb * 12u) * 2u * W;      // of the item's first mantissa, in the tile
    float2 v[N];
#pragma unroll
    for (uint32_t h = 0; h < N; ++h) {
      const uint32_t at = bit + h * 2u * W, d = at >> 5, off = at & 31u;
      const uint64_t win = ((uint64_t)__builtin_bswap32(pay[d]) << 32) | (uint64_t)__builtin_bswap32(pay[d + 1u]);
      v[h] = fh_expand((uint32_t)((win << off) >> 32), W, e, A.scale);
    }
    if (N == 2) *reinterpret_cast<float4*>(dst + re0) = make_float4(v[0].x, v[0].y, v[N - 1].x, v[N - 1].y);
    else dst[re0] = v[0];
  }
}

// x inv_scale to the nearest even integer, NaN -> 0, saturated to int16; as the low 16 bits
__device__ __forceinline__ uint32_t fh_quantise(const float x, const float inv_scale) {
  const float q = x * inv_scale;
  float r = rintf(q);
  r = (q != q) ? 0.0f : r;
  r = fminf(fmaxf(r, -32768.0f), 32767.0f);
  return (uint32_t)(int32_t)r & 0xFFFFu;
}

__device__ __forceinline__ int32_t fh_lo(const uint32_t d) { return (int32_t)(d << 16) >> 16; }
__device__ __forceinline__ int32_t fh_hi(const uint32_t d) { return (int32_t)d >> 16; }
__device__ __forceinline__ uint32_t fh_mag(const int32_t v) { return (uint32_t)(v ^ (v >> 31)); }      // v >= 0 ? v : ~v

// n_bits <= 32 bits of PRB p's mantissa stream from bit `pos` on, MSB first, as the low bits of the result
__device__ __forceinline__ uint32_t fh_bits(const FhDev& A, const uint32_t* qv, const uint32_t p, const uint32_t e, const uint32_t pos, const uint32_t n_bits) {
  const uint32_t W = A.W, mask = (1u << W) - 1u;
  uint32_t m = fh_div(pos, A.magic_w);
  const uint32_t need = pos - m * W + n_bits;              // <= W - 1 + 32
  uint64_t acc = 0u;
  uint32_t have = 0u;
  while (have < need) {                                    // have <= need + W - 1 <= 62 bits
    const uint32_t d = qv[p * 12u + (m >> 1)];
    const int32_t v = (m & 1u) ? fh_hi(d) : fh_lo(d);
    acc = (acc << W) | (uint64_t)((uint32_t)(v >> e) & mask);
    have += W, ++m;
  }
  const uint32_t out = (uint32_t)(acc >> (have - need));
  return n_bits == 32u ? out : out & ((1u << n_bits) - 1u);
}

template <uint32_t N>
__global__ __launch_bounds__(FH_NT) void ce_fh_compress_kernel(const FhDev A) {
  __shared__ alignas(16) uint32_t lds[FH_TILE_PRB * 12 + FH_TILE_PRB];      // the pair path stores 8 bytes at a time
  uint32_t* const qv = lds;                                // per RE: I in the low, Q in the high 16 bits
  uint32_t* const ex = lds + FH_TILE_PRB * 12;             // per PRB: e
  const uint32_t tid = threadIdx.x;
  const FhTile t = fh_tile(A);
  const uint32_t W = A.W;

  // ---- stage and quantise ----
  {
    const float2* src = A.grid + ((int64_t)t.b * A.g_ss + (int64_t)t.r * A.g_ps + (int64_t)t.y * A.g_ys + (int64_t)t.prb0 * 12);
    const uint32_t n_items = t.np * (12u / N);
    for (uint32_t i = tid; i < n_items; i += FH_NT) {
      if (N == 2) {
        const float4 v = *reinterpret_cast<const float4*>(src + 2u * i);
        uint2 o;
        o.x = fh_quantise(v.x, A.scale) | (fh_quantise(v.y, A.scale) << 16);
        o.y = fh_quantise(v.z, A.scale) | (fh_quantise(v.w, A.scale) << 16);
        *reinterpret_cast<uint2*>(qv + 2u * i) = o;
      } else {
        const float2 v = src[i];
        qv[i] = fh_quantise(v.x, A.scale) | (fh_quantise(v.y, A.scale) << 16);
      }
    }
  }
  __syncthreads();

  // ---- per PRB: the exponent.  Lanes 4 p .. 4 p + 3 take three REs each of PRB p ----
  {
    const uint32_t prb = tid >> 2, part = tid & 3u;
    uint32_t m = 0u;
    if (prb < t.np) {
#pragma unroll
      for (uint32_t i = 0; i < 3; ++i) {
        const uint32_t d = qv[prb * 12u + part * 3u + i];
        m |= fh_mag(fh_lo(d)) | fh_mag(fh_hi(d));
      }
    }
    m |= (uint32_t)__shfl_xor((int)m, 1, 4);
    m |= (uint32_t)__shfl_xor((int)m, 2, 4);
    const uint32_t L = 32u - (uint32_t)__clz((int)m);      // __clz(0) = 32
    if (part == 0u && prb < t.np) ex[prb] = (A.hdr && L + 1u > W) ? L + 1u - W : 0u;
  }
  __syncthreads();

  // ---- pack: dword k of the tile holds its bytes 4 k .. 4 k + 3, the first in the low 8 bits ----
  uint8_t* const dst = A.pay + ((int64_t)t.b * A.p_ss + (int64_t)t.r * A.p_ps + (int64_t)t.y * A.p_ys + (int64_t)t.prb0 * A.prb_bytes);
  const uint32_t nb = t.np * A.prb_bytes, n_dwords = (nb + 3u) >> 2;
  for (uint32_t k = tid; k < n_dwords; k += FH_NT) {
    const uint32_t b0 = 4u * k, total = min(4u, nb - b0);
    uint32_t p = fh_div(b0, A.magic_prb), o = b0 - p * A.prb_bytes, out = 0u, filled = 0u;
    while (filled < total) {
      const uint32_t e = ex[p];
      if (A.hdr && o == 0u) {                              // the parameter byte: the reserved high nibble is 0
        out |= e << (8u * filled);
        ++filled, o = 1u;
        continue;
      }
      const uint32_t n = min(total - filled, A.prb_bytes - o);
      const uint32_t val = fh_bits(A, qv, p, e, (o - A.hdr) * 8u, 8u * n);
      out |= __builtin_bswap32(val << (32u - 8u * n)) << (8u * filled);
      filled += n, o += n;
      if (o == A.prb_bytes) ++p, o = 0u;
    }
    if (total == 4u) {
      reinterpret_cast<uint32_t*>(dst)[k] = out;
    } else {
      for (uint32_t i = 0; i < total; ++i) dst[b0 + i] = (uint8_t)(out >> (8u * i));
    }
  }
}

uint32_t fh_magic(uint32_t d) { return d == 1u ? 0u : (uint32_t)((1ull << 32) / d) + 1u; }

int fh_format(int32_t method, int32_t iq_width, int32_t n_prb, uint32_t* W, uint32_t* hdr) {
  if (method != CE_FH_NONE && method != CE_FH_BFP) return ce_fail(CE_ERR_UNSUPPORTED, "method=%d is neither CE_FH_NONE (0) nor CE_FH_BFP (1)", method);
  if (iq_width < 1 || iq_width > 16) return ce_fail(CE_ERR_INVALID, "iq_width=%d outside 1..16", iq_width);
  if (n_prb < 1 || n_prb > CE_FH_MAX_PRBS) return ce_fail(CE_ERR_INVALID, "n_prb=%d outside 1..%d", n_prb, CE_FH_MAX_PRBS);
  *W = method == CE_FH_BFP ? (uint32_t)iq_width : 16u;
  *hdr = method == CE_FH_BFP ? 1u : 0u;
  return CE_OK;
}

// Rows of `len` units at b s[0] + r s[1] + y s[2]: pairwise disjoint in some nesting of the three dimensions -- taken by
// ascending stride, each stride of a dimension with more than one entry is at least the extent of everything inside it.
int fh_rows_disjoint(const int64_t n[3], const int64_t s[3], int64_t len, const char* what, const char* unit) {
  int order[3] = {0, 1, 2};
  std::sort(order, order + 3, [&](int a, int b) { return s[a] < s[b]; });
  int64_t extent = len;
  for (int i = 0; i < 3; ++i) {
    const int d = order[i];
    if (n[d] == 1) continue;
    if (s[d] < extent)
      return ce_fail(CE_ERR_INVALID, "%s: slot_stride=%lld, port_stride=%lld and symbol_stride=%lld: the rows of %lld %s of %lld slots x %lld ports x %lld symbols overlap",
                     what, (long long)s[0], (long long)s[1], (long long)s[2], (long long)len, unit, (long long)n[0], (long long)n[1], (long long)n[2]);
    extent += (n[d] - 1) * s[d];
  }
  return CE_OK;
}

// The checks and the kernel arguments the two directions share; `compress`: the payload is the written side.
int fh_prepare(bool compress, int32_t abi_version, const void* payload, const int64_t ps[3], const void* grid, const int64_t gs[3], int64_t n_slots,
               int64_t n_ports, int32_t n_sym, int32_t n_prb, int32_t method, int32_t iq_width, float scale, FhDev* A, int64_t* n_wg, bool* wide) {
  if (abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", abi_version, CE_ABI_VERSION);
  uint32_t W, hdr;
  if (const int rc = fh_format(method, iq_width, n_prb, &W, &hdr); rc != CE_OK) return rc;
  if (n_sym < 1) return ce_fail(CE_ERR_INVALID, "n_sym=%d must be >= 1", n_sym);
  if (n_ports < 1) return ce_fail(CE_ERR_INVALID, "n_ports=%lld must be >= 1", (long long)n_ports);
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (!(scale >= 0x1p-96f && scale <= 0x1p96f)) return ce_fail(CE_ERR_INVALID, "%s=%g outside 2^-96 .. 2^96", compress ? "inv_scale" : "scale", (double)scale);
  *n_wg = 0;
  if (n_slots == 0) return CE_OK;
  if (!payload || !grid) return ce_fail(CE_ERR_INVALID, "null argument");
  for (int i = 0; i < 3; ++i)
    if (ps[i] < 0 || gs[i] < 0) return ce_fail(CE_ERR_INVALID, "strides must be >= 0");
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(payload), g0 = reinterpret_cast<uintptr_t>(grid);
  if ((p0 & 3u) || ((ps[0] | ps[1] | ps[2]) & 3)) return ce_fail(CE_ERR_INVALID, "the payload and its strides must be multiples of 4 bytes");
  if (g0 & 7u) return ce_fail(CE_ERR_INVALID, "grid must be 8-byte aligned");
  const int64_t tiles = (n_prb + FH_TILE_PRB - 1) / FH_TILE_PRB, prb_bytes = hdr + 3 * (int64_t)W, row_bytes = n_prb * prb_bytes, n_sc = 12 * (int64_t)n_prb;
  if (const int rc = ce_rows_workgroups(n_slots, n_ports, (int64_t)n_sym * tiles, n_wg); rc != CE_OK) return rc;
  const int64_t n[3] = {n_slots, n_ports, n_sym};
  const int64_t room = INT64_MAX >> 6;
  for (int i = 0; i < 3; ++i)
    if (ps[i] > room / n[i] || gs[i] > room / n[i])
      return ce_fail(CE_ERR_INVALID, "strides whose extent over %lld slots x %lld ports x %lld symbols exceeds the address space", (long long)n[0], (long long)n[1], (long long)n[2]);
  if (const int rc = compress ? fh_rows_disjoint(n, ps, row_bytes, "payload", "bytes") : fh_rows_disjoint(n, gs, n_sc, "grid", "REs"); rc != CE_OK) return rc;
  int64_t p_ext = row_bytes, g_ext = n_sc;
  for (int i = 0; i < 3; ++i) p_ext += (n[i] - 1) * ps[i], g_ext += (n[i] - 1) * gs[i];
  const uintptr_t p1 = p0 + (uintptr_t)p_ext, g1 = g0 + 8u * (uintptr_t)g_ext;
  if (p0 < g1 && g0 < p1) return ce_fail(CE_ERR_INVALID, "payload overlaps grid");

  *A = FhDev{};
  A->pay = static_cast<uint8_t*>(const_cast<void*>(payload)), A->p_ss = ps[0], A->p_ps = ps[1], A->p_ys = ps[2];
  A->grid = static_cast<float2*>(const_cast<void*>(grid)), A->g_ss = gs[0], A->g_ps = gs[1], A->g_ys = gs[2];
  A->R = (uint32_t)n_ports, A->S = (uint32_t)n_sym, A->tiles = (uint32_t)tiles, A->n_prb = (uint32_t)n_prb;
  A->W = W, A->hdr = hdr, A->prb_bytes = (uint32_t)prb_bytes;
  A->magic_prb = fh_magic((uint32_t)prb_bytes), A->magic_w = fh_magic(W);
  A->scale = scale;
  // 16-byte accesses where every row starts on 16 bytes: the base, and the stride of every dimension with more than one entry
  *wide = !(g0 & 15u) && !((n_slots > 1 ? gs[0] : 0) & 1) && !((n_ports > 1 ? gs[1] : 0) & 1) && !((n_sym > 1 ? gs[2] : 0) & 1);
  return CE_OK;
}

}  // namespace

extern "C" int ce_fh_row_bytes(int32_t method, int32_t iq_width, int32_t n_prb, int64_t* bytes) {
  if (!bytes) return ce_fail(CE_ERR_INVALID, "null argument");
  uint32_t W, hdr;
  if (const int rc = fh_format(method, iq_width, n_prb, &W, &hdr); rc != CE_OK) return rc;
  *bytes = (int64_t)n_prb * (hdr + 3 * (int64_t)W);
  return CE_OK;
}

extern "C" int ce_fh_decompress(int32_t abi_version, const void* payload, int64_t payload_slot_stride, int64_t payload_port_stride,
                                int64_t payload_symbol_stride, void* grid, int64_t grid_slot_stride, int64_t grid_port_stride, int64_t grid_symbol_stride,
                                int64_t n_slots, int64_t n_ports, int32_t n_sym, int32_t n_prb, int32_t method, int32_t iq_width, float scale, void* stream) {
  const int64_t ps[3] = {payload_slot_stride, payload_port_stride, payload_symbol_stride}, gs[3] = {grid_slot_stride, grid_port_stride, grid_symbol_stride};
  FhDev A;
  int64_t n_wg;
  bool wide;
  if (const int rc = fh_prepare(false, abi_version, payload, ps, grid, gs, n_slots, n_ports, n_sym, n_prb, method, iq_width, scale, &A, &n_wg, &wide); rc != CE_OK) return rc;
  if (n_wg == 0) return CE_OK;
  hipStream_t s = (hipStream_t)stream;
  if (wide) hipLaunchKernelGGL((ce_fh_decompress_kernel<2>), dim3((unsigned)n_wg), dim3(FH_NT), 0, s, A);
  else hipLaunchKernelGGL((ce_fh_decompress_kernel<1>), dim3((unsigned)n_wg), dim3(FH_NT), 0, s, A);
  return ce_launch_status("fronthaul decompressor");
}

extern "C" int ce_fh_compress(int32_t abi_version, void* payload, int64_t payload_slot_stride, int64_t payload_port_stride, int64_t payload_symbol_stride,
                              const void* grid, int64_t grid_slot_stride, int64_t grid_port_stride, int64_t grid_symbol_stride, int64_t n_slots,
                              int64_t n_ports, int32_t n_sym, int32_t n_prb, int32_t method, int32_t iq_width, float inv_scale, void* stream) {
  const int64_t ps[3] = {payload_slot_stride, payload_port_stride, payload_symbol_stride}, gs[3] = {grid_slot_stride, grid_port_stride, grid_symbol_stride};
  FhDev A;
  int64_t n_wg;
  bool wide;
  if (const int rc = fh_prepare(true, abi_version, payload, ps, grid, gs, n_slots, n_ports, n_sym, n_prb, method, iq_width, inv_scale, &A, &n_wg, &wide); rc != CE_OK) return rc;
  if (n_wg == 0) return CE_OK;
  hipStream_t s = (hipStream_t)stream;
  if (wide) hipLaunchKernelGGL((ce_fh_compress_kernel<2>), dim3((unsigned)n_wg), dim3(FH_NT), 0, s, A);
  else hipLaunchKernelGGL((ce_fh_compress_kernel<1>), dim3((unsigned)n_wg), dim3(FH_NT), 0, s, A);
  return ce_launch_status("fronthaul compressor");
}

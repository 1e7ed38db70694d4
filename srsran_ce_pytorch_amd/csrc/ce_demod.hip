// EXTENSION (no reference counterpart, see include/ce_demod.h): max-log LLRs of the equalizer's x_hat / nvar in codeword
// order, with the PUSCH scrambling of TS 38.211 6.3.1.1 undone, as float32 or as the int8 an LDPC decoder consumes.
//
// Gold sequence.  c = x1 ^ x2, x1 does not depend on c_init and x2 is linear over GF(2) in it.  The host derives once per
// plan the words of x1 (at Nc = 1600) for the whole codeword and, per block of DQ_BW = 8 words, the 31-bit x2 state at the
// block's first bit for each c_init = 1 << i (the jump entries).  A thread XORs the entries of the set bits of c_init and
// steps the x2 recurrence a word at a time (ce_gold.h) through its own block only: nobody walks from n = 0, the cost of a
// bit does not depend on Nc or on where the bit sits in the codeword.  Tables: DESIGN 6f.
//
// Kernel: one 256-thread workgroup per slot and tile of DQ_TILE = 1024 symbols (32 Qm words of c = 4 Qm whole blocks).
//   1. every thread issues the loads of its two pairs of neighbouring symbols (a 16-byte load of x_hat and an 8-byte load
//      of nvar per pair, consecutive lanes on consecutive addresses);
//   2. with descrambling, thread g < 4 Qm builds the 8 words of block g of the tile into the LDS; one barrier;
//   3. per pair: the per-axis closed form, the sign flips, the quantisation, and the 2 Qm results into the LDS in
//      output order (packed, 16-byte aligned per pair where the format allows); one barrier;
//   4. the tile leaves in output order as 16-byte stores on 16-byte aligned addresses.  A slot's row starts at element
//      b G of the output, which is in general not 16-byte aligned: the tile's first and last partial 16 bytes go out
//      element by element (the other elements of those 16 bytes are the neighbouring tile's or slot's), and an interior
//      store takes its 16 bytes from the LDS at the tile's byte offset: one 16-byte read where the tile starts on 16
//      bytes of the output, five aligned words and a byte shift where it does not.
// rnti / n_id only enter the unsigned 32-bit arithmetic of c_init; x_hat / nvar only arithmetic: every address comes
// from the block index, the thread index and host-derived plan values.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "ce_demod.h"
#include "ce_gold.h"
#include "ce_stage.h"

namespace {

constexpr int DQ_NT = 256;
constexpr int DQ_TILE = CE_DEMOD_TILE_SYMBOLS;
constexpr int DQ_BW = CE_DEMOD_BLOCK_WORDS;
static_assert(DQ_TILE == 4 * DQ_NT && (DQ_TILE * 2 / 32) % DQ_BW == 0, "a tile is two pairs per thread and whole Gold blocks");

struct DemodDev {
  uint32_t n_sym;      // M
  uint32_t n_bits;     // G = M Qm
  uint32_t n_tiles;    // workgroups per slot
  uint32_t n_blocks;   // Gold blocks per slot (0: no descrambling)
  float scale;         // llr_scale
};

// Sign-bit LLR of a Gray PAM axis with levels +-1, +-3, .. +-K in units of A^2: (distance to the nearest negative level)^2
// - (distance to the nearest positive level)^2 for v >= 0, odd in v.
template <int K>
__device__ __forceinline__ float dq_fold_llr(float v) {
  const float av = fabsf(v);
  float f;
  if (K == 1) {
    f = 4.0f * av;
  } else {
    const float s = fminf(2.0f * floorf(0.5f * av) + 1.0f, (float)K);
    f = (s + 1.0f) * (2.0f * av + 1.0f - s);
  }
  return copysignf(f, v);
}

// The Qm / 2 LLRs of one axis (bits k = 0 .. m - 1 of the axis are bits 2k (real) / 2k + 1 (imaginary) of the symbol).
template <int QM>
__device__ __forceinline__ void dq_axis(float y, float g, float* llr) {
  constexpr int m = QM / 2;
  constexpr float inv_a = QM == 2 ? 1.41421356237309505f : QM == 4 ? 3.16227766016837933f : QM == 6 ? 6.48074069840786023f : 13.0384048104052974f;
  float v = y * inv_a;
#pragma unroll
  for (int k = 0; k < m; ++k) {
    const int K = (1 << (m - k)) - 1;
    float f;
    switch (K) {   // k is a compile-time constant after unrolling
      case 15: f = dq_fold_llr<15>(v); break;
      case 7: f = dq_fold_llr<7>(v); break;
      case 3: f = dq_fold_llr<3>(v); break;
      default: f = dq_fold_llr<1>(v); break;
    }
    llr[k] = f * g;
    v = (float)((K + 1) / 2) - fabsf(v);
  }
}

// The QM LLRs of one symbol in output order; all zero for an erasure.
template <int QM>
__device__ __forceinline__ void dq_symbol(float re, float im, float nv, float* llr) {
  constexpr float a2 = QM == 2 ? 0.5f : QM == 4 ? 0.1f : QM == 6 ? (1.0f / 42.0f) : (1.0f / 170.0f);
  const bool ok = nv > 0.0f && nv < INFINITY && fabsf(re) < INFINITY && fabsf(im) < INFINITY;   // every comparison is false for a NaN
  const float g = a2 / (ok ? nv : 1.0f);
  float lr[QM / 2], li[QM / 2];
  dq_axis<QM>(ok ? re : 0.0f, g, lr);
  dq_axis<QM>(ok ? im : 0.0f, g, li);
#pragma unroll
  for (int k = 0; k < QM / 2; ++k) {
    llr[2 * k] = ok ? lr[k] : 0.0f;
    llr[2 * k + 1] = ok ? li[k] : 0.0f;
  }
}

__device__ __forceinline__ uint32_t dq_quant(float llr, float scale) {
  const float q = fminf(fmaxf(rintf(llr * scale), -127.0f), 127.0f);
  return (uint32_t)(int32_t)q & 0xFFu;
}

template <int QM, bool I8>
__global__ __launch_bounds__(DQ_NT) void ce_demod_kernel(DemodDev P, const uint32_t* __restrict__ x1, const uint32_t* __restrict__ jump,
                                                         const float2* __restrict__ x_hat, const float* __restrict__ nvar,
                                                         const int32_t* __restrict__ rnti, const int32_t* __restrict__ n_id,
                                                         int64_t st_rnti, int64_t st_id, void* __restrict__ out_) {
  constexpr int TILE_BITS = DQ_TILE * QM;            // output elements of a full tile
  constexpr int TILE_WORDS = TILE_BITS / 32;
  constexpr int BPT = TILE_WORDS / DQ_BW;            // Gold blocks per tile
  constexpr int ES = I8 ? 1 : 4;                     // bytes per output element
  constexpr int EPC = 16 / ES;                       // elements per 16-byte store
  __shared__ uint32_t cw[TILE_WORDS + 1];            // the tile's words of c (+1: the two-word read of the last pair)
  __shared__ uint4 stage4[TILE_BITS * ES / 16 + 1];  // the tile's output (+16 bytes: the fifth word of the last shifted store)
  uint32_t* const stage = reinterpret_cast<uint32_t*>(stage4);

  const uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x / P.n_tiles;
  const uint32_t t = blockIdx.x - b * P.n_tiles;
  const uint32_t sym0 = t * DQ_TILE;                                  // the tile's first symbol in the slot
  const uint32_t n_tile_sym = min((uint32_t)DQ_TILE, P.n_sym - sym0);
  const int64_t in0 = (int64_t)b * P.n_sym + sym0;                    // its first input element
  const bool in_al = (in0 & 1) == 0;                                   // pairs of the tile start on 16 bytes of x_hat / 8 of nvar

  // 1. loads: pair p of the tile = symbols 2p, 2p + 1
  float4 xy[2];
  float2 nv[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t s = 2 * (h * DQ_NT + tid);
    xy[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    nv[h] = make_float2(0.f, 0.f);
    if (s + 1 < n_tile_sym && in_al) {
      xy[h] = *reinterpret_cast<const float4*>(x_hat + in0 + s);
      nv[h] = *reinterpret_cast<const float2*>(nvar + in0 + s);
    } else {
      if (s < n_tile_sym) {
        const float2 a = x_hat[in0 + s];
        xy[h].x = a.x;
        xy[h].y = a.y;
        nv[h].x = nvar[in0 + s];
      }
      if (s + 1 < n_tile_sym) {
        const float2 a = x_hat[in0 + s + 1];
        xy[h].z = a.x;
        xy[h].w = a.y;
        nv[h].y = nvar[in0 + s + 1];
      }
    }
  }

  // 2. the tile's words of c
  const bool descramble = P.n_blocks != 0;
  if (descramble) {
    const uint32_t c_init = (((uint32_t)rnti[b * st_rnti] << 15) + (uint32_t)n_id[b * st_id]) & 0x7FFFFFFFu;
    const uint32_t blk = t * BPT + tid;
    if (tid < BPT && blk < P.n_blocks) {
      uint32_t s = 0;   // row i of `jump`: the entries of c_init bit i, block-fastest; row 31: zeros
#pragma unroll
      for (uint32_t i = 0; i < 31; ++i) s ^= jump[((c_init >> i) & 1u ? i : 31u) * P.n_blocks + blk];
      const uint4* xw = reinterpret_cast<const uint4*>(x1 + (size_t)blk * DQ_BW);   // x1 is padded to whole blocks
      uint32_t w[DQ_BW];
#pragma unroll
      for (int q = 0; q < DQ_BW / 4; ++q) {
        const uint4 x = xw[q];
        w[4 * q] = x.x;
        w[4 * q + 1] = x.y;
        w[4 * q + 2] = x.z;
        w[4 * q + 3] = x.w;
      }
#pragma unroll
      for (int k = 0; k < DQ_BW; ++k) cw[tid * DQ_BW + k] = w[k] ^ ce_gold_step_word<true>(s);
    }
    __syncthreads();
  }

  // 3. LLRs of both pairs into the LDS, in output order
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t p = h * DQ_NT + tid;
    if (2 * p >= n_tile_sym) continue;
    float llr[2 * QM];
    dq_symbol<QM>(xy[h].x, xy[h].y, nv[h].x, llr);
    dq_symbol<QM>(xy[h].z, xy[h].w, nv[h].y, llr + QM);
    uint32_t bits = 0;
    if (descramble) {
      const uint32_t o = 2 * p * QM;   // the pair's first bit in the tile
      const uint64_t two = (uint64_t)cw[o >> 5] | ((uint64_t)cw[(o >> 5) + 1] << 32);
      bits = (uint32_t)(two >> (o & 31u));
    }
#pragma unroll
    for (int j = 0; j < 2 * QM; ++j) llr[j] = __uint_as_float(__float_as_uint(llr[j]) ^ (((bits >> j) & 1u) << 31));
    if (I8) {
      uint32_t* dst = stage + p * (2 * QM / 4);   // 2 Qm bytes per pair
#pragma unroll
      for (int q = 0; q < 2 * QM / 4; ++q)
        dst[q] = dq_quant(llr[4 * q], P.scale) | (dq_quant(llr[4 * q + 1], P.scale) << 8) | (dq_quant(llr[4 * q + 2], P.scale) << 16) |
                 (dq_quant(llr[4 * q + 3], P.scale) << 24);
    } else {
      uint4* dst = stage4 + p * (2 * QM / 4);     // 2 Qm floats per pair
#pragma unroll
      for (int q = 0; q < 2 * QM / 4; ++q)
        dst[q] = make_uint4(__float_as_uint(llr[4 * q]), __float_as_uint(llr[4 * q + 1]), __float_as_uint(llr[4 * q + 2]), __float_as_uint(llr[4 * q + 3]));
    }
  }
  __syncthreads();

  // 4. out: the tile's elements [e0, e0 + n_el) of the flat output, cut into the 16-byte aligned chunks of `out`
  const int64_t e0 = (int64_t)b * P.n_bits + (int64_t)sym0 * QM;
  const int32_t n_el = (int32_t)(n_tile_sym * QM);
  const int64_t c0 = e0 / EPC;                       // first chunk (EPC is a power of two; e0 >= 0)
  const int32_t a = (int32_t)(e0 - c0 * EPC);        // elements of chunk c0 before the tile
  const int32_t n_chunks = (a + n_el + EPC - 1) / EPC;
  uint4* const out16 = reinterpret_cast<uint4*>(out_) + c0;
  for (int32_t j = (int32_t)tid; j < n_chunks; j += DQ_NT) {
    const int32_t lo = j * EPC - a;                  // the chunk's first element, tile-local
    if (lo >= 0 && lo + EPC <= n_el) {
      if (a == 0) {                                  // the tile starts on 16 bytes of `out`: chunk j is 16 aligned bytes of the LDS
        out16[j] = stage4[j];
      } else if (I8) {
        const uint32_t d = (uint32_t)lo >> 2, sh = 8u * ((uint32_t)lo & 3u);
        const uint32_t w0 = stage[d], w1 = stage[d + 1], w2 = stage[d + 2], w3 = stage[d + 3], w4 = stage[d + 4];
        out16[j] = make_uint4((uint32_t)((((uint64_t)w1 << 32) | w0) >> sh), (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh),
                              (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh), (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh));
      } else {
        out16[j] = make_uint4(stage[lo], stage[lo + 1], stage[lo + 2], stage[lo + 3]);
      }
    } else {
      for (int32_t k = 0; k < EPC; ++k) {
        const int32_t e = lo + k;
        if (e < 0 || e >= n_el) continue;
        if (I8)
          reinterpret_cast<uint8_t*>(out16 + j)[k] = (uint8_t)(stage[e >> 2] >> (8 * (e & 3)));
        else
          reinterpret_cast<uint32_t*>(out16 + j)[k] = stage[e];
      }
    }
  }
}

template <int QM>
void dq_launch(const DemodDev& P, bool i8, unsigned n_wg, const uint32_t* x1, const uint32_t* jump, const float2* x_hat, const float* nvar,
               const int32_t* rnti, const int32_t* n_id, int64_t st_rnti, int64_t st_id, void* out, hipStream_t stream) {
  if (i8)
    hipLaunchKernelGGL((ce_demod_kernel<QM, true>), dim3(n_wg), dim3(DQ_NT), 0, stream, P, x1, jump, x_hat, nvar, rnti, n_id, st_rnti, st_id, out);
  else
    hipLaunchKernelGGL((ce_demod_kernel<QM, false>), dim3(n_wg), dim3(DQ_NT), 0, stream, P, x1, jump, x_hat, nvar, rnti, n_id, st_rnti, st_id, out);
}

// ---- host derivation: integers only ----

int dq_derive(const ce_demod_desc* d, ce_demod_host_view* v) {
  memset(v, 0, sizeof(*v));
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  if (d->qm != 2 && d->qm != 4 && d->qm != 6 && d->qm != 8) return ce_fail(CE_ERR_UNSUPPORTED, "qm=%d: modulation orders 2, 4, 6 and 8 are supported", d->qm);
  if (d->out_format != CE_DEMOD_OUT_F32 && d->out_format != CE_DEMOD_OUT_I8) return ce_fail(CE_ERR_INVALID, "out_format=%d is neither float32 (0) nor int8 (1)", d->out_format);
  if (d->descramble != 0 && d->descramble != 1) return ce_fail(CE_ERR_INVALID, "descramble=%d is neither 0 nor 1", d->descramble);
  if (d->n_symbols < 1) return ce_fail(CE_ERR_INVALID, "n_symbols=%d must be positive", d->n_symbols);
  if ((int64_t)d->n_symbols * d->qm > CE_DEMOD_MAX_BITS) return ce_fail(CE_ERR_UNSUPPORTED, "n_symbols=%d at qm=%d: more than %d bits per slot", d->n_symbols, d->qm, CE_DEMOD_MAX_BITS);
  if (d->out_format == CE_DEMOD_OUT_I8 && !(d->llr_scale > 0.0f && d->llr_scale < INFINITY)) return ce_fail(CE_ERR_INVALID, "llr_scale=%g must be positive and finite", (double)d->llr_scale);
  v->n_bits = d->n_symbols * d->qm;
  v->block_words = DQ_BW;
  v->tile_symbols = DQ_TILE;
  v->n_tiles = (d->n_symbols + DQ_TILE - 1) / DQ_TILE;
  if (d->descramble) {
    v->n_words = (v->n_bits + 31) / 32;
    v->n_blocks = (v->n_words + DQ_BW - 1) / DQ_BW;
    v->table_bytes = 4ll * v->n_blocks * DQ_BW + 4ll * 32 * v->n_blocks;
  }
  return CE_OK;
}

// x1[n_blocks * DQ_BW] and jump[n_blocks][31]
void dq_tables(const ce_demod_host_view& v, std::vector<uint32_t>& x1, std::vector<uint32_t>& jump) {
  ce_gold_block_tables((size_t)v.n_blocks, DQ_BW, x1, jump);   // shared with the modulator (ce_gold.h)
}

}  // namespace

struct ce_demod_plan {
  int device = 0;
  int qm = 0;
  bool i8 = false;
  ce_demod_info info{};
  DemodDev dev{};
  CeGoldDev gold;   // with descrambling: the tables of blocks of DQ_BW words
};

extern "C" int ce_demod_derive_host(const ce_demod_desc* d, ce_demod_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  return dq_derive(d, v);
}

extern "C" int ce_demod_copy_tables(const ce_demod_desc* d, uint32_t* x1, uint32_t* jump) {
  if (!d || !x1 || !jump) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_demod_host_view v;
  if (const int rc = dq_derive(d, &v); rc != CE_OK) return rc;
  if (!d->descramble) return ce_fail(CE_ERR_INVALID, "a plan without descrambling holds no tables");
  std::vector<uint32_t> a, j;
  dq_tables(v, a, j);
  memcpy(x1, a.data(), sizeof(uint32_t) * (size_t)v.n_words);
  memcpy(jump, j.data(), sizeof(uint32_t) * j.size());
  return CE_OK;
}

extern "C" int ce_demod_plan_create(const ce_demod_desc* d, ce_demod_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_demod_host_view v;
  if (const int rc = dq_derive(d, &v); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_demod_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->device = d->device;
  p->qm = d->qm;
  p->i8 = d->out_format == CE_DEMOD_OUT_I8;
  p->info.n_bits = v.n_bits;
  p->info.out_elem_bytes = p->i8 ? 1 : 4;
  p->info.bytes_per_slot = 12ll * d->n_symbols + (int64_t)v.n_bits * p->info.out_elem_bytes;
  p->dev.n_sym = (uint32_t)d->n_symbols;
  p->dev.n_bits = (uint32_t)v.n_bits;
  p->dev.n_tiles = (uint32_t)v.n_tiles;
  p->dev.n_blocks = (uint32_t)v.n_blocks;
  p->dev.scale = p->i8 ? d->llr_scale : 1.0f;
  if (!d->descramble) {
    *out = p.release();
    return CE_OK;
  }
  CeDeviceScope scope(d->device);
  const hipError_t e = ce_gold_upload(scope.err, (size_t)v.n_blocks, DQ_BW, &p->gold);
  if (e != hipSuccess) {
    ce_demod_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "demapper plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_demod_plan_destroy(ce_demod_plan* p) {
  if (!p) return;
  ce_gold_free(&p->gold);
  delete p;
}

extern "C" int ce_demod_plan_get_info(const ce_demod_plan* p, ce_demod_info* info) { return ce_get_info(p, info); }

extern "C" int ce_demod_demap(const ce_demod_plan* p, const void* x_hat, const float* nvar, const int32_t* rnti, const int32_t* n_id,
                              const int64_t strides[2], int64_t n_slots, void* out, void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  if (!x_hat || !nvar || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  const bool descramble = p->dev.n_blocks != 0;
  if (descramble && (!rnti || !n_id || !strides)) return ce_fail(CE_ERR_INVALID, "descrambling needs rnti, n_id and their strides");
  if (descramble && (strides[0] < 0 || strides[1] < 0)) return ce_fail(CE_ERR_INVALID, "negative strides are not supported");
  if ((reinterpret_cast<uintptr_t>(x_hat) | reinterpret_cast<uintptr_t>(nvar) | reinterpret_cast<uintptr_t>(out)) & 15u)
    return ce_fail(CE_ERR_INVALID, "x_hat, nvar and out must be 16-byte aligned");
  if (n_slots * (int64_t)p->dev.n_tiles > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "%lld slots of %u tiles: more than 2^31-1 workgroups in one launch", (long long)n_slots, p->dev.n_tiles);
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  const unsigned n_wg = (unsigned)(n_slots * p->dev.n_tiles);
  const float2* x = reinterpret_cast<const float2*>(x_hat);
  const int64_t s0 = descramble ? strides[0] : 0, s1 = descramble ? strides[1] : 0;
  const hipStream_t st = (hipStream_t)stream;
  switch (p->qm) {
    case 2: dq_launch<2>(p->dev, p->i8, n_wg, p->gold.x1, p->gold.jump, x, nvar, rnti, n_id, s0, s1, out, st); break;
    case 4: dq_launch<4>(p->dev, p->i8, n_wg, p->gold.x1, p->gold.jump, x, nvar, rnti, n_id, s0, s1, out, st); break;
    case 6: dq_launch<6>(p->dev, p->i8, n_wg, p->gold.x1, p->gold.jump, x, nvar, rnti, n_id, s0, s1, out, st); break;
    default: dq_launch<8>(p->dev, p->i8, n_wg, p->gold.x1, p->gold.jump, x, nvar, rnti, n_id, s0, s1, out, st); break;
  }
  return ce_launch_status("demapper");
}

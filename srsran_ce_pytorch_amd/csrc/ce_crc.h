// GF(2) polynomial arithmetic of the CRCs of TS 38.212 5.1 on residues kept left-aligned in 32 bits (the x^(L-1)
// coefficient in bit 31), which makes the 16- and the 24-bit polynomials one code path without masks.  `g` is the
// polynomial without its leading term, left-aligned the same way.  Shared by transport-block assembly (ce_tb.hip) and the
// encoder (ce_enc.hip); DESIGN 6k.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// r(x) x mod g
__host__ __device__ __forceinline__ uint32_t ce_crc_xtime(uint32_t r, uint32_t g) { return (r << 1) ^ ((uint32_t)((int32_t)r >> 31) & g); }

// a(x) b(x) mod g for residues of L bits: Horner over the bits of b
__host__ __device__ __forceinline__ uint32_t ce_crc_mulmod(uint32_t a, uint32_t b, uint32_t g, uint32_t L) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < L; ++i) {
    r = ce_crc_xtime(r, g) ^ ((uint32_t)((int32_t)b >> 31) & a);
    b <<= 1;
  }
  return r;
}

// Host: x^e mod g; `one` is the polynomial 1, left-aligned
inline uint32_t ce_crc_pow_x(uint32_t one, uint32_t g, int64_t e) {
  uint32_t r = one;
  for (int64_t i = 0; i < e; ++i) r = ce_crc_xtime(r, g);
  return r;
}

// XOR of v over the 64 lanes of a wave, in every lane
__device__ __forceinline__ uint32_t ce_crc_wave_xor(uint32_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v ^= (uint32_t)__shfl_xor((int)v, off);
  return v;
}

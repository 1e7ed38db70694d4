// The Gold sequence of TS 38.211 5.2.1, c(n) = x1(n + Nc) ^ x2(n + Nc), a word (32 bits) at a time.  The one generator of
// the DM-RS tables (ce_dmrs.hip), the (de)scrambling tables and the kernels of the demapper and the modulator (ce_demod.hip,
// ce_mod.hip); DESIGN 6d.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ce_stage.h"

constexpr int CE_GOLD_NC_WORDS = 50;   // Nc = 1600 bits = 50 words

// One word (32 steps) of a length-31 LFSR whose feedback is x(n + 31) = XOR of x(n + t) over the taps: x1 has taps {0, 3},
// x2 {0, 1, 2, 3}.  `s` holds x(n .. n + 30) in bits 0 .. 30; returns x(n .. n + 31) and leaves x(n + 32 .. n + 62) in s.
template <bool IS_X2>
__host__ __device__ __forceinline__ uint32_t ce_gold_step_word(uint32_t& s) {
  uint64_t v = s;
  uint64_t t = IS_X2 ? v ^ (v >> 1) ^ (v >> 2) ^ (v >> 3) : v ^ (v >> 3);
  v |= (t & 0x0FFFFFFFull) << 31;                        // x(n + 31 .. n + 58) from x(n .. n + 30)
  t = IS_X2 ? v ^ (v >> 1) ^ (v >> 2) ^ (v >> 3) : v ^ (v >> 3);
  v |= ((t >> 28) & 0xFull) << 59;                       // x(n + 59 .. n + 62) from x(n + 28 .. n + 34)
  s = (uint32_t)(v >> 32) & 0x7FFFFFFFu;
  return (uint32_t)v;
}

// Host: the state x(32 w + Nc .. 32 w + Nc + 30) of one m-sequence at the first bit of word `w` of c, from its 31-bit
// initial state x(0 .. 30) (x1: 1; x2: c_init).
template <bool IS_X2>
inline uint32_t ce_gold_state_at(uint32_t init, int w) {
  uint32_t s = init & 0x7FFFFFFFu;
  for (int i = 0; i < CE_GOLD_NC_WORDS + w; ++i) (void)ce_gold_step_word<IS_X2>(s);
  return s;
}

// Host: words w_lo .. w_hi of c for one m-sequence alone (the other all zero) into out[0 .. w_hi - w_lo].
template <bool IS_X2>
inline void ce_gold_words(uint32_t init, int w_lo, int w_hi, uint32_t* out) {
  uint32_t s = ce_gold_state_at<IS_X2>(init, w_lo);
  for (int w = w_lo; w <= w_hi; ++w) out[w - w_lo] = ce_gold_step_word<IS_X2>(s);
}

// Host: the tables of a scrambling sequence cut into blocks of `block_words` words (the demapper's and the modulator's;
// ce_demod.h): x1[n_blocks * block_words], the words of c for c_init = 0, and jump[n_blocks][31], the 31-bit x2 state at each
// block's first bit for c_init = 1 << i.
template <class Vec>
inline void ce_gold_block_tables(size_t n_blocks, int block_words, Vec& x1, Vec& jump) {
  const size_t nw = n_blocks * (size_t)block_words;
  x1.assign(nw, 0u);
  jump.assign(n_blocks * 31, 0u);
  if (nw) ce_gold_words<false>(1u, 0, (int)nw - 1, x1.data());   // x1(0) = 1, x1(1 .. 30) = 0
  for (int i = 0; i < 31; ++i) {
    uint32_t s = ce_gold_state_at<true>(1u << i, 0);
    for (size_t blk = 0; blk < n_blocks; ++blk) {
      jump[blk * 31 + i] = s;
      for (int k = 0; k < block_words; ++k) (void)ce_gold_step_word<true>(s);
    }
  }
}

// Those tables on the device, as the kernels read them.
struct CeGoldDev {
  uint32_t* x1 = nullptr;     // [n_blocks * block_words]
  uint32_t* jump = nullptr;   // [32][n_blocks]: rows 0 .. 30 = the entries of c_init bit i, row 31 = zeros
};

// Host: the next two links of a plan's upload chain (ce_stage.h) -- builds the tables, turns jump block-fastest and uploads
// the pair to the current device.  The pointers stay the plan's to free (ce_gold_free) either way.
inline hipError_t ce_gold_upload(hipError_t e, size_t n_blocks, int block_words, CeGoldDev* t) {
  std::vector<uint32_t> x1, j, rows(32 * n_blocks, 0u);
  ce_gold_block_tables(n_blocks, block_words, x1, j);
  for (size_t blk = 0; blk < n_blocks; ++blk)
    for (int i = 0; i < 31; ++i) rows[(size_t)i * n_blocks + blk] = j[blk * 31 + i];
  e = ce_upload(e, &t->x1, x1.data(), x1.size() * sizeof(uint32_t));
  return ce_upload(e, &t->jump, rows.data(), rows.size() * sizeof(uint32_t));
}

inline void ce_gold_free(CeGoldDev* t) {
  if (t->x1) (void)hipFree(t->x1);
  if (t->jump) (void)hipFree(t->jump);
}

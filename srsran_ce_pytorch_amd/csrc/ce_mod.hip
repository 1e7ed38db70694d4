// EXTENSION (no reference counterpart, see include/ce_mod.h): the PUSCH modulator -- scrambling, QAM and layer mapping, RE
// mapping and DM-RS insertion of TS 38.211 6.3.1.1 - 6.3.1.3, 6.3.1.6 and 6.4.1.1.3 in one store-bound pass from the bit row
// g and the pilots to the resource grid tx[slot][layer][symbol][subcarrier].
//
// Kernel: one 256-thread workgroup per (slot, group of MOD_GROUP = 7 OFDM symbols, tile of MOD_TILE = 256 subcarriers), for
// all L layers.
//   1. Within one symbol the data rows ascend with the subcarrier and the layers are interleaved, so a symbol's tile needs ONE
//      contiguous bit range of g and of c: [(first_row + rows before the tile) L Qm, (first_row + rows before its end) L Qm).
//      The range is cut into the Gold blocks (8 words = 256 bits) it touches, at most 33.  Thread (j, i) loads the 32 bytes of
//      block i of symbol j's range of g (two 16-byte loads, the row is 16-byte aligned and padded to 16 bytes), turns each
//      little-endian dword from MSB-first bytes into the LSB-first order c is kept in -- bit reversal plus byte swap, once per
//      dword -- and, with scrambling, XORs the eight words of c it builds as the demapper does (ce_gold.h: x1 words plus the
//      jump entries of the set bits of c_init, stepped a word at a time).  The words go to the LDS; one barrier.  All seven
//      symbols' blocks are built side by side, so the workgroup waits once for the chain table entry -> g, jump entries ->
//      LDS, not once per symbol (one symbol per workgroup measured 2.5 - 4.0 times a fill of tx: DESIGN 6m).
//   2. Lane p of a half workgroup owns subcarriers 2p, 2p + 1 of the tile; the halves take the (symbol, layer) rows in turn.
//      Per symbol the thread finds from the table entry what its pair of REs carries -- both lie in one PRB, so one division
//      serves the pair and every layer; per layer a data RE picks its Qm bits out of the LDS with a funnel shift over two
//      words (v_alignbit) and forms the level by integer arithmetic; a pilot RE reads pilots[k][col][l] and scales it; all
//      else is +0.  The two REs leave as one 16-byte store; lanes run along the subcarrier axis of one layer row.
// No atomics, no scratch.  rnti / n_id only enter the unsigned arithmetic of c_init, the bits of g only arithmetic: every
// address comes from the block index, the thread index and host-derived plan values.  Which REs carry data, their rows and
// the table entry that says so are ce_remap.h's, shared with the equalizer.  Geometry and measurements: DESIGN 6m.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "ce_gold.h"
#include "ce_mod.h"
#include "ce_remap.h"
#include "ce_stage.h"

namespace {

constexpr int MOD_NT = CE_MOD_THREADS;
constexpr int MOD_TILE = CE_MOD_TILE_SC;
constexpr int MOD_BW = CE_DEMOD_BLOCK_WORDS;
constexpr int MOD_BLOCK_BITS = 32 * MOD_BW;
constexpr int MOD_MAXB = CE_MOD_MAX_TILE_BLOCKS;
constexpr int MOD_GROUP = CE_MOD_GROUP_SYMBOLS;
constexpr int MOD_LDS_WORDS = (MOD_MAXB + 1) * MOD_BW;   // + 1 block: the second word of the last funnel shift
static_assert(MOD_TILE == MOD_NT && MOD_BLOCK_BITS == 256, "a half workgroup covers a tile's layer row two REs per lane; a block is 256 bits");
static_assert(MOD_TILE * CE_MAX_LAYERS * 8 / MOD_BLOCK_BITS + 2 <= MOD_MAXB, "the blocks of the widest tile fit the LDS");
static_assert(MOD_GROUP * MOD_MAXB <= MOD_NT, "one thread per (symbol of the group, block)");

struct ModDev {
  uint32_t n_sym, n_sc, n_layers, n_tiles;   // n_tiles: per symbol
  uint32_t g_row_bytes, n_blocks, scramble, n_dmrs_total;
  uint32_t n_groups, pad0, pad1, pad2;       // n_groups: symbol groups per slot
};

// Per symbol (uint4): x, y, z are the data-RE map's entry (ce_remap_entry: x = lo | hi << 16, the hop's subcarriers [lo, hi);
// 0, 0 outside both hops; y = data_mask | data REs per PRB << 16, z = first_row), w = re_mask[0] | re_mask[1] << 12 |
// pilot column << 24 | is DM-RS << 28.

// Data REs of the allocation below subcarrier lo + d of a symbol (the host's ce_rows_before).
__device__ __forceinline__ uint32_t mod_rows_before(uint32_t d, uint32_t dmask, uint32_t dpp) {
  const uint32_t q = d / 12u, r = d - 12u * q;
  return q * dpp + (uint32_t)__popc(dmask & ((1u << r) - 1u));
}

// What a tile (subcarriers sc0 .. sc0 + MOD_TILE - 1) of one symbol needs of the slot's bits.
struct ModTile {
  uint32_t lo, hi, dmask, dpp;
  uint32_t rb0;    // data REs of the allocation below the tile
  uint32_t bit0;   // the tile's first bit of the slot
  uint32_t blk0;   // the Gold block that holds it
  uint32_t nblk;   // blocks the tile's bits [bit0, bit1) touch: <= 33 (ce_mod_derive_host checks)
};

__device__ __forceinline__ ModTile mod_tile(const uint4 S, uint32_t sc0, uint32_t bits_per_row) {
  ModTile T;
  T.lo = S.x & 0xFFFFu, T.hi = S.x >> 16, T.dmask = S.y & 0xFFFu, T.dpp = S.y >> 16;
  const uint32_t a0 = min(max(sc0, T.lo), T.hi), a1 = min(max(sc0 + MOD_TILE, T.lo), T.hi);   // the tile's part [a0, a1) of the allocation
  T.rb0 = mod_rows_before(a0 - T.lo, T.dmask, T.dpp);
  const uint32_t rb1 = mod_rows_before(a1 - T.lo, T.dmask, T.dpp);
  T.bit0 = (S.z + T.rb0) * bits_per_row;
  const uint32_t bit1 = (S.z + rb1) * bits_per_row;                                          // <= G
  T.blk0 = T.bit0 / MOD_BLOCK_BITS;
  T.nblk = bit1 > T.bit0 ? (bit1 - 1u) / MOD_BLOCK_BITS - T.blk0 + 1u : 0u;
  return T;
}

// The odd integer level of one axis from bits 0, 2, 4, .. of `b` (38.211 5.1.3 - 5.1.6, ce_mod.h).
template <int QM>
__device__ __forceinline__ float mod_level(uint32_t b) {
  constexpr int m = QM / 2;
  int t = 1 - 2 * (int)((b >> (2 * (m - 1))) & 1u);
#pragma unroll
  for (int k = m - 2; k >= 0; --k) t = (1 - 2 * (int)((b >> (2 * k)) & 1u)) * ((1 << (m - 1 - k)) - t);
  return (float)t;
}

// A little-endian dword of MSB-first bytes -> bit n of the 32 in bit n.
__device__ __forceinline__ uint32_t mod_lsb_first(uint32_t d) { return __builtin_bswap32(__brev(d)); }

template <int QM>
__global__ __launch_bounds__(MOD_NT) void ce_mod_kernel(ModDev P, const uint4* __restrict__ symtab, const uint32_t* __restrict__ x1,
                                                       const uint32_t* __restrict__ jump, const uint8_t* __restrict__ g,
                                                       const float2* __restrict__ pilots, int64_t pil_stride, float beta,
                                                       const int32_t* __restrict__ rnti, const int32_t* __restrict__ n_id,
                                                       int64_t st_rnti, int64_t st_id, float2* __restrict__ tx) {
  constexpr uint32_t A_BITS = QM == 2 ? CE_MOD_A_QPSK : QM == 4 ? CE_MOD_A_16QAM : QM == 6 ? CE_MOD_A_64QAM : CE_MOD_A_256QAM;
  __shared__ uint32_t W[MOD_GROUP][MOD_LDS_WORDS];   // per symbol of the group: the tile's scrambled bits, LSB first, from the first bit of its block blk0

  const uint32_t tid = threadIdx.x;
  const uint32_t per_slot = P.n_groups * P.n_tiles;
  const uint32_t b = blockIdx.x / per_slot;
  const uint32_t rem = blockIdx.x - b * per_slot;
  const uint32_t grp = rem / P.n_tiles, t = rem - grp * P.n_tiles;
  const uint32_t s0 = grp * MOD_GROUP, ns = min((uint32_t)MOD_GROUP, P.n_sym - s0);   // the group's symbols s0 .. s0 + ns - 1
  const uint32_t sc0 = t * MOD_TILE, L = P.n_layers;

  // 1. the blocks of g ^ c of every symbol's tile: thread (j, i) builds block i of symbol s0 + j
  {
    const uint32_t j = tid / MOD_MAXB, i = tid - j * MOD_MAXB;
    ModTile T;
    T.nblk = 0u, T.blk0 = 0u;
    if (j < ns) T = mod_tile(symtab[s0 + j], sc0, L * QM);
    if (i < T.nblk) {
      const uint32_t blk = T.blk0 + i;
      const uint8_t* row = g + (size_t)b * P.g_row_bytes;
      uint32_t w[MOD_BW];
#pragma unroll
      for (int q = 0; q < MOD_BW / 4; ++q) {
        const uint32_t off = blk * (4u * MOD_BW) + 16u * q;   // the row ends on 16 bytes, not on a block
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (off < P.g_row_bytes) x = *reinterpret_cast<const uint4*>(row + off);
        w[4 * q] = mod_lsb_first(x.x);
        w[4 * q + 1] = mod_lsb_first(x.y);
        w[4 * q + 2] = mod_lsb_first(x.z);
        w[4 * q + 3] = mod_lsb_first(x.w);
      }
      if (P.scramble) {
        const uint32_t c_init = (((uint32_t)rnti[b * st_rnti] << 15) + (uint32_t)n_id[b * st_id]) & 0x7FFFFFFFu;
        uint32_t st = 0;   // row i of `jump`: the entries of c_init bit i, block-fastest; row 31: zeros
#pragma unroll
        for (uint32_t n = 0; n < 31; ++n) st ^= jump[((c_init >> n) & 1u ? n : 31u) * P.n_blocks + blk];
        const uint4* xw = reinterpret_cast<const uint4*>(x1 + (size_t)blk * MOD_BW);   // x1 is padded to whole blocks
#pragma unroll
        for (int q = 0; q < MOD_BW / 4; ++q) {
          const uint4 x = xw[q];
          w[4 * q] ^= x.x;
          w[4 * q + 1] ^= x.y;
          w[4 * q + 2] ^= x.z;
          w[4 * q + 3] ^= x.w;
        }
#pragma unroll
        for (int k = 0; k < MOD_BW; ++k) w[k] ^= ce_gold_step_word<true>(st);
      }
#pragma unroll
      for (int k = 0; k < MOD_BW; ++k) W[j][i * MOD_BW + k] = w[k];
    }
  }
  __syncthreads();

  // 2. two REs per thread and (symbol, layer): the pairs (j, l), counted j L + l, alternate between the halves of the workgroup
  const uint32_t k = sc0 + 2u * (tid & (MOD_NT / 2 - 1));
  if (k >= P.n_sc) return;   // (n_sc is even: k + 1 < n_sc as well)
  const uint32_t half = tid / (MOD_NT / 2), LQ = L * QM;
  const float a = __uint_as_float(A_BITS);
  const float2* const pil = pilots + (size_t)b * pil_stride;
  const size_t layer_step = 2 * (size_t)P.n_sym * P.n_sc;   // two layers on
  for (uint32_t j = 0; j < ns; ++j) {
    const uint32_t l0 = (half ^ (j * L)) & 1u;   // the half's first layer on this symbol
    if (l0 >= L) continue;
    const uint32_t s = s0 + j;
    const uint4 S = symtab[s];
    const ModTile T = mod_tile(S, sc0, LQ);
    // k is even, lo and hi are multiples of 12: k + 1 lies in the same PRB and on the same side of the allocation's edges
    const bool inside = k >= T.lo && k < T.hi;
    const uint32_t d = inside ? k - T.lo : 0u;
    const uint32_t prb = d / 12u, re = d - 12u * prb;                          // the RE of k inside its PRB: even, <= 10
    const uint32_t dbits = inside ? (T.dmask >> re) & 3u : 0u;                  // bit e: RE k + e carries data
    const uint32_t o0 = (mod_rows_before(d, T.dmask, T.dpp) - T.rb0) * LQ + (T.bit0 & (MOD_BLOCK_BITS - 1u));   // layer 0's symbol of the pair's first data RE, in W[j]
    const uint32_t o1 = o0 + (dbits & 1u) * LQ;                                 // ... of RE k + 1 where it carries data
    const uint32_t dm = inside ? S.w : 0u, col = (dm >> 24) & 15u;              // (dm = 0: no DM-RS symbol, no pilot)
    float2* dst = tx + (((size_t)b * L + l0) * P.n_sym + s) * P.n_sc + k;       // 16-byte aligned: n_sc and k are even
    for (uint32_t l = l0; l < L; l += 2, dst += layer_step) {
      const uint32_t rm = (l < 2 ? dm : dm >> 12) & 0xFFFu;
      float v[4];
#pragma unroll
      for (uint32_t e = 0; e < 2; ++e) {
        float x = 0.0f, y = 0.0f;
        if ((dbits >> e) & 1u) {
          const uint32_t o = (e ? o1 : o0) + l * QM;
          const uint32_t bits = __builtin_amdgcn_alignbit(W[j][(o >> 5) + 1], W[j][o >> 5], o & 31u);   // 32 bits from bit o
          x = mod_level<QM>(bits) * a;
          y = mod_level<QM>(bits >> 1) * a;
        } else if ((rm >> (re + e)) & 1u) {
          const uint32_t row = prb * (uint32_t)__popc(rm) + (uint32_t)__popc(rm & ((1u << (re + e)) - 1u));   // < n_re
          const float2 pv = pil[((size_t)row * P.n_dmrs_total + col) * L + l];
          x = beta * pv.x;
          y = beta * pv.y;
        }
        v[2 * e] = x;
        v[2 * e + 1] = y;
      }
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// ---- host derivation: integers only ----

int mod_derive(const ce_mod_desc* d, ce_mod_host_view* v) {
  memset(v, 0, sizeof(*v));
  for (int s = 0; s < CE_MAX_SYMBOLS; ++s) v->sym_hop[s] = v->dmrs_col[s] = -1;
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  if (d->qm != 2 && d->qm != 4 && d->qm != 6 && d->qm != 8) return ce_fail(CE_ERR_UNSUPPORTED, "qm=%d: modulation orders 2, 4, 6 and 8 are supported", d->qm);
  if (d->scramble != 0 && d->scramble != 1) return ce_fail(CE_ERR_INVALID, "scramble=%d is neither 0 nor 1", d->scramble);
  CeReMap ev;   // the rows the equalizer writes: ce_remap.h
  if (const int rc = ce_remap_derive(*d, &ev); rc != CE_OK) return rc;
  const int n_cdm = (d->n_layers + 1) / 2, ppp = ce_popcount12(d->hop[0].re_mask[0]);
  int col = 0;
  for (int h = 0; h < d->n_hops; ++h) {
    const ce_mod_hop_desc& hd = d->hop[h];
    if (hd.n_prbs != d->hop[0].n_prbs) return ce_fail(CE_ERR_INVALID, "hop %d has %d PRBs, hop 0 has %d: the pilots of both hops share one row count", h, hd.n_prbs, d->hop[0].n_prbs);
    if (hd.mask_prbs)
      for (int q = 0; q < d->n_prb_grid; ++q)
        if ((hd.mask_prbs[q] != 0) != (q >= hd.prb_start && q < hd.prb_start + hd.n_prbs))
          return ce_fail(CE_ERR_INVALID, "hop %d: mask_prbs differs from the run %d..%d at PRB %d: a scattered allocation is not transmitted", h, hd.prb_start,
                         hd.prb_start + hd.n_prbs - 1, q);
    int n_dmrs = 0;
    for (int s = 0; s < d->n_sym; ++s) {
      if (!hd.dmrs_symbols[s]) continue;
      if (s < hd.start_symbol || s >= hd.start_symbol + hd.n_alloc_symbols)
        return ce_fail(CE_ERR_INVALID, "hop %d: DM-RS symbol %d outside its symbols %d..%d", h, s, hd.start_symbol, hd.start_symbol + hd.n_alloc_symbols - 1);
      v->dmrs_col[s] = col++;
      ++n_dmrs;
    }
    if (!n_dmrs) continue;   // a hop without DM-RS reads no mask
    for (int c = 0; c < n_cdm; ++c) {
      const unsigned m = hd.re_mask[c];
      if (m == 0 || m > 0xFFFu) return ce_fail(CE_ERR_INVALID, "hop %d: re_mask[%d]=0x%x is not a non-empty 12-bit RE mask", h, c, m);
      if (m & ~(unsigned)hd.reserved_re_mask)
        return ce_fail(CE_ERR_INVALID, "hop %d: re_mask[%d]=0x%x lies outside reserved_re_mask=0x%x: an RE would carry a pilot and data", h, c, m, hd.reserved_re_mask);
      if (ce_popcount12(m) != ppp) return ce_fail(CE_ERR_INVALID, "hop %d: re_mask[%d]=0x%x has %d REs, hop 0's re_mask[0] has %d", h, c, m, ce_popcount12(m), ppp);
    }
  }
  const int64_t G = (int64_t)ev.n_data_re * d->n_layers * d->qm;
  if (G > CE_DEMOD_MAX_BITS)
    return ce_fail(CE_ERR_UNSUPPORTED, "n_symbols=%lld at qm=%d: more than %d bits per slot", (long long)ev.n_data_re * d->n_layers, d->qm, CE_DEMOD_MAX_BITS);
  v->n_bits = (int32_t)G;
  v->g_row_bytes = 16 * (int32_t)((G + 127) / 128);
  v->n_data_re = ev.n_data_re;
  v->n_symbols = ev.n_data_re * d->n_layers;
  v->n_dmrs_total = col;
  v->n_re = col ? d->hop[0].n_prbs * ppp : 0;
  for (int s = 0; s < CE_MAX_SYMBOLS; ++s) {
    v->sym_hop[s] = ev.sym_hop[s], v->data_mask[s] = ev.data_mask[s];
    v->data_res_per_prb[s] = ev.data_res_per_prb[s], v->first_row[s] = ev.first_row[s];
  }
  v->block_words = MOD_BW;
  if (d->scramble) {
    v->n_words = (v->n_bits + 31) / 32;
    v->n_blocks = (v->n_words + MOD_BW - 1) / MOD_BW;
    v->table_bytes = 4 * v->n_blocks * MOD_BW + 4 * 32 * v->n_blocks;
  }
  v->tile_sc = MOD_TILE;
  v->tiles_per_symbol = (12 * d->n_prb_grid + MOD_TILE - 1) / MOD_TILE;
  v->group_symbols = MOD_GROUP;
  v->n_groups = (d->n_sym + MOD_GROUP - 1) / MOD_GROUP;
  v->workgroups_per_slot = v->n_groups * v->tiles_per_symbol;
  v->threads = MOD_NT;
  v->lds_bytes = (int32_t)(MOD_GROUP * MOD_LDS_WORDS * sizeof(uint32_t));
  // every tile through the kernel's own block count
  for (int s = 0; s < d->n_sym; ++s) {
    if (ev.sym_hop[s] < 0) continue;
    const ce_mod_hop_desc& hd = d->hop[ev.sym_hop[s]];
    const int lo = 12 * hd.prb_start, hi = lo + 12 * hd.n_prbs;
    for (int t = 0; t < v->tiles_per_symbol; ++t) {
      const int a0 = std::min(std::max(t * MOD_TILE, lo), hi), a1 = std::min(std::max((t + 1) * MOD_TILE, lo), hi);
      const int64_t per_row = (int64_t)d->n_layers * d->qm;
      const int64_t bit0 = (ev.first_row[s] + ce_rows_before(a0 - lo, ev.data_mask[s], ev.data_res_per_prb[s])) * per_row;
      const int64_t bit1 = (ev.first_row[s] + ce_rows_before(a1 - lo, ev.data_mask[s], ev.data_res_per_prb[s])) * per_row;
      if (bit1 > G) return ce_fail(CE_ERR_UNSUPPORTED, "symbol %d, tile %d ends at bit %lld of %lld", s, t, (long long)bit1, (long long)G);
      const int nblk = bit1 > bit0 ? (int)((bit1 - 1) / MOD_BLOCK_BITS - bit0 / MOD_BLOCK_BITS + 1) : 0;
      if (nblk > MOD_MAXB - 1) return ce_fail(CE_ERR_UNSUPPORTED, "symbol %d, tile %d touches %d Gold blocks: at most %d fit", s, t, nblk, MOD_MAXB - 1);
      v->max_tile_blocks = std::max(v->max_tile_blocks, nblk);
    }
  }
  return CE_OK;
}

template <int QM>
void mod_launch(const ModDev& P, unsigned n_wg, const uint4* symtab, const uint32_t* x1, const uint32_t* jump, const uint8_t* g, const float2* pilots,
                int64_t pil_stride, float beta, const int32_t* rnti, const int32_t* n_id, int64_t st_rnti, int64_t st_id, float2* tx, hipStream_t stream) {
  hipLaunchKernelGGL((ce_mod_kernel<QM>), dim3(n_wg), dim3(MOD_NT), 0, stream, P, symtab, x1, jump, g, pilots, pil_stride, beta, rnti, n_id, st_rnti,
                     st_id, tx);
}

}  // namespace

struct ce_mod_plan {
  int device = 0;
  int qm = 0;
  ce_mod_info info{};
  ModDev dev{};
  uint4* symtab = nullptr;    // [CE_MAX_SYMBOLS]
  CeGoldDev gold;             // with scrambling: the tables of blocks of MOD_BW words
};

extern "C" int ce_mod_derive_host(const ce_mod_desc* d, ce_mod_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  return mod_derive(d, v);
}

extern "C" int ce_mod_plan_create(const ce_mod_desc* d, ce_mod_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_mod_host_view v;
  if (const int rc = mod_derive(d, &v); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_mod_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  const int64_t n_sc = 12ll * d->n_prb_grid;
  p->device = d->device;
  p->qm = d->qm;
  p->info.n_bits = v.n_bits, p->info.n_symbols = v.n_symbols, p->info.n_data_re = v.n_data_re, p->info.g_row_bytes = v.g_row_bytes;
  p->info.n_re = v.n_re, p->info.n_dmrs_total = v.n_dmrs_total;
  p->info.bytes_per_slot = v.g_row_bytes + 8ll * v.n_re * v.n_dmrs_total * d->n_layers + 8ll * d->n_layers * d->n_sym * n_sc;
  ModDev& P = p->dev;
  P.n_sym = (uint32_t)d->n_sym, P.n_sc = (uint32_t)n_sc, P.n_layers = (uint32_t)d->n_layers, P.n_tiles = (uint32_t)v.tiles_per_symbol;
  P.g_row_bytes = (uint32_t)v.g_row_bytes, P.n_blocks = (uint32_t)v.n_blocks, P.scramble = (uint32_t)d->scramble, P.n_dmrs_total = (uint32_t)v.n_dmrs_total;
  P.n_groups = (uint32_t)v.n_groups;
  uint4 tab[CE_MAX_SYMBOLS];
  memset(tab, 0, sizeof(tab));
  for (int s = 0; s < d->n_sym; ++s) {
    if (v.sym_hop[s] < 0) continue;
    const ce_mod_hop_desc& hd = d->hop[v.sym_hop[s]];
    tab[s] = ce_remap_entry(v, s, hd);
    tab[s].w = v.dmrs_col[s] < 0 ? 0u : (uint32_t)hd.re_mask[0] | ((d->n_layers > 2 ? (uint32_t)hd.re_mask[1] : 0u) << 12) | ((uint32_t)v.dmrs_col[s] << 24) | (1u << 28);
  }
  CeDeviceScope scope(d->device);
  hipError_t e = ce_upload(scope.err, &p->symtab, tab, sizeof(tab));
  if (d->scramble) e = ce_gold_upload(e, (size_t)v.n_blocks, MOD_BW, &p->gold);
  if (e != hipSuccess) {
    ce_mod_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "modulator plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_mod_plan_destroy(ce_mod_plan* p) {
  if (!p) return;
  if (p->symtab) (void)hipFree(p->symtab);
  ce_gold_free(&p->gold);
  delete p;
}

extern "C" int ce_mod_plan_get_info(const ce_mod_plan* p, ce_mod_info* info) { return ce_get_info(p, info); }

extern "C" int ce_mod_modulate(const ce_mod_plan* p, const uint8_t* g, const void* pilots, int64_t pilot_slot_stride, float beta_dmrs,
                               const int32_t* rnti, const int32_t* n_id, const int64_t strides[2], int64_t n_slots, void* tx, void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  const ModDev& P = p->dev;
  if (!g || !tx || (P.n_dmrs_total && !pilots)) return ce_fail(CE_ERR_INVALID, "null argument");
  if (P.scramble && (!rnti || !n_id || !strides)) return ce_fail(CE_ERR_INVALID, "scrambling needs rnti, n_id and their strides");
  if (pilot_slot_stride < 0 || (P.scramble && (strides[0] < 0 || strides[1] < 0))) return ce_fail(CE_ERR_INVALID, "negative strides are not supported");
  if (!(fabsf(beta_dmrs) < INFINITY)) return ce_fail(CE_ERR_INVALID, "beta_dmrs=%g must be finite", (double)beta_dmrs);
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(tx)) & 15u) return ce_fail(CE_ERR_INVALID, "g and tx must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(pilots) & 7u) return ce_fail(CE_ERR_INVALID, "pilots must be 8-byte aligned");
  const int64_t per_slot = (int64_t)P.n_groups * P.n_tiles;
  if (n_slots * per_slot > 0x7FFFFFFFll)
    return ce_fail(CE_ERR_UNSUPPORTED, "%lld slots of %lld tiles: more than 2^31-1 workgroups in one launch", (long long)n_slots, (long long)per_slot);
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  const unsigned n_wg = (unsigned)(n_slots * per_slot);
  const int64_t s0 = P.scramble ? strides[0] : 0, s1 = P.scramble ? strides[1] : 0;
  const float2* pil = reinterpret_cast<const float2*>(pilots);
  float2* out = reinterpret_cast<float2*>(tx);
  const hipStream_t st = (hipStream_t)stream;
  switch (p->qm) {
    case 2: mod_launch<2>(P, n_wg, p->symtab, p->gold.x1, p->gold.jump, g, pil, pilot_slot_stride, beta_dmrs, rnti, n_id, s0, s1, out, st); break;
    case 4: mod_launch<4>(P, n_wg, p->symtab, p->gold.x1, p->gold.jump, g, pil, pilot_slot_stride, beta_dmrs, rnti, n_id, s0, s1, out, st); break;
    case 6: mod_launch<6>(P, n_wg, p->symtab, p->gold.x1, p->gold.jump, g, pil, pilot_slot_stride, beta_dmrs, rnti, n_id, s0, s1, out, st); break;
    default: mod_launch<8>(P, n_wg, p->symtab, p->gold.x1, p->gold.jump, g, pil, pilot_slot_stride, beta_dmrs, rnti, n_id, s0, s1, out, st); break;
  }
  return ce_launch_status("modulator");
}

// The data-RE map of a PUSCH allocation, as integers on the host: which REs of every OFDM symbol carry data, and the row
// each of them has in the slot's data order (symbol ascending, subcarrier ascending).  The equalizer (ce_eq) writes its
// outputs in that order and the modulator (ce_mod) reads its bits in it.  One definition, so the two cannot disagree on a
// row, on what they refuse, or on the per-symbol table entry their kernels decode.
#pragma once
#include <string.h>

#include "ce_eq.h"
#include "ce_plan.h"

// Per symbol sym_hop, data_mask, data_res_per_prb and first_row, and n_data_re: the equalizer's public view is the map.
using CeReMap = ce_eq_host_view;

// REs set in the 12-bit mask of a PRB.
inline int ce_popcount12(unsigned m) { return __builtin_popcount(m & 0xFFFu); }

// Data REs of a symbol's allocation below its subcarrier offset d: ce_eq_kernel and mod_rows_before compute the same.
inline int ce_rows_before(int d, int dmask, int dpp) { return (d / 12) * dpp + ce_popcount12((unsigned)dmask & ((1u << (d % 12)) - 1u)); }

// The map of a ce_eq_desc or a ce_mod_desc, which name what it reads alike (n_layers, n_hops, n_prb_grid, n_sym and per hop
// dmrs_symbols, reserved_re_mask, prb_start, n_prbs, start_symbol, n_alloc_symbols): every check behind the ABI version.
// A refused descriptor leaves the symbols assigned so far in *m.
template <class Desc>
__attribute__((visibility("hidden")))   // no exported symbol
int ce_remap_derive(const Desc& d, CeReMap* m) {
  memset(m, 0, sizeof(*m));
  for (int s = 0; s < CE_MAX_SYMBOLS; ++s) m->sym_hop[s] = -1;
  if (d.n_layers < 1 || d.n_layers > CE_MAX_LAYERS) return ce_fail(CE_ERR_UNSUPPORTED, "n_layers=%d outside 1..%d", d.n_layers, CE_MAX_LAYERS);
  if (d.n_hops < 1 || d.n_hops > CE_MAX_HOPS) return ce_fail(CE_ERR_INVALID, "n_hops=%d outside 1..2", d.n_hops);
  if (d.n_prb_grid < 1 || 12 * d.n_prb_grid > CE_FFT_SIZE) return ce_fail(CE_ERR_UNSUPPORTED, "grid of %d PRB: 12*n_prb must be in 12..%d", d.n_prb_grid, CE_FFT_SIZE);
  if (d.n_sym < 1 || d.n_sym > CE_MAX_SYMBOLS) return ce_fail(CE_ERR_INVALID, "n_sym=%d outside 1..%d", d.n_sym, CE_MAX_SYMBOLS);
  for (int h = 0; h < d.n_hops; ++h) {
    const auto& hd = d.hop[h];
    if (hd.reserved_re_mask > 0xFFFu) return ce_fail(CE_ERR_INVALID, "hop %d: reserved_re_mask=0x%x has bits above the 12 REs of a PRB", h, hd.reserved_re_mask);
    if (hd.prb_start < 0 || hd.n_prbs < 1 || (int64_t)hd.prb_start + hd.n_prbs > d.n_prb_grid)
      return ce_fail(CE_ERR_INVALID, "hop %d: PRBs %d..%lld outside the grid of %d PRB", h, hd.prb_start, (long long)hd.prb_start + hd.n_prbs - 1, d.n_prb_grid);
    if (hd.start_symbol < 0 || hd.n_alloc_symbols < 1 || (int64_t)hd.start_symbol + hd.n_alloc_symbols > d.n_sym)
      return ce_fail(CE_ERR_INVALID, "hop %d: symbols %d..%lld outside the grid of %d symbols", h, hd.start_symbol, (long long)hd.start_symbol + hd.n_alloc_symbols - 1, d.n_sym);
    for (int s = hd.start_symbol; s < hd.start_symbol + hd.n_alloc_symbols; ++s) {
      if (m->sym_hop[s] >= 0) return ce_fail(CE_ERR_UNSUPPORTED, "hops %d and %d share OFDM symbol %d", m->sym_hop[s], h, s);
      m->sym_hop[s] = h;
      m->data_mask[s] = hd.dmrs_symbols[s] ? (int32_t)(0xFFFu & ~(unsigned)hd.reserved_re_mask) : 0xFFF;
      m->data_res_per_prb[s] = ce_popcount12((unsigned)m->data_mask[s]);
    }
  }
  // Every data RE is walked through the row formula.
  int64_t n = 0;
  for (int s = 0; s < d.n_sym; ++s) {
    m->first_row[s] = (int32_t)n;
    if (m->sym_hop[s] < 0) continue;
    for (int sc = 0; sc < 12 * d.hop[m->sym_hop[s]].n_prbs; ++sc)
      if ((m->data_mask[s] >> (sc % 12)) & 1) {
        const int64_t row = (int64_t)m->first_row[s] + ce_rows_before(sc, m->data_mask[s], m->data_res_per_prb[s]);
        if (row != n) return ce_fail(CE_ERR_UNSUPPORTED, "row formula gives %lld for data RE %lld", (long long)row, (long long)n);
        ++n;
      }
  }
  if (n < 1) return ce_fail(CE_ERR_INVALID, "the allocation has no data RE");
  m->n_data_re = (int32_t)n;   // <= 4096 * 14
  return CE_OK;
}

// Symbol s's entry of the per-symbol table both kernels decode, from the map or a view that names its members alike:
// x = lo | hi << 16, the subcarriers [lo, hi) of the hop's PRBs (hi <= 4096), y = data_mask | data REs per PRB << 16,
// z = first_row, w = 0.
template <class View, class Hop>
uint4 ce_remap_entry(const View& v, int s, const Hop& hd) {
  const uint32_t lo = 12u * (uint32_t)hd.prb_start, hi = lo + 12u * (uint32_t)hd.n_prbs;
  return make_uint4(lo | (hi << 16), (uint32_t)v.data_mask[s] | ((uint32_t)v.data_res_per_prb[s] << 16), (uint32_t)v.first_row[s], 0u);
}

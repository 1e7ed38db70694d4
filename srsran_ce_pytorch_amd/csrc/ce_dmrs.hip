// EXTENSION (no reference counterpart, see include/ce_dmrs.h): PUSCH DM-RS pilots generated on the GPU from per-slot
// (slot, N_ID, n_SCID), in the [slot][n_re][n_dmrs_total][n_layers] layout ce_estimate_batch consumes.
//
// The Gold generator of TS 38.211 5.2.1 is linear over GF(2) in c_init: word w of c is
//     X1[w] ^ XOR over the set bits i of c_init of T[i][w]
// with X1 = the words of c for c_init = 0 and T[i] = the words for c_init = 1 << i, XORed with X1.  The host derives both
// once per plan (ce_gold.h: a word at a time, integer only) for the words a hop's pilots touch and uploads them as rows of
// one table per hop: row 0 = X1, rows 1 .. 31 = T[0 .. 30], row 32 = zeros.  No thread ever steps the recurrence: the cost
// of a pilot does not depend on Nc = 1600 or on where the allocation sits in the carrier.
//
// Kernel: one 256-thread workgroup per slot.
//   1. per DM-RS column (c_init is uniform over the workgroup), thread w builds word w of the column's c into the LDS:
//      31 unconditional loads of row (bit i of c_init ? 1 + i : 32) -- the row choice is scalar, the loads of one word are
//      independent and in flight together, consecutive threads read consecutive words of a row;
//   2. one barrier;
//   3. the workgroup walks the slot's output in its own memory order (k, s, l), one 16-byte store per thread and step
//      where the slot's element count is even, so a slot leaves as whole contiguous lines.
// The per-slot parameters only enter the unsigned 32-bit arithmetic of c_init: no value of theirs can index anything.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "ce_dmrs.h"
#include "ce_gold.h"
#include "ce_stage.h"

namespace {

constexpr int DM_NT = 256;
constexpr int DM_ROWS = 33;          // table rows per hop: X1, T[0..30], zeros
constexpr uint32_t DM_A = 0x3f3504f3u;  // float32 0.70710677

struct DmrsDev {
  uint32_t n_re, n_cols, n_cols0;   // pilots per column; columns; columns of hop 0
  uint32_t row_len, row_magic;      // elements per output row k (n_cols * L); floor(2^32 / row_len) + 1 (row_len > 1)
  uint32_t n_elem;                  // elements per slot
  uint32_t n_symb_slot;
  uint32_t sym1[CE_MAX_SYMBOLS];    // per column: OFDM symbol index + 1
  uint32_t nw[CE_MAX_HOPS], toff[CE_MAX_HOPS];  // words per table row of the hop; word offset of the hop's table
};

}  // namespace

struct ce_dmrs_plan {
  int device = 0;
  int n_layers = 0;
  ce_dmrs_info info{};
  DmrsDev dev{};
  uint32_t* tab = nullptr;    // [hop][DM_ROWS][nw]
  uint16_t* ptab = nullptr;   // [hop][n_re]: bit position of c(2m) relative to the hop's first kept word
};

namespace {

// One pilot.  e = (k * n_cols + s) * L + l is its element index inside the slot.
template <int L>
__device__ __forceinline__ void dm_locate(const DmrsDev& P, const uint16_t* __restrict__ ptab, const uint32_t* cw, uint32_t e,
                                          uint32_t& l, uint32_t& two_bits, uint32_t& m_odd) {
  const uint32_t k = P.row_len > 1 ? __umulhi(e, P.row_magic) : e;   // e / row_len (exact: checked on the host for every e)
  const uint32_t j = e - k * P.row_len;
  const uint32_t s = j / L;
  l = j - s * L;
  const uint32_t h = s >= P.n_cols0 ? 1u : 0u;
  const uint32_t br = ptab[h * P.n_re + k];                          // even: c(2m) and c(2m + 1) share a word
  two_bits = cw[s * CE_DMRS_MAX_WORDS + (br >> 5)] >> (br & 31u);
  m_odd = (br >> 1) & 1u;                                            // the kept window starts at a multiple of 32 bits: same parity as m
}

__device__ __forceinline__ float2 dm_value(uint32_t two_bits, uint32_t flip) {
  return make_float2(__uint_as_float(DM_A ^ (((two_bits ^ flip) & 1u) << 31)),
                     __uint_as_float(DM_A ^ ((((two_bits >> 1) ^ flip) & 1u) << 31)));
}

template <int L, bool VEC2>
__global__ __launch_bounds__(DM_NT) void ce_dmrs_kernel(DmrsDev P, const uint32_t* __restrict__ tab, const uint16_t* __restrict__ ptab,
                                                        const int32_t* __restrict__ slot, const int32_t* __restrict__ n_id,
                                                        const int32_t* __restrict__ n_scid, int64_t st_slot, int64_t st_id,
                                                        int64_t st_scid, float2* __restrict__ out) {
  __shared__ uint32_t cw[CE_MAX_SYMBOLS * CE_DMRS_MAX_WORDS];
  const uint32_t tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const uint32_t u_slot = (uint32_t)slot[b * st_slot], u_id = (uint32_t)n_id[b * st_id], u_scid = (uint32_t)n_scid[b * st_scid];
  for (uint32_t col = 0; col < P.n_cols; ++col) {
    const uint32_t h = col >= P.n_cols0 ? 1u : 0u;
    // wrap-around of the 32-bit product is harmless: (x mod 2^32) mod 2^31 = x mod 2^31
    const uint32_t c_init = ((((P.n_symb_slot * u_slot + P.sym1[col]) * (2u * u_id + 1u)) << 17) + 2u * u_id + u_scid) & 0x7FFFFFFFu;
    const uint32_t nw = P.nw[h];
    const uint32_t* __restrict__ t = tab + P.toff[h];
    for (uint32_t w = tid; w < nw; w += DM_NT) {
      uint32_t v = t[w];
#pragma unroll
      for (uint32_t i = 0; i < 31; ++i) v ^= t[((c_init >> i) & 1u ? 1u + i : 32u) * nw + w];
      cw[col * CE_DMRS_MAX_WORDS + w] = v;
    }
  }
  __syncthreads();
  float2* __restrict__ o = out + b * (int64_t)P.n_elem;
  if (VEC2) {   // n_elem even and `out` 16-byte aligned (host)
    float4* __restrict__ o4 = reinterpret_cast<float4*>(o);
    for (uint32_t p = tid; p < P.n_elem / 2; p += DM_NT) {
      uint32_t l0, b0, odd0;
      dm_locate<L>(P, ptab, cw, 2 * p, l0, b0, odd0);
      float2 v0, v1;
      if (L % 2 == 0) {   // layers (l, l + 1) of one CDM group: the same r(m), the second with the sign of (-1)^m
        v0 = dm_value(b0, 0u);
        v1 = dm_value(b0, odd0);
      } else {
        uint32_t l1, b1, odd1;
        dm_locate<L>(P, ptab, cw, 2 * p + 1, l1, b1, odd1);
        v0 = dm_value(b0, (l0 & 1u) ? odd0 : 0u);
        v1 = dm_value(b1, (l1 & 1u) ? odd1 : 0u);
      }
      o4[p] = make_float4(v0.x, v0.y, v1.x, v1.y);
    }
  } else {
    for (uint32_t e = tid; e < P.n_elem; e += DM_NT) {
      uint32_t l0, b0, odd0;
      dm_locate<L>(P, ptab, cw, e, l0, b0, odd0);
      o[e] = dm_value(b0, (l0 & 1u) ? odd0 : 0u);
    }
  }
}

template <int L>
void dm_launch(const ce_dmrs_plan* p, bool vec2, unsigned n_slots, const int32_t* slot, const int32_t* n_id, const int32_t* n_scid,
               const int64_t* st, float2* out, hipStream_t stream) {
  if (vec2)
    hipLaunchKernelGGL((ce_dmrs_kernel<L, true>), dim3(n_slots), dim3(DM_NT), 0, stream, p->dev, p->tab, p->ptab, slot, n_id, n_scid, st[0], st[1], st[2], out);
  else
    hipLaunchKernelGGL((ce_dmrs_kernel<L, false>), dim3(n_slots), dim3(DM_NT), 0, stream, p->dev, p->tab, p->ptab, slot, n_id, n_scid, st[0], st[1], st[2], out);
}

// ---- host derivation: integers only ----

// Set bits per PRB of a standard DM-RS mask (38.211 table 6.4.1.1.3-1 / -2 as 12-bit RE masks), 0 for any other value.
int dm_mask_ppp(unsigned m) {
  if (m == 0x555u || m == 0xAAAu) return 6;
  if (m == 0x0C3u || m == 0x30Cu || m == 0xC30u) return 4;
  return 0;
}

int dm_derive(const ce_dmrs_desc* d, ce_dmrs_host_view* v) {
  memset(v, 0, sizeof(*v));
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  if (d->n_layers < 1 || d->n_layers > CE_MAX_LAYERS) return ce_fail(CE_ERR_UNSUPPORTED, "n_layers=%d outside 1..%d", d->n_layers, CE_MAX_LAYERS);
  if (d->n_hops < 1 || d->n_hops > CE_MAX_HOPS) return ce_fail(CE_ERR_INVALID, "n_hops=%d outside 1..2", d->n_hops);
  if (d->n_prb_grid < 1 || 12 * d->n_prb_grid > CE_FFT_SIZE) return ce_fail(CE_ERR_UNSUPPORTED, "grid of %d PRB: 12*n_prb must be in 12..%d", d->n_prb_grid, CE_FFT_SIZE);
  if (d->grid_start_crb < 0) return ce_fail(CE_ERR_INVALID, "grid_start_crb=%d is negative", d->grid_start_crb);
  if (6ll * ((int64_t)d->grid_start_crb + d->n_prb_grid) > (1ll << 20)) return ce_fail(CE_ERR_UNSUPPORTED, "grid_start_crb=%d: 6*(grid_start_crb + n_prb_grid) must be <= 2^20", d->grid_start_crb);
  if (d->n_symb_slot != 12 && d->n_symb_slot != 14) return ce_fail(CE_ERR_INVALID, "n_symb_slot=%d, expected 14 or 12", d->n_symb_slot);
  if (d->n_sym < 1 || d->n_sym > d->n_symb_slot) return ce_fail(CE_ERR_INVALID, "n_sym=%d outside 1..n_symb_slot=%d", d->n_sym, d->n_symb_slot);
  const int n_cdm = (d->n_layers + 1) / 2;
  int ppp = 0, n_active0 = 0, n_cols = 0;
  uint8_t seen_sym[CE_MAX_SYMBOLS] = {0};
  for (int h = 0; h < d->n_hops; ++h) {
    const ce_dmrs_hop_desc& hd = d->hop[h];
    if (!hd.mask_prbs) return ce_fail(CE_ERR_INVALID, "hop %d: mask_prbs is null", h);
    for (int c = 0; c < n_cdm; ++c) {
      const int pc = dm_mask_ppp(hd.re_mask[c]);
      if (pc == 0) return ce_fail(CE_ERR_INVALID, "hop %d: re_mask[%d]=0x%03x is not a standard DM-RS mask (0x555 0xAAA | 0x0C3 0x30C 0xC30)", h, c, hd.re_mask[c]);
      if (ppp == 0) ppp = pc;
      if (pc != ppp) return ce_fail(CE_ERR_INVALID, "hop %d: re_mask[%d]=0x%03x mixes DM-RS configuration types", h, c, hd.re_mask[c]);
    }
    const int col0 = n_cols;
    for (int s = 0; s < d->n_sym; ++s)
      if (hd.dmrs_symbols[s]) {
        if (seen_sym[s]) return ce_fail(CE_ERR_INVALID, "Hops should not overlap.");
        seen_sym[s] = 1;
        v->col_hop[n_cols] = h;
        v->col_sym[n_cols] = s;
        ++n_cols;
      }
    if (n_cols == col0) return ce_fail(CE_ERR_INVALID, "hop %d has no DM-RS symbol", h);
    // row k <-> the k-th set bit of kron(mask_prbs, re_mask): PRBs ascending, ordinal j inside the PRB ascending
    int k = 0, n_active = 0;
    for (int q = 0; q < d->n_prb_grid; ++q)
      if (hd.mask_prbs[q]) {
        ++n_active;
        for (int j = 0; j < ppp; ++j, ++k) {
          v->m[h][k] = ppp * (d->grid_start_crb + q) + j;
          v->odd_sign[h][k] = (uint8_t)(v->m[h][k] & 1);
        }
      }
    if (n_active < 1) return ce_fail(CE_ERR_INVALID, "hop %d: mask_prbs has no active PRB", h);
    if (h == 0) n_active0 = n_active;
    if (n_active != n_active0) return ce_fail(CE_ERR_INVALID, "hop %d has %d active PRBs, hop 0 has %d (pilots.shape[0] is shared)", h, n_active, n_active0);
    const int n_re = n_active * ppp;
    const int w_lo = (2 * v->m[h][0]) / 32, w_hi = (2 * v->m[h][n_re - 1] + 1) / 32;
    if (w_hi - w_lo + 1 > CE_DMRS_MAX_WORDS) return ce_fail(CE_ERR_UNSUPPORTED, "hop %d spans %d words of the sequence (> %d)", h, w_hi - w_lo + 1, CE_DMRS_MAX_WORDS);
    v->word0[h] = w_lo;
    v->n_words[h] = w_hi - w_lo + 1;
    ce_gold_words<false>(1u, w_lo, w_hi, v->x1[h]);
    for (int i = 0; i < 31; ++i) ce_gold_words<true>(1u << i, w_lo, w_hi, v->t[h][i]);
  }
  v->n_re = n_active0 * ppp;
  v->n_dmrs_total = n_cols;
  v->ppp = ppp;
  return CE_OK;
}

}  // namespace

extern "C" int ce_dmrs_derive_host(const ce_dmrs_desc* d, ce_dmrs_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  return dm_derive(d, v);
}

extern "C" int ce_dmrs_plan_create(const ce_dmrs_desc* d, ce_dmrs_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  std::unique_ptr<ce_dmrs_host_view> v(new (std::nothrow) ce_dmrs_host_view);
  if (!v) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  if (const int rc = dm_derive(d, v.get()); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_dmrs_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->device = d->device;
  p->n_layers = d->n_layers;
  p->info.n_re = v->n_re;
  p->info.n_dmrs_total = v->n_dmrs_total;
  p->info.bytes_per_slot = (int64_t)v->n_re * v->n_dmrs_total * d->n_layers * 8;
  DmrsDev& P = p->dev;
  P.n_re = (uint32_t)v->n_re;
  P.n_cols = (uint32_t)v->n_dmrs_total;
  P.n_cols0 = 0;
  for (int c = 0; c < v->n_dmrs_total; ++c) {
    P.n_cols0 += v->col_hop[c] == 0 ? 1u : 0u;
    P.sym1[c] = (uint32_t)v->col_sym[c] + 1u;
  }
  P.row_len = P.n_cols * (uint32_t)d->n_layers;
  P.row_magic = P.row_len > 1 ? (uint32_t)(0x100000000ull / P.row_len) + 1u : 0u;
  P.n_elem = P.n_re * P.row_len;
  P.n_symb_slot = (uint32_t)d->n_symb_slot;
  for (uint32_t e = 0; P.row_len > 1 && e < P.n_elem; ++e)   // the kernel's division by multiplication, for every element it will see
    if ((uint32_t)(((uint64_t)e * P.row_magic) >> 32) != e / P.row_len) return ce_fail(CE_ERR_UNSUPPORTED, "row length %u: magic division fails at %u", P.row_len, e);
  std::vector<uint32_t> tab;
  std::vector<uint16_t> ptab((size_t)d->n_hops * v->n_re);
  for (int h = 0; h < d->n_hops; ++h) {
    const int nw = v->n_words[h];
    P.nw[h] = (uint32_t)nw;
    P.toff[h] = (uint32_t)tab.size();
    tab.insert(tab.end(), v->x1[h], v->x1[h] + nw);
    for (int i = 0; i < 31; ++i) tab.insert(tab.end(), v->t[h][i], v->t[h][i] + nw);
    tab.insert(tab.end(), (size_t)nw, 0u);
    for (int k = 0; k < v->n_re; ++k) ptab[(size_t)h * v->n_re + k] = (uint16_t)(2 * v->m[h][k] - 32 * v->word0[h]);   // < 32 * CE_DMRS_MAX_WORDS
  }
  CeDeviceScope scope(d->device);
  hipError_t e = ce_upload(scope.err, &p->tab, tab.data(), tab.size() * sizeof(uint32_t));
  e = ce_upload(e, &p->ptab, ptab.data(), ptab.size() * sizeof(uint16_t));
  if (e != hipSuccess) {
    ce_dmrs_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "DM-RS plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_dmrs_plan_destroy(ce_dmrs_plan* p) {
  if (!p) return;
  if (p->tab) (void)hipFree(p->tab);
  if (p->ptab) (void)hipFree(p->ptab);
  delete p;
}

extern "C" int ce_dmrs_plan_get_info(const ce_dmrs_plan* p, ce_dmrs_info* info) { return ce_get_info(p, info); }

extern "C" int ce_dmrs_generate(const ce_dmrs_plan* p, const int32_t* slot, const int32_t* n_id, const int32_t* n_scid,
                                const int64_t strides[3], int64_t n_slots, void* pilots_out, void* stream) {
  if (!p || !strides) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  if (!slot || !n_id || !n_scid || !pilots_out) return ce_fail(CE_ERR_INVALID, "null argument");
  if (strides[0] < 0 || strides[1] < 0 || strides[2] < 0) return ce_fail(CE_ERR_INVALID, "negative strides are not supported");
  if (n_slots > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "more than 2^31-1 slots in one launch");
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  const bool vec2 = p->dev.n_elem % 2 == 0 && (reinterpret_cast<uintptr_t>(pilots_out) & 15u) == 0;
  float2* out = reinterpret_cast<float2*>(pilots_out);
  const hipStream_t st = (hipStream_t)stream;
  switch (p->n_layers) {
    case 1: dm_launch<1>(p, vec2, (unsigned)n_slots, slot, n_id, n_scid, strides, out, st); break;
    case 2: dm_launch<2>(p, vec2, (unsigned)n_slots, slot, n_id, n_scid, strides, out, st); break;
    case 3: dm_launch<3>(p, vec2, (unsigned)n_slots, slot, n_id, n_scid, strides, out, st); break;
    default: dm_launch<4>(p, vec2, (unsigned)n_slots, slot, n_id, n_scid, strides, out, st); break;
  }
  return ce_launch_status("DM-RS");
}

// EXTENSION (no reference counterpart, see include/ce_rm.h): LDPC rate recovery with HARQ combining -- the demapper's
// llr[slot][G] split into code blocks, deinterleaved (TS 38.212 5.4.2.2), placed in the circular buffer at the
// redundancy version's k0 around the filler bits (5.4.2.1), repetitions and the kept HARQ buffer added.
//
// Kernel: a gather over output positions, which gives the defined summation order for free and makes the in-place
// update safe (every output element is read and written by one thread only).  One 256-thread workgroup handles a tile of
// one code block's buffer out[slot][r][.], so E_r, its reciprocal and the block's first element of the row are scalars.
// The buffer's N_cb elements start at flat element (slot C + r) N_cb of `out`, in general not 4-byte aligned in int8
// (N_cb = 350): the range is cut at the 4-byte grid of `out` into units (one float32 / four int8 elements), a tile is
// RM_TILE = 1024 units, thread t handles units t, t + 256, t + 512, t + 768 of it -- a wave's loads of harq_in and its
// stores are 256 contiguous bytes each.  The buffer's first and last unit may hold elements of the neighbouring buffer,
// which writes them the same way: those units go in and out byte by byte, every other one as one dword.
// Per element n: filler -> the filler value; otherwise k = (rank(n) - s) mod P and one load of the slot's row per k,
// k + P, .. < E_r at base_r + i Qm + j with j = floor(k / (E_r/Qm)), i = k mod (E_r/Qm).  (j, i) is divided out once per
// unit and stepped from element to element (k + 1: i + 1, carrying into j at E_r/Qm; back to 0 at P); only a second hit
// k + P (repetition) divides again.  A thread issues the first-hit loads of all its units (4 float32 / 16 int8 elements,
// without a branch: an element without a hit loads f_0 and drops it) before it uses any, so they are in flight together.
// Consecutive lanes read one interleaver row at a stride of Qm (float32) or 4 Qm (int8) elements; the other Qm - 1 rows
// of the same cache lines are read by other workgroups of the same slot, so the workgroup-to-slot map keeps a slot on one
// XCD (blockIdx & 7 is the XCD under round-robin dispatch: XCD x works through slots x, x + 8, ..), where the slot's row
// (at most 8 MiB at the largest G in float32, 0.3 .. 1.3 MB at 273 PRB) stays in that XCD's L2 while its tiles run.
// E_r, P, the fillers and the start ranks are ce_ratematch.h's, derived and laid out once for this kernel and the encoder's.
// DESIGN 6g.
//
// The division of k by E_r/Qm is a float32 multiplication by a host-derived reciprocal with a correction of +-1: the
// dividend is below 2^24, so the estimate is off by at most one (tests/test_rm.py restates the arithmetic in numpy
// float32 and checks every index of every case against the oracle).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <type_traits>

#include "ce_ratematch.h"
#include "ce_rm.h"
#include "ce_stage.h"

namespace {

constexpr int RM_NT = 256;
constexpr int RM_TILE = CE_RM_TILE_UNITS;
constexpr int RM_UPT = RM_TILE / RM_NT;   // units per thread
static_assert(RM_TILE % RM_NT == 0, "a tile is whole units per thread");

struct RmDev {
  uint32_t n_cb, c, f1;           // N_cb, C, the fillers' end f0 + nf
  RmWalkDev rm;
  float inv_eq_lo, inv_eq_hi;     // float32(1 / eq)
  uint32_t tiles_per_block;       // workgroups per code block
  uint32_t n_tiles;               // workgroups per slot = C * tiles_per_block
  float filler;                   // float32 format: the filler value
};

template <bool I8>
__global__ __launch_bounds__(RM_NT) void ce_rm_kernel(RmDev P, const void* __restrict__ llr_, const int32_t* __restrict__ rv, int64_t rv_stride,
                                                      uint32_t n_slots, const void* harq_, void* out_) {
  using Acc = typename std::conditional<I8, int32_t, float>::type;
  using El = typename std::conditional<I8, int8_t, float>::type;
  constexpr int32_t EPU = I8 ? 4 : 1;   // elements per 4-byte unit
  // harq_ and out_ may be the same buffer: no __restrict__, and a thread loads the kept values of its units before it
  // stores any of them
  const uint32_t* const harq = reinterpret_cast<const uint32_t*>(harq_);
  uint32_t* const out = reinterpret_cast<uint32_t*>(out_);

  // workgroup -> (slot, code block, tile): all scalar
  const uint32_t xcd = blockIdx.x & 7u, y = blockIdx.x >> 3;
  const uint32_t grp = y / P.n_tiles, w = y - grp * P.n_tiles;
  const uint32_t b = grp * 8u + xcd;
  if (b >= n_slots) return;
  const uint32_t r = w / P.tiles_per_block, tile = w - r * P.tiles_per_block;
  const bool lo = r < P.rm.n_lo;
  const uint32_t e_r = lo ? P.rm.e_lo : P.rm.e_hi, eq = lo ? P.rm.eq_lo : P.rm.eq_hi;
  const float inv = lo ? P.inv_eq_lo : P.inv_eq_hi;
  const uint32_t base = lo ? r * P.rm.e_lo : P.rm.base_hi + (r - P.rm.n_lo) * P.rm.e_hi;
  const El* __restrict__ const row = reinterpret_cast<const El*>(llr_) + (int64_t)b * P.rm.g + base;   // f_0 .. f_{E_r - 1} of the block
  const uint32_t s = ce_rm_walk_start(P, (uint32_t)rv[(int64_t)b * rv_stride]);
  const int64_t r0 = ((int64_t)b * P.c + r) * P.n_cb;   // the buffer's first element in the flat output
  const int64_t u0 = r0 / EPU;                          // its first unit (r0 >= 0), which holds `lead` elements of the buffer before
  const int32_t lead = (int32_t)(r0 - u0 * EPU);
  const int32_t n_units = (lead + (int32_t)P.n_cb + EPU - 1) / EPU;

  int32_t q[RM_UPT];       // unit of the buffer
  uint32_t kept[RM_UPT];   // its 4 bytes of harq_in
#pragma unroll
  for (int h = 0; h < RM_UPT; ++h) {
    q[h] = (int32_t)(tile * RM_TILE + h * RM_NT + threadIdx.x);
    kept[h] = 0u;
    if (harq == nullptr || q[h] >= n_units) continue;
    const int32_t n0 = q[h] * EPU - lead;   // the unit's first element, buffer-local
    if (!I8 || (n0 >= 0 && n0 + EPU <= (int32_t)P.n_cb)) {
      kept[h] = harq[u0 + q[h]];
    } else {   // the buffer's first or last unit, shared with its neighbour
#pragma unroll
      for (int32_t e = 0; e < EPU; ++e)
        if (n0 + e >= 0 && n0 + e < (int32_t)P.n_cb) kept[h] |= (uint32_t)reinterpret_cast<const uint8_t*>(harq_)[(u0 + q[h]) * EPU + e] << (8 * e);
    }
  }

  // every first hit of the thread's units is loaded before any is used: one load per element, in flight together.  An
  // element without a hit (filler, outside the buffer, k >= E_r) loads f_0 and drops it.
  uint32_t k_first[RM_UPT], hits[RM_UPT];
  El first[RM_UPT][EPU];
#pragma unroll
  for (int h = 0; h < RM_UPT; ++h) {
    const int32_t n0 = q[h] * EPU - lead;
    // (k, j, i) of the first non-filler position at or after the unit's first element inside the buffer
    const uint32_t nf = (uint32_t)max(n0, 0);
    const uint32_t rank = nf < P.rm.f0 ? nf : nf < P.f1 ? P.rm.f0 : nf - P.rm.nf;
    uint32_t k = rank >= s ? rank - s : rank + P.rm.p - s;
    if (k >= P.rm.p) k -= P.rm.p;   // rank = P where the fillers run to the buffer's end (N_cb = K - 2 Zc): no position follows
    uint32_t j, i;
    ce_divmod(k, eq, inv, j, i);
    k_first[h] = k;
    hits[h] = 0u;
#pragma unroll
    for (int32_t e = 0; e < EPU; ++e) {
      const uint32_t n = (uint32_t)(n0 + e);   // an element before the buffer wraps to a large value
      const bool live = q[h] < n_units && n < P.n_cb && !(n >= P.rm.f0 && n < P.f1);
      const bool hit = live && k < e_r;
      hits[h] |= (hit ? 1u : 0u) << e;
      first[h][e] = row[hit ? i * P.rm.qm + j : 0u];   // e_k = f_{j + i Qm}: interleaver row j < Qm, column i < E_r / Qm
      if (I8 && live) {   // the next non-filler position's k
        ++k;
        if (++i == eq) {
          i = 0;
          ++j;
        }
        if (k == P.rm.p) k = i = j = 0;
      }
    }
  }

#pragma unroll
  for (int h = 0; h < RM_UPT; ++h) {
    if (q[h] >= n_units) continue;
    const int32_t n0 = q[h] * EPU - lead;
    uint32_t k = k_first[h];
    uint32_t word = 0u, valid = 0u;
#pragma unroll
    for (int32_t e = 0; e < EPU; ++e) {
      const uint32_t n = (uint32_t)(n0 + e);
      if (n >= P.n_cb) continue;
      valid |= 1u << e;
      Acc acc;
      if (n >= P.rm.f0 && n < P.f1) {
        acc = I8 ? (Acc)127 : (Acc)P.filler;
      } else {
        acc = I8 ? (Acc)(int32_t)(int8_t)(kept[h] >> (8 * e)) : (Acc)__uint_as_float(kept[h]);
        if (hits[h] >> e & 1u) {
          acc += (Acc)first[h][e];
          if (e_r > P.rm.p) {   // repetition: k + P, k + 2 P, ..
            for (uint32_t k2 = k + P.rm.p; k2 < e_r; k2 += P.rm.p) {
              uint32_t j2, i2;
              ce_divmod(k2, eq, inv, j2, i2);
              acc += (Acc)row[i2 * P.rm.qm + j2];
            }
          }
          if constexpr (I8) acc = min(max(acc, -127), 127);
        }
        if (I8 && ++k == P.rm.p) k = 0;
      }
      word |= I8 ? ((uint32_t)(int32_t)acc & 0xFFu) << (8 * e) : __float_as_uint((float)acc);
    }
    if (!I8 || valid == 0xFu) {
      out[u0 + q[h]] = word;
    } else {
#pragma unroll
      for (int32_t e = 0; e < EPU; ++e)
        if (valid >> e & 1u) reinterpret_cast<uint8_t*>(out_)[(u0 + q[h]) * EPU + e] = (uint8_t)(word >> (8 * e));
    }
  }
}

// ---- host derivation: integers only ----

int rm_derive(const ce_rm_desc* d, ce_rm_host_view* v, CeRateMatch* m) {
  memset(v, 0, sizeof(*v));
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  if (d->format != CE_RM_F32 && d->format != CE_RM_I8) return ce_fail(CE_ERR_INVALID, "format=%d is neither float32 (0) nor int8 (1)", d->format);
  if (d->format == CE_RM_F32 && !(d->filler_llr > 0.0f && d->filler_llr < INFINITY)) return ce_fail(CE_ERR_INVALID, "filler_llr=%g must be positive and finite", (double)d->filler_llr);
  if (const int rc = ce_ratematch_derive(d->base_graph, d->tbs, d->qm, d->n_layers, d->g_bits, d->n_ref, m); rc != CE_OK) return rc;
  ce_ratematch_view(*m, v);
  v->p = m->p;
  v->unit_elems = d->format == CE_RM_I8 ? 4 : 1;
  // a buffer starts up to unit_elems - 1 elements into its first unit
  v->tiles_per_block = (int32_t)(((m->n_cb + 2 * (v->unit_elems - 1)) / v->unit_elems + RM_TILE - 1) / RM_TILE);
  v->n_tiles = v->c * v->tiles_per_block;
  return CE_OK;
}

}  // namespace

struct ce_rm_plan {
  int device = 0;
  bool i8 = false;
  ce_rm_info info{};
  RmDev dev{};
};

extern "C" int ce_rm_derive_host(const ce_rm_desc* d, ce_rm_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  CeRateMatch m;
  return rm_derive(d, v, &m);
}

extern "C" int ce_rm_plan_create(const ce_rm_desc* d, ce_rm_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_rm_host_view v;
  CeRateMatch m;
  if (const int rc = rm_derive(d, &v, &m); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_rm_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->device = d->device;
  p->i8 = d->format == CE_RM_I8;
  p->info.n_code_blocks = v.c;
  p->info.n_cb = v.n_cb;
  p->info.elem_bytes = p->i8 ? 1 : 4;
  p->info.bytes_per_slot = ((int64_t)d->g_bits + (int64_t)v.c * v.n_cb) * p->info.elem_bytes;
  RmDev& D = p->dev;
  D.n_cb = (uint32_t)v.n_cb;
  D.c = (uint32_t)v.c;
  D.f1 = (uint32_t)v.f1;
  D.rm = ce_rm_walk_dev(m, d->qm, d->g_bits);
  D.inv_eq_lo = 1.0f / (float)D.rm.eq_lo;
  D.inv_eq_hi = 1.0f / (float)D.rm.eq_hi;
  D.tiles_per_block = (uint32_t)v.tiles_per_block;
  D.n_tiles = (uint32_t)v.n_tiles;
  D.filler = d->filler_llr;
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_rm_plan_destroy(ce_rm_plan* p) { delete p; }

extern "C" int ce_rm_plan_get_info(const ce_rm_plan* p, ce_rm_info* info) { return ce_get_info(p, info); }

extern "C" int ce_rm_recover(const ce_rm_plan* p, const void* llr, const int32_t* rv, int64_t rv_stride, int64_t n_slots, const void* harq_in,
                             void* out, void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  if (!llr || !rv || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  if (rv_stride < 0) return ce_fail(CE_ERR_INVALID, "negative strides are not supported");
  if ((reinterpret_cast<uintptr_t>(llr) | reinterpret_cast<uintptr_t>(harq_in) | reinterpret_cast<uintptr_t>(out)) & 15u)
    return ce_fail(CE_ERR_INVALID, "llr, harq_in and out must be 16-byte aligned");
  const int64_t n_wg = (n_slots + 7) / 8 * 8 * (int64_t)p->dev.n_tiles;
  if (n_wg > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "%lld slots of %u tiles: more than 2^31-1 workgroups in one launch", (long long)n_slots, p->dev.n_tiles);
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  const hipStream_t st = (hipStream_t)stream;
  if (p->i8)
    hipLaunchKernelGGL((ce_rm_kernel<true>), dim3((unsigned)n_wg), dim3(RM_NT), 0, st, p->dev, llr, rv, rv_stride, (uint32_t)n_slots, harq_in, out);
  else
    hipLaunchKernelGGL((ce_rm_kernel<false>), dim3((unsigned)n_wg), dim3(RM_NT), 0, st, p->dev, llr, rv, rv_stride, (uint32_t)n_slots, harq_in, out);
  return ce_launch_status("rate recovery");
}

// EXTENSION (no reference counterpart, see include/ce_ldpc.h): layered normalised min-sum decoding of quasi-cyclic LDPC
// code blocks behind rate recovery.  The base graph is plan data; nothing here depends on which graph it is.
//
// Kernel: a workgroup holds blocks_per_workgroup code blocks, zc threads each: thread z of a block owns the lifted checks
// (r, z) of every base row r.  A block's state lives in LDS from the load to the store:
//   L    int16 [n_cols zc]      the a-posteriori values (|L| <= CE_LDPC_L_BOUND)
//   S32  uint32 [n_rows zc]     per check: bit e = R_e negative | idx << 19 | ((3 min1) >> 2) << 24
//   S8   uint8 [n_rows zc]      per check: (3 min2) >> 2
// so R_e[z] of the previous iteration is rebuilt from 5 bytes instead of being kept per edge (include/ce_ldpc.h).
// The schedule (row starts, (col zc) << 16 | shift per edge) is read from the plan's buffer with uniform indices: scalar
// loads.  A row is: one S32 / S8 read, per edge one L read and one L write, one S32 / S8 write, one workgroup barrier.
// The row body is instantiated per row degree 2 .. 19 and selected by a uniform switch: the t_e stay in registers, nothing
// is indexed dynamically (no scratch), and a row's schedule words and its reads of L are issued together instead of one
// edge at a time behind a branch each (that form measured 1.26 - 1.58 x slower).  Within a row the zc checks touch disjoint variables (every
// edge is a permutation and the columns of a row are distinct), so the result does not depend on thread order.
// The stop decision is per block and never per lane: after an iteration every thread XORs the hard decisions of its
// checks, a thread with an unsatisfied check raises its block's LDS flag, and after a barrier every thread of the block
// reads the same flag.  A stopped block's threads skip the work and still reach every barrier; the workgroup leaves the
// iteration loop together, when no block raised `alive`.  DESIGN 6j.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <vector>

#include "ce_ldpc.h"
#include "ce_stage.h"

namespace {

constexpr int LDPC_WG_THREADS = 256;      // threads a workgroup of several blocks aims at
constexpr int LDPC_WG_LDS = 80896;        // LDS up to which a workgroup takes further blocks: two of them fit a CU

struct LdpcDev {
  uint32_t zc, n_rows, n_bits;     // n_bits = n_cols zc
  uint32_t n_in, punct, k_out;     // punct = n_punctured_cols zc
  uint32_t row_words;              // row_bytes / 4
  uint32_t bpw;                    // blocks per workgroup
  uint32_t max_iters, early_stop, f32;
  uint32_t off32, off8, blk_bytes; // per-block LDS: byte offsets of S32 and S8, and the block's size
  float scale;
};

__device__ __forceinline__ int ldpc_q_i8(int v) { return v < -127 ? -127 : v; }
__device__ __forceinline__ int ldpc_q_f32(float llr, float scale) {
  float v = llr * scale;
  v = (v != v) ? 0.0f : v;
  v = fminf(fmaxf(v, -127.0f), 127.0f);
  return (int)rintf(v);
}

// (col zc) << 16 | shift of an edge -> the variable of lifted check z
__device__ __forceinline__ uint32_t ldpc_var(uint32_t pk, uint32_t z, uint32_t zc) {
  uint32_t zz = z + (pk & 0xFFFFu);
  zz -= zz >= zc ? zc : 0u;
  return (pk >> 16) + zz;
}

// One lifted check of a base row of DEG edges (include/ce_ldpc.h).  DEG is a template parameter so that the DEG schedule
// words are loaded together, the DEG reads of L are in flight together and t[] stays in registers.
template <int DEG>
__device__ __forceinline__ void ldpc_row(int16_t* L, uint32_t* s32, uint8_t* s8, const uint32_t* __restrict__ edges, uint32_t z, uint32_t zc) {
  const uint32_t st = *s32, m2o = *s8;
  const uint32_t m1o = st >> CE_LDPC_STATE_MAG_SHIFT, idxo = (st >> CE_LDPC_STATE_IDX_SHIFT) & 31u;
  uint32_t a[DEG];
  int t[DEG];
#pragma unroll
  for (int e = 0; e < DEG; ++e) a[e] = ldpc_var(edges[e], z, zc);
#pragma unroll
  for (int e = 0; e < DEG; ++e) t[e] = (int)L[a[e]];
  int min1 = 0x7FFF, min2 = 0x7FFF;
  uint32_t idx = 0, neg = 0;
#pragma unroll
  for (int e = 0; e < DEG; ++e) {
    const int mo = (int)((uint32_t)e == idxo ? m2o : m1o);
    const int te = t[e] - (((st >> e) & 1u) ? -mo : mo);
    t[e] = te;
    const int ab = min(abs(te), 127);
    neg |= (te < 0 ? 1u : 0u) << e;
    if (ab < min1) {
      min2 = min1;
      min1 = ab;
      idx = (uint32_t)e;
    } else if (ab < min2) {
      min2 = ab;
    }
  }
  constexpr uint32_t mask = (1u << DEG) - 1u;
  const uint32_t rneg = (__popc(neg) & 1) ? (~neg & mask) : neg;   // bit e: sgn ^ s_e
  const int m1 = (3 * min1) >> 2, m2 = (3 * min2) >> 2;
#pragma unroll
  for (int e = 0; e < DEG; ++e) {
    const int m = (uint32_t)e == idx ? m2 : m1;
    L[a[e]] = (int16_t)(t[e] + (((rneg >> e) & 1u) ? -m : m));
  }
  *s32 = rneg | (idx << CE_LDPC_STATE_IDX_SHIFT) | ((uint32_t)m1 << CE_LDPC_STATE_MAG_SHIFT);
  *s8 = (uint8_t)m2;
}

// XOR of the hard decisions of one lifted check of a base row of DEG edges
template <int DEG>
__device__ __forceinline__ uint32_t ldpc_parity(const int16_t* L, const uint32_t* __restrict__ edges, uint32_t z, uint32_t zc) {
  uint32_t x = 0;
#pragma unroll
  for (int e = 0; e < DEG; ++e) x ^= (uint32_t)(uint16_t)L[ldpc_var(edges[e], z, zc)];
  return x >> 15;
}

// the row degree is uniform: one instance per degree 2 .. CE_LDPC_MAX_ROW_DEGREE
#define LDPC_DEGREES(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19)
__device__ __forceinline__ void ldpc_row_any(uint32_t deg, int16_t* L, uint32_t* s32, uint8_t* s8, const uint32_t* __restrict__ edges, uint32_t z,
                                             uint32_t zc) {
  switch (deg) {
#define X(D) case D: ldpc_row<D>(L, s32, s8, edges, z, zc); break;
    LDPC_DEGREES(X)
#undef X
    default: break;
  }
}
__device__ __forceinline__ uint32_t ldpc_parity_any(uint32_t deg, const int16_t* L, const uint32_t* __restrict__ edges, uint32_t z, uint32_t zc) {
  switch (deg) {
#define X(D) case D: return ldpc_parity<D>(L, edges, z, zc);
    LDPC_DEGREES(X)
#undef X
    default: return 0u;
  }
}
static_assert(CE_LDPC_MAX_ROW_DEGREE == 19, "LDPC_DEGREES lists the degrees 2 .. CE_LDPC_MAX_ROW_DEGREE");

__global__ __launch_bounds__(CE_LDPC_MAX_ZC) void ce_ldpc_kernel(LdpcDev P, const uint32_t* __restrict__ sched, const void* __restrict__ in,
                                                                 int64_t n_blocks, uint32_t* __restrict__ hard, int32_t* __restrict__ status,
                                                                 int16_t* __restrict__ post) {
  extern __shared__ uint4 ldpc_lds[];
  uint8_t* lds = reinterpret_cast<uint8_t*>(ldpc_lds);
  const uint32_t zc = P.zc;
  const uint32_t bl = threadIdx.x / zc, z = threadIdx.x - bl * zc;   // block of the workgroup, lifted check
  const int64_t blk = (int64_t)blockIdx.x * P.bpw + bl;
  const bool active = blk < n_blocks;                                 // the last workgroup may hold fewer blocks
  int16_t* L = reinterpret_cast<int16_t*>(lds + (size_t)bl * P.blk_bytes);
  uint32_t* S32 = reinterpret_cast<uint32_t*>(lds + (size_t)bl * P.blk_bytes + P.off32);
  uint8_t* S8 = lds + (size_t)bl * P.blk_bytes + P.off8;
  uint32_t* flags = reinterpret_cast<uint32_t*>(lds + (size_t)P.bpw * P.blk_bytes);   // [bpw] fail, then alive
  uint32_t* alive = flags + P.bpw;

  // ---- load: channel values into L, R = 0 ----
  if (active) {
    for (uint32_t i = z; i < P.n_bits; i += zc) {
      int ch = 0;
      if (i >= P.punct && i - P.punct < P.n_in) {
        const int64_t src = blk * (int64_t)P.n_in + (i - P.punct);
        ch = P.f32 ? ldpc_q_f32(reinterpret_cast<const float*>(in)[src], P.scale) : ldpc_q_i8(reinterpret_cast<const int8_t*>(in)[src]);
      }
      L[i] = (int16_t)ch;
    }
    for (uint32_t r = 0; r < P.n_rows; ++r) {
      S32[r * zc + z] = 0u;
      S8[r * zc + z] = 0;
    }
  }
  if (z == 0) flags[bl] = 0u;
  if (threadIdx.x == 0) *alive = 0u;
  __syncthreads();

  bool run = active;          // the same for every thread of a block
  uint32_t iters = 0, ok = 0;
  const uint32_t* edges = sched + P.n_rows + 1u;
  for (uint32_t it = 1;; ++it) {
    // ---- one iteration: the rows in order ----
    for (uint32_t r = 0; r < P.n_rows; ++r) {
      const uint32_t e0 = sched[r], deg = sched[r + 1u] - e0;   // uniform
      if (run) ldpc_row_any(deg, L, S32 + r * zc + z, S8 + r * zc + z, edges + e0, z, zc);
      __syncthreads();
    }
    const bool last = it == P.max_iters;
    if (!P.early_stop && !last) continue;   // uniform
    // ---- parity of the hard decisions over the plan's rows ----
    if (run) {
      uint32_t bad = 0;
      for (uint32_t r = 0; r < P.n_rows; ++r) {
        const uint32_t e0 = sched[r];
        bad |= ldpc_parity_any(sched[r + 1u] - e0, L, edges + e0, z, zc);
      }
      if (bad) flags[bl] = 1u;   // every writer stores the same value
    }
    __syncthreads();
    if (run) {
      const bool fail = flags[bl] != 0u;
      if (!fail || last) {
        run = false;
        iters = it;
        ok = fail ? 0u : 1u;
      } else {
        if (z == 0) *alive = 1u;
      }
    }
    __syncthreads();
    const bool go = *alive != 0u;   // uniform over the workgroup
    __syncthreads();
    if (z == 0) flags[bl] = 0u;     // read again only behind the next iteration's row barriers
    if (threadIdx.x == 0) *alive = 0u;
    if (!go) break;
  }

  // ---- store ----
  if (!active) return;
  if (z == 0) {
    status[2 * blk] = (int32_t)iters;
    status[2 * blk + 1] = (int32_t)ok;
  }
  uint32_t* hrow = hard + blk * (int64_t)P.row_words;
  for (uint32_t w = z; w < P.row_words; w += zc) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 32u; ++b) {
      const uint32_t i = 32u * w + b;
      if (i < P.k_out) v |= ((uint32_t)(uint16_t)L[i] >> 15) << ((b & ~7u) + (7u - (b & 7u)));   // byte b / 8 of the dword, MSB first
    }
    hrow[w] = v;
  }
  if (post) {
    int16_t* prow = post + blk * (int64_t)P.n_bits;
    for (uint32_t i = z; i < P.n_bits; i += zc) prow[i] = L[i];
  }
}

// ---- host derivation ----

int ldpc_derive(const ce_ldpc_desc* d, ce_ldpc_host_view* v, std::vector<uint32_t>* sched) {
  memset(v, 0, sizeof(*v));
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  if (d->zc < 2 || d->zc > CE_LDPC_MAX_ZC) return ce_fail(CE_ERR_INVALID, "zc=%d outside 2..%d", d->zc, CE_LDPC_MAX_ZC);
  if (d->n_rows < 1 || d->n_rows > CE_LDPC_MAX_ROWS) return ce_fail(CE_ERR_INVALID, "n_rows=%d outside 1..%d", d->n_rows, CE_LDPC_MAX_ROWS);
  if (d->n_cols <= d->n_rows || d->n_cols > CE_LDPC_MAX_COLS)
    return ce_fail(CE_ERR_INVALID, "n_cols=%d outside n_rows + 1 = %d..%d", d->n_cols, d->n_rows + 1, CE_LDPC_MAX_COLS);
  const int n_sys = d->n_cols - d->n_rows, n_bits = d->n_cols * d->zc;
  if (d->n_punctured_cols < 0 || d->n_punctured_cols > n_sys)
    return ce_fail(CE_ERR_INVALID, "n_punctured_cols=%d outside 0..n_sys = %d", d->n_punctured_cols, n_sys);
  if (d->n_in < 1 || d->n_in > n_bits - d->n_punctured_cols * d->zc)
    return ce_fail(CE_ERR_INVALID, "n_in=%d outside 1..(n_cols - n_punctured_cols) zc = %d", d->n_in, n_bits - d->n_punctured_cols * d->zc);
  if (d->k_out < 1 || d->k_out > n_sys * d->zc) return ce_fail(CE_ERR_INVALID, "k_out=%d outside 1..n_sys zc = %d", d->k_out, n_sys * d->zc);
  if (d->in_format != CE_LDPC_I8 && d->in_format != CE_LDPC_F32) return ce_fail(CE_ERR_INVALID, "in_format=%d: CE_LDPC_F32 or CE_LDPC_I8", d->in_format);
  if (d->in_format == CE_LDPC_F32 && !(d->llr_scale > 0.0f && d->llr_scale < INFINITY))
    return ce_fail(CE_ERR_INVALID, "llr_scale=%g must be positive and finite", (double)d->llr_scale);
  if (d->max_iters < 1 || d->max_iters > 255) return ce_fail(CE_ERR_INVALID, "max_iters=%d outside 1..255", d->max_iters);
  if (d->early_stop != 0 && d->early_stop != 1) return ce_fail(CE_ERR_INVALID, "early_stop=%d: 0 or 1", d->early_stop);
  if (!d->row_start || !d->col || !d->shift) return ce_fail(CE_ERR_INVALID, "row_start, col and shift must not be null");
  if (d->row_start[0] != 0) return ce_fail(CE_ERR_INVALID, "row_start[0]=%d must be 0", d->row_start[0]);
  int col_deg[CE_LDPC_MAX_COLS] = {0};
  int max_row = 0;
  for (int r = 0; r < d->n_rows; ++r) {
    const int64_t deg = (int64_t)d->row_start[r + 1] - d->row_start[r];
    if (deg < 2 || deg > CE_LDPC_MAX_ROW_DEGREE)
      return ce_fail(CE_ERR_INVALID, "row_start: row %d has %lld edges, outside 2..%d", r, (long long)deg, CE_LDPC_MAX_ROW_DEGREE);
    if ((int)deg > max_row) max_row = (int)deg;
    bool seen[CE_LDPC_MAX_COLS] = {false};
    for (int e = d->row_start[r]; e < d->row_start[r + 1]; ++e) {
      if (d->col[e] < 0 || d->col[e] >= d->n_cols) return ce_fail(CE_ERR_INVALID, "col[%d]=%d outside 0..n_cols - 1 = %d", e, d->col[e], d->n_cols - 1);
      if (seen[d->col[e]]) return ce_fail(CE_ERR_INVALID, "col[%d]=%d appears twice in row %d", e, d->col[e], r);
      seen[d->col[e]] = true;
      ++col_deg[d->col[e]];
      if (d->shift[e] < 0 || d->shift[e] >= d->zc) return ce_fail(CE_ERR_INVALID, "shift[%d]=%d outside 0..zc - 1 = %d", e, d->shift[e], d->zc - 1);
    }
  }
  const int n_edges = d->row_start[d->n_rows];
  v->n_sys = n_sys;
  v->n_edges = n_edges;
  v->max_row_degree = max_row;
  for (int c = 0; c < d->n_cols; ++c)
    if (col_deg[c] > v->max_col_degree) v->max_col_degree = col_deg[c];
  v->row_bytes = 16 * ((d->k_out + 127) / 128);
  v->n_bits = n_bits;
  v->threads_per_block = d->zc;
  v->lds_l_bytes = (2 * n_bits + 15) & ~15;
  v->lds_state32_bytes = (4 * d->n_rows * d->zc + 15) & ~15;
  v->lds_state8_bytes = (d->n_rows * d->zc + 15) & ~15;
  v->lds_bytes_per_block = v->lds_l_bytes + v->lds_state32_bytes + v->lds_state8_bytes;
  int bpw = LDPC_WG_THREADS / d->zc;
  if (bpw > LDPC_WG_LDS / v->lds_bytes_per_block) bpw = LDPC_WG_LDS / v->lds_bytes_per_block;
  if (bpw < 1) bpw = 1;
  v->blocks_per_workgroup = bpw;
  v->threads = bpw * d->zc;
  v->lds_flag_bytes = (4 * (bpw + 1) + 15) & ~15;
  v->lds_bytes = bpw * v->lds_bytes_per_block + v->lds_flag_bytes;
  v->schedule_bytes = 4 * (d->n_rows + 1 + n_edges);
  v->state_idx_shift = CE_LDPC_STATE_IDX_SHIFT;
  v->state_mag_shift = CE_LDPC_STATE_MAG_SHIFT;
  if (v->lds_bytes > CE_LDPC_LDS_MAX)
    return ce_fail(CE_ERR_UNSUPPORTED, "the plan needs %d bytes of LDS per workgroup, a CU has %d", v->lds_bytes, CE_LDPC_LDS_MAX);
  if (sched) {
    sched->resize((size_t)d->n_rows + 1 + n_edges);
    for (int r = 0; r <= d->n_rows; ++r) (*sched)[r] = (uint32_t)d->row_start[r];
    for (int e = 0; e < n_edges; ++e)   // col zc <= 67 * 384 < 2^16, shift < 2^9
      (*sched)[(size_t)d->n_rows + 1 + e] = ((uint32_t)(d->col[e] * d->zc) << 16) | (uint32_t)d->shift[e];
  }
  return CE_OK;
}

// The kernel's dynamic-LDS limit, raised once per device to what a CU has (plans above 64 KiB need it; the limit never
// falls, so plans of every size may be created in any order and from several host threads).
hipError_t ldpc_raise_lds_limit(int device) {
  static std::mutex mu;
  static bool raised[CE_MAX_DEVICES] = {false};
  if (device < 0 || device >= CE_MAX_DEVICES) return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(mu);
  if (raised[device]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ce_ldpc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CE_LDPC_LDS_MAX);
  if (e == hipSuccess) raised[device] = true;
  return e;
}

}  // namespace

struct ce_ldpc_plan {
  int device = 0;
  ce_ldpc_info info{};
  LdpcDev dev{};
  uint32_t* sched = nullptr;
};

extern "C" int ce_ldpc_derive_host(const ce_ldpc_desc* d, ce_ldpc_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  return ldpc_derive(d, v, nullptr);
}

extern "C" int ce_ldpc_plan_create(const ce_ldpc_desc* d, ce_ldpc_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_ldpc_host_view v;
  std::vector<uint32_t> sched;
  if (const int rc = ldpc_derive(d, &v, &sched); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_ldpc_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->device = d->device;
  p->info.n_edges = v.n_edges;
  p->info.row_bytes = v.row_bytes;
  p->info.n_bits = v.n_bits;
  p->info.blocks_per_workgroup = v.blocks_per_workgroup;
  p->info.threads = v.threads;
  p->info.lds_bytes = v.lds_bytes;
  LdpcDev& D = p->dev;
  D.zc = (uint32_t)d->zc;
  D.n_rows = (uint32_t)d->n_rows;
  D.n_bits = (uint32_t)v.n_bits;
  D.n_in = (uint32_t)d->n_in;
  D.punct = (uint32_t)(d->n_punctured_cols * d->zc);
  D.k_out = (uint32_t)d->k_out;
  D.row_words = (uint32_t)v.row_bytes / 4u;
  D.bpw = (uint32_t)v.blocks_per_workgroup;
  D.max_iters = (uint32_t)d->max_iters;
  D.early_stop = (uint32_t)d->early_stop;
  D.f32 = d->in_format == CE_LDPC_F32 ? 1u : 0u;
  D.off32 = (uint32_t)v.lds_l_bytes;
  D.off8 = (uint32_t)(v.lds_l_bytes + v.lds_state32_bytes);
  D.blk_bytes = (uint32_t)v.lds_bytes_per_block;
  D.scale = d->llr_scale;
  CeDeviceScope scope(d->device);
  hipError_t e = ce_upload(scope.err, &p->sched, sched.data(), sched.size() * sizeof(uint32_t));
  if (e == hipSuccess) e = ldpc_raise_lds_limit(d->device);
  if (e != hipSuccess) {
    ce_ldpc_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "LDPC decoder plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_ldpc_plan_destroy(ce_ldpc_plan* p) {
  if (!p) return;
  if (p->sched) (void)hipFree(p->sched);
  delete p;
}

extern "C" int ce_ldpc_plan_get_info(const ce_ldpc_plan* p, ce_ldpc_info* info) { return ce_get_info(p, info); }

extern "C" int ce_ldpc_decode(const ce_ldpc_plan* p, const void* in, int64_t n_blocks, uint8_t* hard, int32_t* status, int16_t* post,
                              void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_blocks < 0) return ce_fail(CE_ERR_INVALID, "n_blocks=%lld", (long long)n_blocks);
  if (n_blocks == 0) return CE_OK;
  if (!in || !hard || !status) return ce_fail(CE_ERR_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(hard) | reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(post)) & 15u)
    return ce_fail(CE_ERR_INVALID, "in, hard, status and post must be 16-byte aligned");
  const int64_t n_wg = (n_blocks + p->dev.bpw - 1) / p->dev.bpw;
  if (n_wg > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "%lld blocks: more than 2^31-1 workgroups in one launch", (long long)n_blocks);
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  hipLaunchKernelGGL(ce_ldpc_kernel, dim3((unsigned)n_wg), dim3((unsigned)p->info.threads), (size_t)p->info.lds_bytes, (hipStream_t)stream, p->dev,
                     p->sched, in, n_blocks, reinterpret_cast<uint32_t*>(hard), status, post);
  return ce_launch_status("LDPC decoding");
}

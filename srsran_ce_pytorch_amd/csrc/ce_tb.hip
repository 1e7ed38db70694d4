// EXTENSION (no reference counterpart, see include/ce_tb.h): CRC checks and transport-block assembly behind the LDPC
// decoder -- per code block the CRC24B residue and the block's share of the transport-block CRC, per slot the payloads
// spliced at bit granularity into the transport block, its CRC residue and the number of failed blocks.
//
// Kernel: one wave per code block, CE_TB_THREADS / 64 blocks per workgroup, over the flat index slot C + r, so 8 slots of
// 152 blocks fill the chip as 1216 slots of one block do.  The kernel is bound by vector-instruction issue, so
// its shape follows the instruction count per wave.
//  Pieces.  A row of `hard` is cut into 64 pieces of piece_dwords = ceil(in_row_bytes / 256) dwords, 1 .. 5, one per lane:
//   at K' = 8448 (264 dwords) a lane runs 20 bytes, not two 16-byte chunks of which the second exists for two lanes only.
//  CRC.  Registers hold a residue left-aligned in 32 bits (the x^(L-1) coefficient in bit 31), which makes the 16- and the
//   24-bit polynomial one code path without masks.  A lane runs its piece through both CRCs byte by byte from a table in
//   LDS: the bits of the piece below P for the transport-block polynomial, below K' for CRC24B.  The cut is made without a
//   branch -- the piece is shifted right as one number until the kept bits are its last, and zeros in front do not move a
//   zero register -- so the two chains are straight-line code side by side.  Each residue is then multiplied by
//   x^(bits that follow the piece) mod g -- a host-derived power from the plan's device buffer, an L-step shift-and-reduce
//   product, both chains in one loop.  The transport block's powers are kept per code block r and include x^((C-1-r) P),
//   so the product yields the lane's part of t_r directly.  The wave XORs the 64 lane values with __shfl_xor and lane 0
//   stores the pair.
//  Table.  256 entries per polynomial, read at the byte's value: one lookup per byte.  32 random indices on ds_read_b32's
//   32 banks ((a / 4) mod 32, per 32-lane half) put about 3.5 on the fullest bank.  -DCE_TB_NIBBLE builds the other form
//   for comparison: 16 entries per polynomial, each replicated 32 times, entry e of lane l at dword 32 e + (l mod 32), bank
//   l mod 32 -- no conflict whatever the data, but two lookups per byte.  Measured, the second lookup's instructions cost
//   more than the conflicts.
//  Transport block.  Dword j of a slot's row belongs to the block that holds stream bit 32 j.  The wave of block r writes
//   dwords ceil(r P / 32) .. ceil((r + 1) P / 32) - 1, lane by lane: two big-endian dwords of its own row funnel-shifted by
//   the bit offset, the bits past P replaced by the first dword of block r + 1 (P >= 32 whenever C > 1, so one neighbour
//   suffices), the bits from A on cleared.  The wave of block C - 1 goes on to the end of the row with zeros.  These loads
//   hit the lines the wave's own piece loads fetch.
//  Fold.  For C > 1 a second launch, one wave per slot, XORs cb_status[slot][.][1] and counts the nonzero
//   cb_status[slot][.][0]; for C = 1 the first kernel writes tb_status itself and there is no second launch.
// Every output byte has one writer; nothing is read back in the kernel that wrote it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ce_crc.h"
#include "ce_segment.h"
#include "ce_stage.h"
#include "ce_tb.h"

namespace {

constexpr int TB_NT = CE_TB_THREADS;
constexpr int TB_BPW = TB_NT / 64;   // code blocks (waves) per workgroup
constexpr int TB_MAXP = CE_TB_MAX_PIECE;
#ifdef CE_TB_NIBBLE
constexpr int TB_TAB = 16 * 32;      // dwords per polynomial
#else
constexpr int TB_TAB = 256;
#endif

struct TbDev {
  uint32_t c, kp, p, a;             // C, K', P, A
  uint32_t g_tb, g_cb;              // the polynomials, left-aligned
  uint32_t l_tb, sh_tb;             // L_tb and 32 - L_tb (CRC24B: 24 and 8)
  uint32_t piece, in_row_dwords;    // dwords per lane, dwords per row
  uint32_t tb_row_dwords;
};

__device__ __forceinline__ uint32_t tb_step_byte(uint32_t reg, uint32_t byte, const uint32_t* tab, uint32_t lane) {
#ifdef CE_TB_NIBBLE
  reg = (reg << 4) ^ tab[((((reg >> 28) ^ (byte >> 4)) & 15u) << 5) | (lane & 31u)];
  return (reg << 4) ^ tab[((((reg >> 28) ^ byte) & 15u) << 5) | (lane & 31u)];
#else
  (void)lane;
  return (reg << 8) ^ tab[((reg >> 24) ^ byte) & 255u];   // the one data-dependent address: masked to the table's size
#endif
}

// The first `nbits` (<= 32 PIECE, may be <= 0) bits of a piece as one number, o[0] the most significant dword: the piece
// shifted right until they are its last bits.  Zeros in front leave a zero register where it is, so the CRC of all bytes of
// the result, from zero, is the CRC of those bits alone -- no branch on the position of P or K' inside the piece.
template <int PIECE>
__device__ __forceinline__ void tb_keep_leading(const uint32_t (&w)[TB_MAXP], int32_t nbits, uint32_t (&o)[PIECE]) {
  const uint32_t s = 32u * PIECE - (uint32_t)min(max(nbits, 0), 32 * PIECE), q = s >> 5, t = s & 31u;
  uint32_t v[PIECE];   // shifted by whole dwords: v[i] = w[i - q], 0 in front
#pragma unroll
  for (int i = 0; i < PIECE; ++i) {
    v[i] = 0u;
#pragma unroll
    for (int k = 0; k <= i; ++k) v[i] = q == (uint32_t)(i - k) ? w[k] : v[i];
  }
#pragma unroll
  for (int i = 0; i < PIECE; ++i) {
    const uint32_t hi = i ? v[i - 1] : 0u;
    o[i] = t ? (hi << (32u - t)) | (v[i] >> t) : v[i];
  }
}

// The lane's part of the block's residues: its piece w (big-endian dwords) cut at P for the transport-block polynomial
// (times the power that also carries the block's x^((C-1-r) P)) and, with MULTI, at K' for CRC24B.
template <bool MULTI, int PIECE>
__device__ __forceinline__ void tb_residues(const TbDev& P, const uint32_t* __restrict__ pw, const uint32_t (*tab)[TB_TAB], uint32_t lane, uint32_t r,
                                            const uint32_t (&w)[TB_MAXP], uint32_t& part_tb, uint32_t& part_cb) {
  const int32_t first = (int32_t)(lane * 32u * PIECE);
  uint32_t o_tb[PIECE], o_cb[PIECE];
  tb_keep_leading<PIECE>(w, (int32_t)P.p - first, o_tb);
  if constexpr (MULTI) tb_keep_leading<PIECE>(w, (int32_t)P.kp - first, o_cb);
  uint32_t a_tb = 0u, a_cb = 0u;
#pragma unroll
  for (int b = 0; b < 4 * PIECE; ++b) {
    a_tb = tb_step_byte(a_tb, (o_tb[b >> 2] >> (24 - 8 * (b & 3))) & 255u, tab[0], lane);
    if constexpr (MULTI) a_cb = tb_step_byte(a_cb, (o_cb[b >> 2] >> (24 - 8 * (b & 3))) & 255u, tab[1], lane);
  }
  uint32_t b_tb = pw[(r + 1u) * 64u + lane], b_cb = MULTI ? pw[lane] : 0u;
  // C > 1 needs B > K_cb >= 3840, that is A > 3824: then both polynomials have 24 bits and the chains share the loop
  const uint32_t L = MULTI ? 24u : P.l_tb;
  uint32_t r_tb = 0u, r_cb = 0u;
  for (uint32_t i = 0; i < L; ++i) {
    r_tb = ce_crc_xtime(r_tb, P.g_tb) ^ ((uint32_t)((int32_t)b_tb >> 31) & a_tb);
    b_tb <<= 1;
    if constexpr (MULTI) {
      r_cb = ce_crc_xtime(r_cb, P.g_cb) ^ ((uint32_t)((int32_t)b_cb >> 31) & a_cb);
      b_cb <<= 1;
    }
  }
  part_tb = r_tb;
  part_cb = r_cb;
}

__global__ __launch_bounds__(TB_NT) void ce_tb_kernel(TbDev P, const uint32_t* __restrict__ pw, const uint8_t* __restrict__ hard, uint32_t n_blocks,
                                                      uint8_t* __restrict__ tb, int32_t* __restrict__ tb_status, int32_t* __restrict__ cb_status) {
  __shared__ uint32_t tab[2][TB_TAB];   // [0]: the transport-block polynomial, [1]: CRC24B
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t blk = blockIdx.x * TB_BPW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // slot C + r: wave-uniform
  const bool live = blk < n_blocks;
  const uint32_t* const roww = reinterpret_cast<const uint32_t*>(hard + (size_t)(live ? blk : 0u) * P.in_row_dwords * 4u);
  // the lane's piece is on its way while the tables are built
  uint32_t w[TB_MAXP];
#pragma unroll
  for (int i = 0; i < TB_MAXP; ++i) {
    const uint32_t dw = lane * P.piece + (uint32_t)i;
    w[i] = live && (uint32_t)i < P.piece && dw < P.in_row_dwords ? __builtin_bswap32(roww[dw]) : 0u;
  }

  for (uint32_t i = threadIdx.x; i < 2 * TB_TAB; i += TB_NT) {
    const uint32_t which = i / TB_TAB, e = i % TB_TAB, g = which ? P.g_cb : P.g_tb;
#ifdef CE_TB_NIBBLE
    uint32_t v = (e >> 5) << 28;
    for (int k = 0; k < 4; ++k) v = ce_crc_xtime(v, g);
#else
    uint32_t v = e << 24;
    for (int k = 0; k < 8; ++k) v = ce_crc_xtime(v, g);
#endif
    tab[which][e] = v;
  }
  __syncthreads();
  if (!live) return;
  const uint32_t slot = blk / P.c, r = blk - slot * P.c;
  const bool multi = P.c > 1;

  // ---- the dwords of the transport block this code block owns ----
  const uint32_t s0 = r * P.p;   // the block's first stream bit
  const uint32_t j0 = (s0 + 31u) >> 5;
  const uint32_t j1 = r + 1u == P.c ? P.tb_row_dwords : (s0 + P.p + 31u) >> 5;
  uint32_t* const out = reinterpret_cast<uint32_t*>(tb + (size_t)slot * P.tb_row_dwords * 4u);
  for (uint32_t j = j0 + lane; j < j1; j += 64) {
    const uint32_t sbit = j << 5;
    uint32_t val = 0;
    if (sbit < P.a) {                       // sbit < A < s0 + P: the dword starts inside this block's payload
      const uint32_t o = sbit - s0, dw = o >> 5, sh = o & 31u;
      const uint32_t hi = __builtin_bswap32(roww[dw]);
      const uint32_t lo = dw + 1u < P.in_row_dwords ? __builtin_bswap32(roww[dw + 1u]) : 0u;
      val = sh ? (hi << sh) | (lo >> (32u - sh)) : hi;
      const uint32_t nv = P.p - o;          // payload bits of this block from o on
      if (nv < 32u) {
        val &= ~(0xFFFFFFFFu >> nv);
        if (r + 1u < P.c) val |= __builtin_bswap32(roww[P.in_row_dwords]) >> nv;   // the next block's first payload bits
      }
      const uint32_t na = P.a - sbit;
      if (na < 32u) val &= ~(0xFFFFFFFFu >> na);
    }
    out[j] = __builtin_bswap32(val);
  }

  // ---- the two residues of the block ----
  uint32_t part_tb = 0u, part_cb = 0u;
#define TB_CASE(PC)                                                                      \
  case PC:                                                                               \
    if (multi) tb_residues<true, PC>(P, pw, tab, lane, r, w, part_tb, part_cb);          \
    else tb_residues<false, PC>(P, pw, tab, lane, r, w, part_tb, part_cb);               \
    break;
  switch (P.piece) {   // wave-uniform
    TB_CASE(1) TB_CASE(2) TB_CASE(3) TB_CASE(4) TB_CASE(5)
  }
#undef TB_CASE
  const uint32_t t_r = ce_crc_wave_xor(part_tb) >> P.sh_tb;
  const uint32_t res = multi ? ce_crc_wave_xor(part_cb) >> 8 : t_r;
  if (lane == 0) {
    reinterpret_cast<int2*>(cb_status)[blk] = make_int2((int)res, (int)t_r);
    if (!multi) reinterpret_cast<int2*>(tb_status)[slot] = make_int2((int)res, res != 0u ? 1 : 0);
  }
}

// C > 1: tb_status[slot] = {XOR of t_r, number of failed blocks}, one wave per slot
__global__ __launch_bounds__(TB_NT) void ce_tb_fold_kernel(uint32_t c, uint32_t n_slots, const int32_t* __restrict__ cb_status, int32_t* __restrict__ tb_status) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t slot = blockIdx.x * TB_BPW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (slot >= n_slots) return;
  const int2* const cb = reinterpret_cast<const int2*>(cb_status) + (size_t)slot * c;
  uint32_t x = 0, bad = 0;
  for (uint32_t r = lane; r < c; r += 64) {
    const int2 v = cb[r];
    x ^= (uint32_t)v.y;
    bad += v.x != 0 ? 1u : 0u;
  }
  x = ce_crc_wave_xor(x);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bad += (uint32_t)__shfl_xor((int)bad, off);
  if (lane == 0) reinterpret_cast<int2*>(tb_status)[slot] = make_int2((int)x, (int)bad);
}

// ---- host derivation: integers only ----

int tb_derive(const ce_tb_desc* d, ce_tb_host_view* v) {
  memset(v, 0, sizeof(*v));
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  if (d->base_graph != 1 && d->base_graph != 2) return ce_fail(CE_ERR_INVALID, "base_graph=%d is neither 1 nor 2", d->base_graph);
  if (d->tbs < 1) return ce_fail(CE_ERR_INVALID, "tbs=%d must be positive", d->tbs);
  CeSegment seg;
  if (const int rc = ce_segment_derive(d->base_graph, d->tbs, &seg); rc != CE_OK) return rc;
  const CeCrcSelect crc = ce_crc_select(d->tbs, seg.c, seg.k_prime);
  v->b = (int32_t)seg.b;
  v->k_cb = (int32_t)seg.k_cb;
  v->c = (int32_t)seg.c;
  v->b_prime = (int32_t)seg.b_prime;
  v->k_prime = (int32_t)seg.k_prime;
  v->l_tb = crc.l_tb, v->l_cb = crc.l_cb, v->p = crc.p, v->g_tb = crc.g_tb, v->g_cb = crc.g_cb;
  v->in_row_bytes = 16 * ((v->k_prime + 127) / 128);
  v->tb_row_bytes = crc.tb_row_bytes;
  v->piece_dwords = (v->in_row_bytes + 255) / 256;   // K' <= K_b 384 <= 8448: at most CE_TB_MAX_PIECE
  v->threads = TB_NT;
  v->blocks_per_workgroup = TB_BPW;
  v->lds_bytes = 2 * TB_TAB * 4;
  v->fold_slots_per_workgroup = seg.c > 1 ? TB_BPW : 0;
  v->power_bytes = 4 * 64 * (v->c + 1);
  return CE_OK;
}

// dst[l], l < 64: base x^(bits of the first n that follow piece l of W bits) -- x^(n mod W + W (f - 1 - l)) for the
// f = floor(n / W) whole pieces, 1 for the partial piece (and whatever lies behind it, whose residue is 0)
void tb_lane_powers(uint32_t* dst, uint32_t base, uint32_t one, uint32_t g, uint32_t L, uint32_t n, uint32_t W) {
  const uint32_t f = n / W, xw = ce_crc_pow_x(one, g, W);
  for (uint32_t l = f; l < 64; ++l) dst[l] = base;
  uint32_t t = ce_crc_mulmod(base, ce_crc_pow_x(one, g, n % W), g, L);
  for (uint32_t l = f; l-- > 0;) {
    dst[l] = t;
    t = ce_crc_mulmod(t, xw, g, L);
  }
}

}  // namespace

struct ce_tb_plan {
  int device = 0;
  ce_tb_info info{};
  TbDev dev{};
  // [64] per lane x^(bits of K' behind the lane's piece) mod g24B, then per code block r [64] the same for P mod g_tb
  // times x^((C-1-r) P)
  uint32_t* pw = nullptr;
};

extern "C" int ce_tb_derive_host(const ce_tb_desc* d, ce_tb_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  return tb_derive(d, v);
}

extern "C" int ce_tb_plan_create(const ce_tb_desc* d, ce_tb_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_tb_host_view v;
  if (const int rc = tb_derive(d, &v); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_tb_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->device = d->device;
  p->info.n_code_blocks = v.c;
  p->info.in_row_bytes = v.in_row_bytes;
  p->info.tb_row_bytes = v.tb_row_bytes;
  p->info.bytes_per_slot = (int64_t)v.c * v.in_row_bytes + v.tb_row_bytes + 8 * (int64_t)v.c + 8;
  TbDev& D = p->dev;
  D.c = (uint32_t)v.c;
  D.kp = (uint32_t)v.k_prime;
  D.p = (uint32_t)v.p;
  D.a = (uint32_t)d->tbs;
  D.l_tb = (uint32_t)v.l_tb;
  D.sh_tb = 32u - D.l_tb;
  D.g_tb = (uint32_t)v.g_tb << D.sh_tb;
  D.g_cb = (uint32_t)v.g_cb << 8;
  D.piece = (uint32_t)v.piece_dwords;
  D.in_row_dwords = (uint32_t)v.in_row_bytes / 4u;
  D.tb_row_dwords = (uint32_t)v.tb_row_bytes / 4u;
  const uint32_t one_tb = 1u << D.sh_tb, one_cb = 1u << 8, W = 32u * D.piece;
  std::vector<uint32_t> pw((size_t)v.power_bytes / 4);
  tb_lane_powers(pw.data(), one_cb, one_cb, D.g_cb, 24u, D.kp, W);
  const uint32_t xp = ce_crc_pow_x(one_tb, D.g_tb, D.p);
  uint32_t base = one_tb;   // x^((C-1-r) P)
  for (int64_t r = (int64_t)D.c - 1; r >= 0; --r) {
    tb_lane_powers(pw.data() + 64 * (r + 1), base, one_tb, D.g_tb, D.l_tb, D.p, W);
    base = ce_crc_mulmod(base, xp, D.g_tb, D.l_tb);
  }
  CeDeviceScope scope(d->device);
  const hipError_t e = ce_upload(scope.err, &p->pw, pw.data(), pw.size() * sizeof(uint32_t));
  if (e != hipSuccess) {
    ce_tb_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "transport-block plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_tb_plan_destroy(ce_tb_plan* p) {
  if (!p) return;
  if (p->pw) (void)hipFree(p->pw);
  delete p;
}

extern "C" int ce_tb_plan_get_info(const ce_tb_plan* p, ce_tb_info* info) { return ce_get_info(p, info); }

extern "C" int ce_tb_assemble(const ce_tb_plan* p, const uint8_t* hard, int64_t n_slots, uint8_t* tb, int32_t* tb_status, int32_t* cb_status,
                              void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  if (!hard || !tb || !tb_status || !cb_status) return ce_fail(CE_ERR_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(hard) | reinterpret_cast<uintptr_t>(tb) | reinterpret_cast<uintptr_t>(tb_status) | reinterpret_cast<uintptr_t>(cb_status)) & 15u)
    return ce_fail(CE_ERR_INVALID, "hard, tb, tb_status and cb_status must be 16-byte aligned");
  const int64_t n_blocks = n_slots * (int64_t)p->dev.c;
  if (n_blocks > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "%lld slots of %u code blocks: more than 2^31-1 code blocks in one launch", (long long)n_slots, p->dev.c);
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ce_tb_kernel, dim3((unsigned)((n_blocks + TB_BPW - 1) / TB_BPW)), dim3(TB_NT), 0, st, p->dev, p->pw, hard, (uint32_t)n_blocks, tb, tb_status,
                     cb_status);
  if (const int rc = ce_launch_status("transport-block assembly"); rc != CE_OK || p->dev.c == 1) return rc;
#ifdef CE_TB_NO_FOLD   // diagnostic builds only (tools/tb_perf.py): the first launch alone, tb_status is left unwritten
  return CE_OK;
#endif
  hipLaunchKernelGGL(ce_tb_fold_kernel, dim3((unsigned)((n_slots + TB_BPW - 1) / TB_BPW)), dim3(TB_NT), 0, st, p->dev.c, (uint32_t)n_slots, cb_status, tb_status);
  return ce_launch_status("transport-block fold");
}

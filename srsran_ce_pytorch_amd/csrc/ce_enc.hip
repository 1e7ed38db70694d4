// EXTENSION (no reference counterpart, see include/ce_enc.h): the PUSCH transport-block encoder -- transport-block CRC,
// segmentation with CRC24B and fillers, LDPC encoding under the caller's graph, bit selection and interleaving into the
// slot's bit row g.  The forward counterpart of ce_rm, ce_ldpc and ce_tb.
//
// Encode kernel: one 256-thread workgroup per (slot, code block), the codeword never leaves LDS before it is complete.
//  Bit strings.  Every bit string in LDS is a row of dwords holding bit b in bit 31 - (b mod 32) of dword b / 32, so a
//   global row (MSB first in bytes) is the same dwords byte-swapped, and 32 bits from any bit position are two dwords and
//   one funnel shift (enc_get32).
//  CRC.  Registers hold a residue left-aligned in 32 bits (ce_crc.h).  A string is cut into chunks of
//   CE_ENC_CRC_CHUNK dwords; thread t runs dwords 4 t .. 4 t + 3 of every chunk through the CRC (one 16-byte load; four
//   table lookups per dword from four 256-entry tables in LDS, the lookups of a dword independent of one another) and
//   carries its residue from chunk to chunk by x^(32 (CHUNK - 4)).  The 256 residues are advanced by x^(128 (255 - t)),
//   XORed (shuffles, then four values through LDS), and the zeros that pad the string to whole chunks are taken back by
//   x^-(their number) -- x is invertible modulo a polynomial with a constant term.  All powers are host-derived.  The
//   transport block's CRC (up to 39 chunks, 160 KB) is computed by the workgroup of the slot's LAST block only: its parity
//   lands there, because P >= 24 whenever C > 1.  CRC24B is one chunk, from LDS.
//  Payload.  Thread j builds dword j of the block's K bits: two dwords of the tb row funnel-shifted by the bit offset r P,
//   cut at A and at P, the parity ORed in; zeros (the fillers) behind.
//  Columns.  Column c of Zc bits is kept as its periodic image of 2 Zc + 32 bits at a dword-aligned row of ext_dwords: the
//   rotation x[(z + s) mod Zc] of 32 consecutive z is then enc_get32 at bit 32 w + s, exact for every Zc from 2 to 384.
//   Only the columns the rows read need the image: the systematic ones and the four core parity columns.
//  Core.  lambda_i (four rows x ceil(Zc / 32) dwords, one thread each), then four host-derived steps, one per core parity
//   column: XOR of lambdas and of solved columns at a shift, optionally rotated as a whole (the NR core's first column),
//   then the image of the result.  Both accepted core forms are the same four-step program with other constants.
//  Extension rows.  One thread per (row, dword): XOR of <= 18 enc_get32.  The rows are independent of one another; rows
//   whose column lies beyond 2 Zc + N_cb are computed only when the codeword is asked for.
//  Codeword.  The columns are packed at Zc-bit granularity into one flat string, which is stored byte-swapped to `cw`
//   where that is given.
//  Gather.  One thread builds a whole dword of g: per bit the closed form of ce_rm.h (interleaver row and column, k mod P
//   where bits repeat, rank + s, unrank round the fillers) over the words of ce_ratematch.h, which rate recovery walks
//   too, and one LDS read.  Where two blocks meet inside a dword of g no
//   workgroup holds all its bits: the gather is then a second launch over g's dwords that reads the codewords from `cw`
//   (ce_enc.h).
// DESIGN 6l.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ce_crc.h"
#include "ce_enc.h"
#include "ce_ratematch.h"
#include "ce_stage.h"

namespace {

constexpr int ENC_NT = CE_ENC_THREADS;
constexpr int ENC_MAX_EDGES = CE_LDPC_MAX_ROWS * CE_LDPC_MAX_ROW_DEGREE;
constexpr int ENC_STEP_DW = 8;                                                     // dwords of a core step
constexpr int ENC_GRAPH_DW = (CE_LDPC_MAX_ROWS + 1 + ENC_MAX_EDGES + 4 * ENC_STEP_DW + 3) / 4 * 4;  // row_start | edges | steps, whole 16-byte pieces
constexpr int ENC_MAX_W = (CE_LDPC_MAX_ZC + 31) / 32;                              // 12
constexpr int ENC_MAX_WE = (2 * CE_LDPC_MAX_ZC + 32 + 31) / 32 + 1;                // 26
constexpr int ENC_FLAT_DW = (CE_LDPC_MAX_ZC * 22 / 32 + 2 + 3) / 4 * 4;                // K <= 8448 bits and a dword to spare, in whole 16-byte pieces
constexpr int ENC_CW_DW = CE_LDPC_MAX_COLS * CE_LDPC_MAX_ZC / 32 + 4;              // 26112 bits
constexpr uint32_t ENC_CHUNK = CE_ENC_CRC_CHUNK;
static_assert(ENC_CHUNK == 4 * ENC_NT, "a chunk is four dwords per thread");

struct EncDev {
  uint32_t c, a, p;                     // C, A, payload P
  uint32_t l_tb, g_tb, g_cb;            // L_tb; the polynomials, left-aligned
  uint32_t nc_tb, xc_tb, finv_tb;       // chunks of the transport block; x^(32 (CHUNK - 4)) and x^-(padding) mod g_tb
  uint32_t finv_cb;                     // x^-(32 CHUNK - P) mod g24B
  uint32_t tb_row_dwords, g_row_dwords, cw_row_dwords;
  uint32_t zc, n_sys, n_rows, w, we, kd;   // kd: dwords of the K information bits and one to spare, a multiple of 4
  uint32_t graph_dw;                    // dwords of the plan's table the kernel copies to LDS
  RmWalkDev rm;                         // bit selection and interleaving (ce_ratematch.h); rm.p is P, not the payload above
  uint32_t rep;                         // some E_r > P: bits repeat
  float inv_prm;                        // float32(1 / P)
  uint32_t two_zc;
};

// bits [pos, pos + 32) of a bit string; reads dwords pos / 32 and pos / 32 + 1
__device__ __forceinline__ uint32_t enc_get32(const uint32_t* p, uint32_t pos) {
  const uint32_t d = pos >> 5, sh = pos & 31u;
  return (uint32_t)(((((uint64_t)p[d]) << 32) | p[d + 1]) >> (32u - sh));
}

// the n <= 32 leading bits of a dword
__device__ __forceinline__ uint32_t enc_keep(uint32_t v, uint32_t n) { return n >= 32u ? v : v & ~(0xFFFFFFFFu >> n); }

// bits [i0, i0 + 32) of the periodic continuation of the zc-bit string that starts at bit `off` of p
__device__ __forceinline__ uint32_t enc_periodic32(const uint32_t* p, uint32_t off, uint32_t zc, uint32_t i0) {
  const uint32_t m = i0 % zc;
  if (zc >= 32u) {   // wave-uniform: at most one wrap inside 32 bits
    const uint32_t a = enc_get32(p, off + m), n1 = zc - m;
    return n1 >= 32u ? a : enc_keep(a, n1) | (enc_get32(p, off) >> n1);
  }
  uint64_t x = (uint64_t)enc_keep(enc_get32(p, off), zc) << 32;
  for (uint32_t w = zc; w < 64u; w <<= 1) x |= x >> w;   // periodic over all 64 bits
  return (uint32_t)((x << m) >> 32);
}

__device__ __forceinline__ uint32_t enc_crc_dword(uint32_t v, const uint32_t (*T)[256]) {
  // v(x) x^L mod g: the one data-dependent address, masked to the table's size
  return T[3][v >> 24] ^ T[2][(v >> 16) & 255u] ^ T[1][(v >> 8) & 255u] ^ T[0][v & 255u];
}

// CRC of a bit string given as n_chunks chunks of zero-padded dwords; fetch(q) returns dwords 4 q .. 4 q + 3.  Every thread
// of the workgroup calls it and gets the residue, left-aligned.  `red` is four dwords of LDS of this call's own.
template <class Fetch>
__device__ __forceinline__ uint32_t enc_crc(const uint32_t (*T)[256], uint32_t g, uint32_t L, uint32_t n_chunks, uint32_t xc, uint32_t pw, uint32_t finv,
                                            uint32_t* red, Fetch fetch) {
  uint32_t acc = 0u;
#pragma unroll 4
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint4 d = fetch(c * (uint32_t)ENC_NT + threadIdx.x);
    if (c) acc = ce_crc_mulmod(acc, xc, g, L);
    acc = enc_crc_dword(acc ^ d.x, T);
    acc = enc_crc_dword(acc ^ d.y, T);
    acc = enc_crc_dword(acc ^ d.z, T);
    acc = enc_crc_dword(acc ^ d.w, T);
  }
  acc = ce_crc_wave_xor(ce_crc_mulmod(acc, pw, g, L));
  if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ce_crc_mulmod(red[0] ^ red[1] ^ red[2] ^ red[3], finv, g, L);
}

// One dword of g: bits 32 d .. 32 d + 31 of the slot's row, zeros from G on.  word(r, i) is dword i of block r's codeword.
template <class Word>
__device__ __forceinline__ uint32_t enc_gather_dword(const EncDev& P, uint32_t d, uint32_t s, Word word) {
  const uint32_t f = d << 5;
  if (f >= P.rm.g) return 0u;
  uint32_t r, fl;   // the first bit's block and its index in the block's E_r bits
  if (f < P.rm.base_hi) {
    r = f / P.rm.e_lo;
    fl = f - r * P.rm.e_lo;
  } else {
    r = (f - P.rm.base_hi) / P.rm.e_hi;
    fl = f - P.rm.base_hi - r * P.rm.e_hi;
    r += P.rm.n_lo;
  }
  uint32_t e_r = r < P.rm.n_lo ? P.rm.e_lo : P.rm.e_hi, eq = r < P.rm.n_lo ? P.rm.eq_lo : P.rm.eq_hi;
  uint32_t j = fl / P.rm.qm, i = fl - j * P.rm.qm;   // f_{i + j Qm} = e_{i E/Qm + j}
  const uint32_t nb = min(32u, P.rm.g - f);
  uint32_t val = 0u;
  for (uint32_t b = 0; b < nb; ++b) {
    uint32_t k = i * eq + j, q;
    if (P.rep) ce_divmod(k, P.rm.p, P.inv_prm, q, k);   // repetition wraps round the buffer
    uint32_t rho = s + k;
    if (rho >= P.rm.p) rho -= P.rm.p;
    const uint32_t pos = (rho < P.rm.f0 ? rho : rho + P.rm.nf) + P.two_zc;
    val |= ((word(r, pos >> 5) >> (31u - (pos & 31u))) & 1u) << (31u - b);
    if (++i == P.rm.qm) {
      i = 0u;
      ++j;
    }
    if (++fl == e_r) {   // the next block's bits follow (5.5)
      ++r;
      fl = i = j = 0u;
      e_r = r < P.rm.n_lo ? P.rm.e_lo : P.rm.e_hi;
      eq = r < P.rm.n_lo ? P.rm.eq_lo : P.rm.eq_hi;
    }
  }
  return val;
}

__global__ __launch_bounds__(ENC_NT) void ce_enc_kernel(EncDev P, const uint32_t* __restrict__ tab, const uint8_t* __restrict__ tb, const int32_t* __restrict__ rv,
                                                        int64_t rv_stride, uint32_t rows_used, uint32_t gather, uint8_t* __restrict__ g, uint8_t* __restrict__ cw) {
  __shared__ uint32_t s_crc[2][4][256];          // [0]: the transport-block polynomial, [1]: CRC24B; [k]: e(x) x^(L + 8 k)
  __shared__ uint32_t s_graph[ENC_GRAPH_DW];
  __shared__ uint32_t s_flat[ENC_FLAT_DW];       // the K information bits
  __shared__ uint32_t s_cols[CE_LDPC_MAX_COLS * ENC_MAX_WE];
  __shared__ uint32_t s_cw[ENC_CW_DW];           // the codeword, packed
  __shared__ uint32_t s_lam[4][ENC_MAX_W];
  __shared__ uint32_t s_tmp[ENC_MAX_W + 4];
  __shared__ uint32_t s_red[2][4];
  const uint32_t t = threadIdx.x;
  const uint32_t slot = blockIdx.x / P.c, r = blockIdx.x - slot * P.c;   // scalar
  const uint32_t zc = P.zc, W = P.w, WE = P.we;

  // ---- CRC tables, the graph ----
  for (uint32_t which = 0; which < 2; ++which) {
    const uint32_t gp = which ? P.g_cb : P.g_tb;
    uint32_t v = t << 24;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      for (int q = 0; q < 8; ++q) v = ce_crc_xtime(v, gp);
      s_crc[which][k][t] = v;
    }
  }
  for (uint32_t i = t; i < P.graph_dw; i += ENC_NT) s_graph[i] = tab[i];
  __syncthreads();
  const uint32_t* const rs = s_graph;
  const uint32_t* const edges = s_graph + P.n_rows + 1;
  const uint32_t* const steps = tab + (P.graph_dw - 4 * ENC_STEP_DW);   // wave-uniform: scalar loads
  const uint32_t* const pw = tab + P.graph_dw;                        // [2][256]: x^(128 (255 - t)) mod g_tb, mod g24B

  // ---- 5.1: the transport block's CRC, in the workgroup of the last block ----
  const uint32_t* const tbrow = reinterpret_cast<const uint32_t*>(tb) + (size_t)slot * P.tb_row_dwords;
  uint32_t crc_tb = 0u;
  if (r + 1u == P.c) {
    crc_tb = enc_crc(s_crc[0], P.g_tb, P.l_tb, P.nc_tb, P.xc_tb, pw[t], P.finv_tb, s_red[0], [&](uint32_t q) -> uint4 {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      const uint32_t bit0 = q << 7;
      if (bit0 < P.a) {   // A <= 32 tb_row_dwords and the row is whole 16-byte pieces
        v = reinterpret_cast<const uint4*>(tbrow)[q];
        const uint32_t n = P.a - bit0;   // bits of the piece below A
        v.x = enc_keep(__builtin_bswap32(v.x), n);
        v.y = n > 32u ? enc_keep(__builtin_bswap32(v.y), n - 32u) : 0u;
        v.z = n > 64u ? enc_keep(__builtin_bswap32(v.z), n - 64u) : 0u;
        v.w = n > 96u ? enc_keep(__builtin_bswap32(v.w), n - 96u) : 0u;
      }
      return v;
    });
  }

  // ---- 5.2.2: the block's payload, funnel-shifted out of the tb row; parity; fillers ----
  for (uint32_t j = t; j < P.kd; j += ENC_NT) {
    uint32_t val = 0u;
    const uint32_t b0 = j << 5;   // the dword's first bit in the block
    if (b0 < P.p) {
      const uint32_t sp = r * P.p + b0;   // ... in the stream s
      if (sp < P.a) {
        const uint32_t dw = sp >> 5, sh = sp & 31u;
        const uint32_t hi = __builtin_bswap32(tbrow[dw]);
        const uint32_t lo = dw + 1u < P.tb_row_dwords ? __builtin_bswap32(tbrow[dw + 1u]) : 0u;
        val = enc_keep((uint32_t)(((((uint64_t)hi) << 32) | lo) >> (32u - sh)), P.a - sp);
      }
      val = enc_keep(val, P.p - b0);
      if (r + 1u == P.c) {   // the parity occupies bits [P - L_tb, P) of the last block
        const int32_t q = (int32_t)(P.p - P.l_tb) - (int32_t)b0;
        if (q >= 0 && q < 32) val |= crc_tb >> q;
        if (q < 0 && q > -32) val |= crc_tb << -q;
      }
    }
    s_flat[j] = val;
  }
  __syncthreads();
  if (P.c > 1u) {   // CRC24B of the P payload bits, appended
    const uint32_t crc_cb = enc_crc(s_crc[1], P.g_cb, 24u, 1u, 0u, pw[256 + t], P.finv_cb, s_red[1], [&](uint32_t q) -> uint4 {
      const uint32_t d = q << 2;
      return d < P.kd ? make_uint4(s_flat[d], s_flat[d + 1], s_flat[d + 2], s_flat[d + 3]) : make_uint4(0u, 0u, 0u, 0u);
    });
    if (t == 0u) {   // K >= K' = P + 24: both dwords exist
      const uint32_t d = P.p >> 5, sh = P.p & 31u;
      s_flat[d] |= crc_cb >> sh;
      if (sh > 8u) s_flat[d + 1] |= crc_cb << (32u - sh);
    }
    __syncthreads();
  }

  // ---- the periodic images of the systematic columns ----
  for (uint32_t it = t; it < P.n_sys * WE; it += ENC_NT) {
    const uint32_t c = it / WE, e = it - c * WE;
    s_cols[it] = enc_periodic32(s_flat, c * zc, zc, e << 5);
  }
  __syncthreads();

  // XOR of a row's listed edges at dword w
  const auto row_xor = [&](uint32_t row, uint32_t w) -> uint32_t {
    uint32_t acc = 0u;
    for (uint32_t e = rs[row]; e < rs[row + 1]; ++e) {
      const uint32_t ed = edges[e];
      acc ^= enc_get32(s_cols + (ed & 255u) * WE, (w << 5) + (ed >> 8));
    }
    return acc;
  };

  // ---- 5.3.2, the core: lambda_i, then four steps ----
  if (t < 4u * W) {
    const uint32_t i = t / W, w = t - i * W;
    s_lam[i][w] = row_xor(i, w);
  }
  __syncthreads();
  for (uint32_t st = 0; st < 4u; ++st) {
    const uint32_t* const S = steps + st * ENC_STEP_DW;   // {target, lambda mask, n_terms, rot, term[3]}
    const uint32_t target = S[0], mask = S[1], n_terms = S[2], rot = S[3];
    if (t < W) {
      uint32_t v = 0u;
      for (uint32_t i = 0; i < 4u; ++i)
        if (mask >> i & 1u) v ^= s_lam[i][t];
      for (uint32_t k = 0; k < n_terms; ++k) v ^= enc_get32(s_cols + (P.n_sys + (S[4 + k] & 255u)) * WE, (t << 5) + (S[4 + k] >> 8));
      s_tmp[t] = v;
    }
    __syncthreads();
    if (rot) {   // the whole column rotated: p[y] = v[(y + rot) mod Zc]
      const uint32_t v = t < W ? enc_periodic32(s_tmp, 0u, zc, (t << 5) + rot) : 0u;
      __syncthreads();
      if (t < W) s_tmp[t] = v;
      __syncthreads();
    }
    if (t < WE) s_cols[(P.n_sys + target) * WE + t] = enc_periodic32(s_tmp, 0u, zc, t << 5);
    __syncthreads();
  }

  // ---- the extension rows: independent of one another ----
  for (uint32_t it = t; it < (rows_used - 4u) * W; it += ENC_NT) {
    const uint32_t row = it / W, w = it - row * W;
    s_cols[(P.n_sys + 4u + row) * WE + w] = row_xor(4u + row, w);
  }
  __syncthreads();

  // ---- the codeword, packed at Zc-bit granularity ----
  const uint32_t cols_used = P.n_sys + rows_used;
  for (uint32_t d = t; d < P.cw_row_dwords; d += ENC_NT) {
    uint32_t val = 0u, filled = 0u;
    uint32_t col = (d << 5) / zc, z = (d << 5) - col * zc;
    while (filled < 32u && col < cols_used) {
      const uint32_t take = min(32u - filled, zc - z);
      val |= enc_keep(enc_get32(s_cols + col * WE, z), take) >> filled;
      filled += take;
      ++col;
      z = 0u;
    }
    s_cw[d] = val;
    if (cw) reinterpret_cast<uint32_t*>(cw)[(size_t)blockIdx.x * P.cw_row_dwords + d] = __builtin_bswap32(val);
  }
  if (!gather) return;   // two blocks meet inside a dword of g: ce_enc_gather_kernel reads cw
  __syncthreads();

  // ---- 5.4.2.1, 5.4.2.2, 5.5: the block's dwords of g ----
  const uint32_t base = r < P.rm.n_lo ? r * P.rm.e_lo : P.rm.base_hi + (r - P.rm.n_lo) * P.rm.e_hi, e_r = r < P.rm.n_lo ? P.rm.e_lo : P.rm.e_hi;
  const uint32_t d1 = r + 1u == P.c ? P.g_row_dwords : (base + e_r) >> 5;
  const uint32_t s = ce_rm_walk_start(P, (uint32_t)rv[(int64_t)slot * rv_stride]);
  uint32_t* const grow = reinterpret_cast<uint32_t*>(g) + (size_t)slot * P.g_row_dwords;
  for (uint32_t d = (base >> 5) + t; d < d1; d += ENC_NT)
    grow[d] = __builtin_bswap32(enc_gather_dword(P, d, s, [&](uint32_t, uint32_t i) { return s_cw[i]; }));
}

// g from the stored codewords: one thread per dword of g, whichever blocks its bits belong to
__global__ __launch_bounds__(ENC_NT) void ce_enc_gather_kernel(EncDev P, const uint8_t* __restrict__ cw, const int32_t* __restrict__ rv, int64_t rv_stride,
                                                               uint32_t tiles_per_slot, uint8_t* __restrict__ g) {
  const uint32_t slot = blockIdx.x / tiles_per_slot, tile = blockIdx.x - slot * tiles_per_slot;
  const uint32_t d = tile * ENC_NT + threadIdx.x;
  if (d >= P.g_row_dwords) return;
  const uint32_t s = ce_rm_walk_start(P, (uint32_t)rv[(int64_t)slot * rv_stride]);
  const uint32_t* const cws = reinterpret_cast<const uint32_t*>(cw) + (size_t)slot * P.c * P.cw_row_dwords;
  reinterpret_cast<uint32_t*>(g)[(size_t)slot * P.g_row_dwords + d] =
      __builtin_bswap32(enc_gather_dword(P, d, s, [&](uint32_t r, uint32_t i) { return __builtin_bswap32(cws[r * P.cw_row_dwords + i]); }));
}

// ---- host derivation: integers only ----

struct EncGraph {                  // what plan creation takes besides the view
  std::vector<uint32_t> table;     // the kernel's part of the graph: row_start | edges (col | shift << 8) | steps
  CeRateMatch rm;
};

int enc_derive(const ce_enc_desc* d, ce_enc_host_view* v, EncGraph* out) {
  EncGraph local;
  if (!out) out = &local;
  memset(v, 0, sizeof(*v));
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  if (const int rc = ce_ratematch_derive(d->base_graph, d->tbs, d->qm, d->n_layers, d->g_bits, d->n_ref, &out->rm); rc != CE_OK) return rc;
  ce_ratematch_view(out->rm, v);
  v->p_rm = out->rm.p;
  const CeCrcSelect crc = ce_crc_select(d->tbs, v->c, v->k_prime);
  v->l_tb = crc.l_tb, v->l_cb = crc.l_cb, v->p = crc.p, v->g_tb = crc.g_tb, v->g_cb = crc.g_cb;
  v->tb_row_bytes = crc.tb_row_bytes;
  v->g_row_bytes = 16 * ((d->g_bits + 127) / 128);

  // ---- the graph ----
  const int32_t zc = v->zc, n_rows = d->n_rows, n_cols = d->n_cols, n_sys = n_cols - n_rows;
  const int32_t want_sys = d->base_graph == 1 ? 22 : 10, max_cols = d->base_graph == 1 ? 68 : 52;
  if (!d->row_start || !d->col || !d->shift) return ce_fail(CE_ERR_INVALID, "null graph arrays");
  if (n_rows < 4 || n_rows > CE_LDPC_MAX_ROWS) return ce_fail(CE_ERR_INVALID, "n_rows=%d outside 4..%d", n_rows, CE_LDPC_MAX_ROWS);
  if (n_sys != want_sys || n_cols > max_cols)
    return ce_fail(CE_ERR_INVALID, "base graph %d has n_sys = %d and at most %d columns; the graph given has n_sys = %d and %d columns", d->base_graph, want_sys,
                   max_cols, n_sys, n_cols);
  if ((int64_t)(n_cols - 2) * zc < v->n_cb)
    return ce_fail(CE_ERR_INVALID, "a graph of %d columns is too short for the circular buffer: (n_cols - 2) Zc = %d < N_cb = %d", n_cols, (n_cols - 2) * zc, v->n_cb);
  if (d->row_start[0] != 0) return ce_fail(CE_ERR_INVALID, "row_start[0]=%d must be 0", d->row_start[0]);
  for (int32_t r = 0; r < n_rows; ++r) {
    const int32_t deg = d->row_start[r + 1] - d->row_start[r];
    if (deg < 1 || deg > CE_LDPC_MAX_ROW_DEGREE) return ce_fail(CE_ERR_INVALID, "row %d has %d edges: 1..%d are supported", r, deg, CE_LDPC_MAX_ROW_DEGREE);
    for (int32_t e = d->row_start[r]; e < d->row_start[r + 1]; ++e) {
      if (d->col[e] < 0 || d->col[e] >= n_cols) return ce_fail(CE_ERR_INVALID, "row %d: column %d outside 0..%d", r, d->col[e], n_cols - 1);
      if (d->shift[e] < 0 || d->shift[e] >= zc) return ce_fail(CE_ERR_INVALID, "row %d, column %d: shift %d outside 0..%d", r, d->col[e], d->shift[e], zc - 1);
    }
  }
  v->n_sys = n_sys;
  v->n_edges = d->row_start[n_rows];
  // core_at[i][j]: shift of column n_sys + j in core row i, -1 where absent
  int32_t core_at[4][4];
  for (auto& row : core_at)
    for (auto& x : row) x = -1;
  for (int32_t r = 0; r < n_rows; ++r) {
    int own = 0;
    for (int32_t e = d->row_start[r]; e < d->row_start[r + 1]; ++e) {
      const int32_t c = d->col[e], sh = d->shift[e];
      if (r < 4) {
        if (c >= n_sys + 4) return ce_fail(CE_ERR_INVALID, "row %d: column %d lies beyond the core columns (< n_sys + 4 = %d)", r, c, n_sys + 4);
        if (c >= n_sys) {
          if (core_at[r][c - n_sys] >= 0) return ce_fail(CE_ERR_INVALID, "row %d holds core column %d more than once", r, c);
          core_at[r][c - n_sys] = sh;
        }
      } else if (c == n_sys + r) {
        if (sh != 0 || ++own > 1) return ce_fail(CE_ERR_INVALID, "row %d: its own parity column %d must appear exactly once, at shift 0", r, c);
      } else if (c >= n_sys + 4) {
        return ce_fail(CE_ERR_INVALID, "row %d: column %d is neither below n_sys + 4 = %d nor the row's own column %d", r, c, n_sys + 4, n_sys + r);
      }
    }
    if (r >= 4 && own != 1) return ce_fail(CE_ERR_INVALID, "row %d: its own parity column %d must appear exactly once, at shift 0", r, n_sys + r);
  }
  bool triangular = true;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) triangular = triangular && (j == i ? core_at[i][j] == 0 : j < i || core_at[i][j] < 0);
  uint32_t steps[4][ENC_STEP_DW] = {};
  if (triangular) {
    v->core_form = CE_ENC_CORE_TRIANGULAR;
    for (uint32_t i = 0; i < 4; ++i) {
      steps[i][0] = i;
      steps[i][1] = 1u << i;
      for (uint32_t j = 0; j < i; ++j)
        if (core_at[i][j] >= 0) steps[i][4 + steps[i][2]++] = j | (uint32_t)core_at[i][j] << 8;
    }
  } else {
    for (int j = 1; j < 4; ++j)
      for (int i = 0; i < 4; ++i) {
        const bool want = i == j - 1 || i == j;
        if (want ? core_at[i][j] != 0 : core_at[i][j] >= 0)
          return ce_fail(CE_ERR_INVALID, "the core is neither triangular nor an NR core: column %d must appear in exactly rows %d and %d, both at shift 0 (row %d breaks it)",
                         n_sys + j, j - 1, j, i);
      }
    int rows = 0, n = 0, sh[3] = {0, 0, 0};
    for (int i = 0; i < 4; ++i)
      if (core_at[i][0] >= 0) {
        rows |= 1 << i;
        if (n < 3) sh[n] = core_at[i][0];
        ++n;
      }
    if (n != 3) return ce_fail(CE_ERR_INVALID, "the core is neither triangular nor an NR core: column %d appears in %d of the four core rows, not in three", n_sys, n);
    if (sh[0] != sh[1] && sh[0] != sh[2] && sh[1] != sh[2])
      return ce_fail(CE_ERR_INVALID, "the core is neither triangular nor an NR core: column %d has three different shifts %d, %d, %d: two must be equal", n_sys, sh[0],
                     sh[1], sh[2]);
    v->core_form = CE_ENC_CORE_NR;
    v->core_rows = rows;
    v->core_shift = sh[0] == sh[1] ? sh[2] : sh[0] == sh[2] ? sh[1] : sh[0];   // the equal pair cancels
    steps[0][0] = 0;
    steps[0][1] = 15u;
    steps[0][3] = (uint32_t)((zc - v->core_shift) % zc);
    for (uint32_t j = 1; j < 4; ++j) {   // row j - 1 gives column n_sys + j
      steps[j][0] = j;
      steps[j][1] = 1u << (j - 1);
      if (j >= 2) steps[j][4 + steps[j][2]++] = j - 1;
      if (core_at[j - 1][0] >= 0) steps[j][4 + steps[j][2]++] = 0u | (uint32_t)core_at[j - 1][0] << 8;
    }
  }
  const int32_t cols_needed = (2 * zc + v->n_cb + zc - 1) / zc;
  v->rows_needed = cols_needed - n_sys < 4 ? 4 : cols_needed - n_sys > n_rows ? n_rows : cols_needed - n_sys;
  v->col_dwords = (zc + 31) / 32;
  v->ext_dwords = (2 * zc + 32 + 31) / 32 + 1;
  v->cw_row_bytes = 16 * ((n_cols * zc + 127) / 128);
  // two blocks meet inside a dword of g where a prefix sum of the E_r is no multiple of 32
  for (int32_t r = 1; r < v->c; ++r) {
    const int64_t base = r <= v->n_lo ? (int64_t)r * v->e_lo : (int64_t)v->n_lo * v->e_lo + (int64_t)(r - v->n_lo) * v->e_hi;
    if (base % 32) v->cw_required = 1;
  }
  v->threads = ENC_NT;
  v->lds_bytes = 4 * (2 * 4 * 256 + ENC_GRAPH_DW + ENC_FLAT_DW + CE_LDPC_MAX_COLS * ENC_MAX_WE + ENC_CW_DW + 4 * ENC_MAX_W + ENC_MAX_W + 4 + 8);
  {   // the kernel's edge lists: a core row keeps its systematic edges, an extension row all but its own column
    std::vector<uint32_t>& T = out->table;
    T.assign((size_t)n_rows + 1, 0u);
    for (int32_t r = 0; r < n_rows; ++r) {
      for (int32_t e = d->row_start[r]; e < d->row_start[r + 1]; ++e)
        if (r < 4 ? d->col[e] < n_sys : d->col[e] != n_sys + r) T.push_back((uint32_t)d->col[e] | (uint32_t)d->shift[e] << 8);
      T[r + 1] = (uint32_t)(T.size() - (size_t)(n_rows + 1));
    }
    for (auto& st : steps) T.insert(T.end(), st, st + ENC_STEP_DW);
  }
  v->table_bytes = 4 * ((int32_t)out->table.size() + 2 * 256);
  return CE_OK;
}

// x^-e mod g: x h(x) = 1 for h = (g + 1) / x, g taken with its leading term
uint32_t enc_pow_x_inv(uint32_t g, uint32_t L, int64_t e) {
  const uint32_t one = 1u << (32u - L), h = 0x80000000u | (((g >> (32u - L)) >> 1) << (32u - L));   // left-aligned: x^(L-1) + (g_low >> 1)
  uint32_t r = one;
  for (int64_t i = 0; i < e; ++i) r = ce_crc_mulmod(r, h, g, L);
  return r;
}

}  // namespace

struct ce_enc_plan {
  int device = 0;
  ce_enc_info info{};
  EncDev dev{};
  uint32_t rows_needed = 0, n_rows = 0;
  uint32_t* table = nullptr;   // row_start | edges | steps | powers
};

extern "C" int ce_enc_derive_host(const ce_enc_desc* d, ce_enc_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  return enc_derive(d, v, nullptr);
}

extern "C" int ce_enc_plan_create(const ce_enc_desc* d, ce_enc_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_enc_host_view v;
  EncGraph graph;
  if (const int rc = enc_derive(d, &v, &graph); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_enc_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->device = d->device;
  p->info.n_code_blocks = v.c;
  p->info.tb_row_bytes = v.tb_row_bytes;
  p->info.g_row_bytes = v.g_row_bytes;
  p->info.cw_row_bytes = v.cw_row_bytes;
  p->info.cw_required = v.cw_required;
  p->info.bytes_per_slot = (int64_t)v.tb_row_bytes + v.g_row_bytes;
  p->rows_needed = (uint32_t)v.rows_needed;
  p->n_rows = (uint32_t)d->n_rows;
  EncDev& D = p->dev;
  D.c = (uint32_t)v.c, D.a = (uint32_t)d->tbs, D.p = (uint32_t)v.p;
  D.l_tb = (uint32_t)v.l_tb;
  D.g_tb = (uint32_t)v.g_tb << (32u - D.l_tb);
  D.g_cb = (uint32_t)v.g_cb << 8;
  const uint32_t one_tb = 1u << (32u - D.l_tb), one_cb = 1u << 8;
  const int64_t chunk_bits = 32 * (int64_t)ENC_CHUNK;
  D.nc_tb = (uint32_t)((d->tbs + chunk_bits - 1) / chunk_bits);
  D.xc_tb = ce_crc_pow_x(one_tb, D.g_tb, 32 * (int64_t)(ENC_CHUNK - 4));
  D.finv_tb = enc_pow_x_inv(D.g_tb, D.l_tb, D.nc_tb * chunk_bits - d->tbs);
  D.finv_cb = enc_pow_x_inv(D.g_cb, 24u, chunk_bits - v.p);
  if (ce_crc_mulmod(ce_crc_pow_x(one_tb, D.g_tb, 1), enc_pow_x_inv(D.g_tb, D.l_tb, 1), D.g_tb, D.l_tb) != one_tb ||
      ce_crc_mulmod(ce_crc_pow_x(one_cb, D.g_cb, 1), enc_pow_x_inv(D.g_cb, 24u, 1), D.g_cb, 24u) != one_cb)
    return ce_fail(CE_ERR_INVALID, "internal: x has no inverse modulo the CRC polynomial");
  D.tb_row_dwords = (uint32_t)v.tb_row_bytes / 4u, D.g_row_dwords = (uint32_t)v.g_row_bytes / 4u, D.cw_row_dwords = (uint32_t)v.cw_row_bytes / 4u;
  D.zc = (uint32_t)v.zc, D.n_sys = (uint32_t)v.n_sys, D.n_rows = (uint32_t)d->n_rows, D.w = (uint32_t)v.col_dwords, D.we = (uint32_t)v.ext_dwords;
  D.kd = ((uint32_t)v.k / 32u + 2u + 3u) / 4u * 4u;
  D.graph_dw = (uint32_t)graph.table.size();
  D.rm = ce_rm_walk_dev(graph.rm, d->qm, d->g_bits);
  D.rep = D.rm.e_hi > D.rm.p ? 1u : 0u;
  D.inv_prm = 1.0f / (float)D.rm.p;
  D.two_zc = 2u * D.zc;
  // powers: x^(128 (255 - t)) for both polynomials
  std::vector<uint32_t>& T = graph.table;
  T.resize(D.graph_dw + 512);
  const uint32_t gs[2] = {D.g_tb, D.g_cb}, Ls[2] = {D.l_tb, 24u}, ones[2] = {one_tb, one_cb};
  for (int w = 0; w < 2; ++w) {
    const uint32_t x128 = ce_crc_pow_x(ones[w], gs[w], 128);
    uint32_t cur = ones[w];
    for (int t = 255; t >= 0; --t) {
      T[D.graph_dw + 256 * w + t] = cur;
      cur = ce_crc_mulmod(cur, x128, gs[w], Ls[w]);
    }
  }
  CeDeviceScope scope(d->device);
  const hipError_t e = ce_upload(scope.err, &p->table, T.data(), T.size() * sizeof(uint32_t));
  if (e != hipSuccess) {
    ce_enc_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "encoder plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_enc_plan_destroy(ce_enc_plan* p) {
  if (!p) return;
  if (p->table) (void)hipFree(p->table);
  delete p;
}

extern "C" int ce_enc_plan_get_info(const ce_enc_plan* p, ce_enc_info* info) { return ce_get_info(p, info); }

extern "C" int ce_enc_encode(const ce_enc_plan* p, const uint8_t* tb, const int32_t* rv, int64_t rv_stride, int64_t n_slots, uint8_t* g, uint8_t* cw,
                             void* stream) {
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_slots == 0) return CE_OK;
  if (!tb || !rv || !g) return ce_fail(CE_ERR_INVALID, "null argument");
  if (rv_stride < 0) return ce_fail(CE_ERR_INVALID, "negative strides are not supported");
  if ((reinterpret_cast<uintptr_t>(tb) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(cw)) & 15u)
    return ce_fail(CE_ERR_INVALID, "tb, g and cw must be 16-byte aligned");
  if (p->info.cw_required && !cw) return ce_fail(CE_ERR_INVALID, "code blocks meet inside a dword of g (cw_required): cw must be given");
  const EncDev& D = p->dev;
  const int64_t n_blocks = n_slots * (int64_t)D.c, tiles = (D.g_row_dwords + ENC_NT - 1) / ENC_NT;
  if (n_blocks > 0x7FFFFFFFll || n_slots * tiles > 0x7FFFFFFFll)
    return ce_fail(CE_ERR_UNSUPPORTED, "%lld slots of %u code blocks: more than 2^31-1 workgroups in one launch", (long long)n_slots, D.c);
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t rows_used = cw ? p->n_rows : p->rows_needed, gather = p->info.cw_required ? 0u : 1u;
  hipLaunchKernelGGL(ce_enc_kernel, dim3((unsigned)n_blocks), dim3(ENC_NT), 0, st, D, p->table, tb, rv, rv_stride, rows_used, gather, g, cw);
  if (const int rc = ce_launch_status("transport-block encoder"); rc != CE_OK || gather) return rc;
  hipLaunchKernelGGL(ce_enc_gather_kernel, dim3((unsigned)(n_slots * tiles)), dim3(ENC_NT), 0, st, D, cw, rv, rv_stride, (uint32_t)tiles, g);
  return ce_launch_status("encoder bit selection");
}

// EXTENSION (no reference counterpart, see include/ce_tp.h): sounding reference signal (SRS) channel estimation over the
// frequency-domain grid rows of TS 38.211 6.4.1.4 -- per (item, receive port) the power delay profile of the sounding ports
// (launch 1, ce_srs_profile) and, with a delay taken out, the per-port channel per 4-PRB block, its wideband mean, the noise
// from the residual and the received energy (launch 2, ce_srs_estimate).
//
// Operator (include/ce_tp.h has it in full): port i sits on comb comb_i with cyclic shift cs_i, rho_i[n] = exp(+j 2 pi cs_i n /
// n_cs_max); element n of symbol s lies on subcarrier k(s, c, n) = 12 start_prb[s] + c + k_tc n; rbar(n) is the low-PAPR base
// sequence of the symbol's (u, v).
//     launch 1   G_i[n] = y[k(s, comb_i, n)] conj(rbar(n)) conj(rho_i[n]),  z[d] = (1 / M) sum_n G_i[n] exp(+j 2 pi n d / N),
//                profile[d'] = sum_s sum_i |z_{s,i}[(d' - g) mod N]|^2, d' < win_len
//     launch 2   g_c[n] = y[k(s, c, n)] conj(rbar(n)) W_N[(n delay) mod N];  h_sb = (1 / Q) sum over the block of g conj(rho_i);
//                e_c[n] = g_c[n] - sum_{i on c} h_sb rho_i[n];  noise = sum |e|^2 / dof;  epre = mean |y|^2;  h_wb = mean h_sb
//
// Both kernels: one 256-thread workgroup per (item, receive port).  The hopping words of the <= 4 symbols are folded from the
// table that is linear in c_init = n_id (SRS's rule for group AND sequence hopping) as ce_dmrs_lp_kernel folds them; (u, v)
// select q[u][v]; rbar(n) = W_{N_ZC}[(q tri[n]) mod N_ZC] is an element-granular gather, so W_{N_ZC} (<= 13 KiB) is staged
// in LDS.  y is read with 8-byte loads, lane n on element n of the comb.
//   profile  the row frame of ce_fft.h with a row being a TERM (s, i): rows_per_workgroup terms at a time, row q taking the
//            terms q, q + rows_per_workgroup, ..; the product into the first buffer, zero beyond M; the passes (the inverse
//            transform natively) with scale float32(1 / M); each thread adds re^2 + im^2 of its outputs into registers; the
//            rows are folded in ascending row order and the window is written.  All LDS is dynamic: the buffers (16 - 64 KiB
//            by N) and behind them the staged W_{N_ZC} where both fit 64 KiB (every N <= 2048; at N = 4096 the gather reads
//            the table from memory instead).
//   estimate per (s, comb) the g_c row goes to LDS (M <= 1632: 13 KiB); barrier; one thread per (port, block) sums its Q
//            elements in ascending n; barrier; one thread per n forms |e|^2 from the residual (never from an energy
//            difference); the sums are reduced by a butterfly per wave and the four waves as (w0 + w1) + (w2 + w3).
// 64-bit addressing; no atomics, no scratch; slot, n_id and delay enter reduced (mod slots_per_frame, mod 30 and bits, mod N):
// they cannot address memory.  DESIGN 6u.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "ce_dmrs.h"
#include "ce_fft.h"
#include "ce_gold.h"
#include "ce_stage.h"
#include "ce_tp.h"

namespace {

constexpr int SRS_MAX_AP = 4, SRS_MAX_SYMB = 4, SRS_MAX_M = 1632, SRS_MAX_BLOCKS = 68, SRS_MAX_RX = 64, SRS_MAX_CS = 12;
constexpr int SRS_MAX_PER_THREAD = 16;   // N / threads_per_row: 2 (N = 128), 4 (256, 512), 8 (1024, 2048), 16 (4096)
constexpr int SRS_MAX_PRB_GRID = 341;
constexpr int SRS_INFO_LEN = 10;
constexpr uint32_t SRS_A = 0x3f3504f3u;  // float32 0.70710677
constexpr int SRS_HW_WORDS = SRS_MAX_SYMB * 32 + SRS_MAX_SYMB;   // the hopping fold's LDS words

struct SrsDev {
  FftDev f;                 // m = N, n_rows = 1, wg_per_item = 1; an item is an (item, receive port)
  uint32_t k_tc, n_ap, n_symb, l0;
  uint32_t m, q_len, n_blocks, n_cs_max, n_combs;   // M, Q
  uint32_t combs[2];                    // the used combs in the order of their first port
  uint32_t port_slot[SRS_MAX_AP];       // per port: index into combs
  uint32_t port_comb[SRS_MAX_AP];
  uint32_t start_re[SRS_MAX_SYMB];      // 12 start_prb[s]
  uint32_t form, n_zc, n_zc_magic, n_w; // CE_DMRS_LP_FORM_*; N_ZC; floor(2^32 / N_ZC); entries of the gather table
  uint32_t hopping, v_live, n_symb_slot, slots_per_frame, nw;
  uint32_t win_len, guard;
  float scale_m;            // float32(1 / M)
  float inv_q, inv_wb, inv_dof, inv_re;   // float32 of 1 / Q, 1 / (n_symb n_blocks), 1 / dof, 1 / (n_symb n_combs M)
};

struct SrsTables {
  const float2* wtab;       // [n_w]
  const float2* rho;        // [n_ap][n_cs_max]
  const uint16_t* qtab;     // [60]
  const uint16_t* tri;      // [M]
  const uint8_t* code;      // [30][M] (table form)
  const uint32_t* hop;      // [32][nw]
};

__device__ __forceinline__ uint32_t srs_mod(uint32_t x, uint32_t n, uint32_t n_magic) {   // as lp_mod of ce_dmrs_lp.hip
  const uint32_t r = x - __umulhi(x, n_magic) * n;
  return r >= n ? r - n : r;
}

// a conj(b)
__device__ __forceinline__ float2 srs_cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }

__device__ __forceinline__ uint32_t srs_pick(const uint32_t (&q)[SRS_MAX_SYMB], uint32_t s) {
  return s == 0u ? q[0] : s == 1u ? q[1] : s == 2u ? q[2] : q[3];
}

// The symbols' q (table form: u) into registers.  `hw`: SRS_HW_WORDS words of LDS nobody else uses until this returns (it
// ends with a barrier).  Every thread of the workgroup calls it.
__device__ __forceinline__ void srs_hop(const SrsDev& P, const SrsTables& T, uint32_t u_slot, uint32_t u_id, uint32_t* hw,
                                        uint32_t (&qs)[SRS_MAX_SYMB]) {
  const uint32_t tid = threadIdx.x;
  if (P.hopping != CE_DMRS_LP_HOP_NEITHER) {
    const bool group = P.hopping == CE_DMRS_LP_HOP_GROUP;
    const uint32_t c_init = u_id & 0x7FFFFFFFu;   // SRS: c_init = n_id in both modes
    for (uint32_t j = tid; j < P.n_symb * 32u; j += TP_NT) {
      const uint32_t col = j >> 5, i = j & 31u;
      const uint32_t p = P.n_symb_slot * u_slot + P.l0 + col;   // < n_symb_slot * slots_per_frame
      const uint32_t wi = group ? p >> 2 : p >> 5;              // < nw
      hw[j] = i == 0u ? T.hop[wi] : (((c_init >> (i - 1u)) & 1u) ? T.hop[i * P.nw + wi] : 0u);
    }
  }
  __syncthreads();
  if (tid < P.n_symb) {
    uint32_t f_gh = 0, v = 0;
    if (P.hopping != CE_DMRS_LP_HOP_NEITHER) {
      uint32_t x = 0;
      for (uint32_t i = 0; i < 32; ++i) x ^= hw[tid * 32u + i];
      const uint32_t p = P.n_symb_slot * u_slot + P.l0 + tid;
      if (P.hopping == CE_DMRS_LP_HOP_GROUP)
        f_gh = ((x >> (8u * (p & 3u))) & 0xFFu) % 30u;
      else
        v = P.v_live ? (x >> (p & 31u)) & 1u : 0u;
    }
    const uint32_t u = (f_gh + u_id % 30u) % 30u;
    hw[SRS_MAX_SYMB * 32 + tid] = P.form == CE_DMRS_LP_FORM_PHI ? u : T.qtab[2u * u + v];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SRS_MAX_SYMB; ++k) qs[k] = (uint32_t)k < P.n_symb ? hw[SRS_MAX_SYMB * 32 + k] : 0u;
  __syncthreads();
}

// rbar(n) of a symbol whose q (table form: u) is `q`, gathered from `w`.
__device__ __forceinline__ float2 srs_base(const SrsDev& P, const SrsTables& T, const float2* w, uint32_t q, uint32_t n) {
  if (P.form == CE_DMRS_LP_FORM_PHI) return w[T.code[q * P.m + n] & 3u];
  return w[srs_mod(q * (uint32_t)T.tri[n], P.n_zc, P.n_zc_magic)];   // q <= N_ZC, tri < N_ZC: the product is below 2^22
}

template <bool STAGE_W>
__global__ __launch_bounds__(TP_NT) void ce_srs_profile_kernel(SrsDev P, SrsTables T, const float2* __restrict__ tw, const float2* __restrict__ y,
                                                               int64_t st_b, int64_t st_r, int64_t st_sym, uint32_t n_rx,
                                                               const int32_t* __restrict__ slot, const int32_t* __restrict__ n_id, int64_t st_slot,
                                                               int64_t st_id, float* __restrict__ profile) {
  extern __shared__ float4 srs_lds[];
  const uint32_t N = P.f.m, M = P.m, mask = N - 1u;
  const uint32_t tpr = 1u << P.f.tpr_log2, rpw = P.f.rpw;
  const uint32_t rl = threadIdx.x >> P.f.tpr_log2, lane = threadIdx.x & (tpr - 1u);   // rl: row of the workgroup (wave-uniform)
  const uint32_t b = blockIdx.x / n_rx, r = blockIdx.x - b * n_rx;
  float2* buf0 = reinterpret_cast<float2*>(srs_lds) + (size_t)rl * 2u * N;
  float2* buf1 = buf0 + N;
  float2* w_lds = reinterpret_cast<float2*>(srs_lds) + (size_t)rpw * 2u * N;   // behind the buffers (STAGE_W)
  const uint32_t u_slot = (uint32_t)slot[(int64_t)b * st_slot] % P.slots_per_frame, u_id = (uint32_t)n_id[(int64_t)b * st_id];
  uint32_t qs[SRS_MAX_SYMB];
  srs_hop(P, T, u_slot, u_id, reinterpret_cast<uint32_t*>(srs_lds), qs);   // over the buffers, which nobody has written yet
  if (STAGE_W)
    for (uint32_t i = threadIdx.x; i < P.n_w; i += TP_NT) w_lds[i] = T.wtab[i];
  __syncthreads();
  const float2* w = STAGE_W ? w_lds : T.wtab;
  const float2* y_item = y + ((int64_t)b * st_b + (int64_t)r * st_r);
  const uint32_t n_terms = P.n_symb * P.n_ap;
  const uint32_t per_thread = N >> P.f.tpr_log2;

  float acc[SRS_MAX_PER_THREAD];
#pragma unroll
  for (int j = 0; j < SRS_MAX_PER_THREAD; ++j) acc[j] = 0.0f;

  for (uint32_t t0 = 0; t0 < n_terms; t0 += rpw) {   // uniform over the workgroup
    const uint32_t term = t0 + rl;
    const bool active = term < n_terms;
    const uint32_t s = active ? term / P.n_ap : 0u, i = active ? term - s * P.n_ap : 0u;
    {
      const float2* row = y_item + ((int64_t)(P.l0 + s) * st_sym + (int64_t)(P.start_re[s] + P.port_comb[i]));
      const float2* rho = T.rho + i * P.n_cs_max;
      const uint32_t q = srs_pick(qs, s);
      for (uint32_t n = lane; n < N; n += tpr) {
        float2 z = make_float2(0.0f, 0.0f);
        if (active && n < M) z = srs_cmulc(srs_cmulc(row[(size_t)P.k_tc * n], srs_base(P, T, w, q, n)), rho[n % P.n_cs_max]);
        buf0[n] = z;
      }
    }
    __syncthreads();

    const float2* res = tp_passes(P.f, buf0, buf1, tw, lane, tpr, P.scale_m);

    if (active) {
#pragma unroll
      for (int j = 0; j < SRS_MAX_PER_THREAD; ++j)
        if ((uint32_t)j < per_thread) {
          const float2 v = res[lane + (uint32_t)j * tpr];
          acc[j] += v.x * v.x + v.y * v.y;
        }
    }
    __syncthreads();   // the next load writes buf0, which may be `res`
  }

  // ---- fold: the rows' sums, in ascending row order, into row 0's place; then the window ----
  float* rows = reinterpret_cast<float*>(srs_lds);   // [rpw][N]; the loop's last barrier is behind every read of the buffers
#pragma unroll
  for (int j = 0; j < SRS_MAX_PER_THREAD; ++j)
    if ((uint32_t)j < per_thread) rows[rl * N + lane + (uint32_t)j * tpr] = acc[j];
  __syncthreads();
  for (uint32_t n = threadIdx.x; n < N; n += TP_NT) {   // thread t alone touches the index n = t + 256 j of any row here
    float p = rows[n];
    for (uint32_t q = 1; q < rpw; ++q) p += rows[q * N + n];
    rows[n] = p;
  }
  __syncthreads();
  float* prof = profile + (int64_t)blockIdx.x * P.win_len;
  for (uint32_t d = threadIdx.x; d < P.win_len; d += TP_NT) prof[d] = rows[(d + N - P.guard) & mask];   // guard < N
}

__global__ __launch_bounds__(TP_NT) void ce_srs_estimate_kernel(SrsDev P, SrsTables T, const float2* __restrict__ tw, const float2* __restrict__ y,
                                                                int64_t st_b, int64_t st_r, int64_t st_sym, uint32_t n_rx,
                                                                const int32_t* __restrict__ slot, const int32_t* __restrict__ n_id, int64_t st_slot,
                                                                int64_t st_id, const int32_t* __restrict__ delay, int64_t st_delay,
                                                                float2* __restrict__ h_sb, float2* __restrict__ h_wb, float* __restrict__ noise,
                                                                float* __restrict__ epre) {
  __shared__ float2 w[SRS_MAX_M];
  __shared__ float2 g_row[SRS_MAX_M];
  __shared__ float2 hsb[SRS_MAX_AP * SRS_MAX_SYMB * SRS_MAX_BLOCKS];   // [port][symbol][block], the item's
  __shared__ float2 rho[SRS_MAX_AP * SRS_MAX_CS];
  __shared__ uint32_t hw[SRS_HW_WORDS];
  __shared__ float wave_sum[8];
  const uint32_t tid = threadIdx.x, M = P.m, Q = P.q_len, mask = P.f.m - 1u;
  const uint32_t b = blockIdx.x / n_rx, r = blockIdx.x - b * n_rx;
  const uint32_t u_slot = (uint32_t)slot[(int64_t)b * st_slot] % P.slots_per_frame, u_id = (uint32_t)n_id[(int64_t)b * st_id];
  const uint32_t dm = delay ? (uint32_t)delay[(int64_t)b * st_delay] & mask : 0u;   // delay mod N (N = 2^n: also of a negative value)
  uint32_t qs[SRS_MAX_SYMB];
  for (uint32_t i = tid; i < P.n_w; i += TP_NT) w[i] = T.wtab[i];
  if (tid < P.n_ap * P.n_cs_max) rho[tid] = T.rho[tid];
  srs_hop(P, T, u_slot, u_id, hw, qs);   // its barriers also publish w and rho
  const float2* y_item = y + ((int64_t)b * st_b + (int64_t)r * st_r);
  float2* hsb_out = h_sb + (int64_t)blockIdx.x * (P.n_ap * P.n_symb * P.n_blocks);
  float part_n = 0.0f, part_e = 0.0f;

  for (uint32_t s = 0; s < P.n_symb; ++s) {
    const uint32_t q = srs_pick(qs, s);
    for (uint32_t ci = 0; ci < P.n_combs; ++ci) {
      const float2* row = y_item + ((int64_t)(P.l0 + s) * st_sym + (int64_t)(P.start_re[s] + P.combs[ci]));
      for (uint32_t n = tid; n < M; n += TP_NT) {
        const float2 v = row[(size_t)P.k_tc * n];
        part_e += v.x * v.x + v.y * v.y;
        g_row[n] = tp_cmul(srs_cmulc(v, srs_base(P, T, w, q, n)), tw[(n * dm) & mask]);   // n dm < 2^23
      }
      __syncthreads();
      for (uint32_t idx = tid; idx < P.n_ap * P.n_blocks; idx += TP_NT) {   // one thread per (port, block)
        const uint32_t i = idx / P.n_blocks, j = idx - i * P.n_blocks;
        if (P.port_slot[i] == ci) {
          const float2* rho_i = rho + i * P.n_cs_max;
          float2 a = make_float2(0.0f, 0.0f);
          for (uint32_t k = 0; k < Q; ++k) {   // Q is a multiple of n_cs_max: the shift's phase starts anew in every block
            const uint32_t n = j * Q + k;
            a = a + srs_cmulc(g_row[n], rho_i[k % P.n_cs_max]);
          }
          const float2 h = P.inv_q * a;
          const uint32_t o = (i * P.n_symb + s) * P.n_blocks + j;
          hsb[o] = h;
          hsb_out[o] = h;
        }
      }
      __syncthreads();
      for (uint32_t n = tid; n < M; n += TP_NT) {
        const uint32_t j = n / Q, c = n % P.n_cs_max;
        float2 e = g_row[n];
        for (uint32_t i = 0; i < P.n_ap; ++i)
          if (P.port_slot[i] == ci) e = e - tp_cmul(hsb[(i * P.n_symb + s) * P.n_blocks + j], rho[i * P.n_cs_max + c]);
        part_n += e.x * e.x + e.y * e.y;
      }
      __syncthreads();   // the next (s, comb) writes g_row
    }
  }

  if (tid < P.n_ap) {   // the wideband mean: s outer, the blocks ascending
    float2 a = make_float2(0.0f, 0.0f);
    const float2* hp = hsb + tid * P.n_symb * P.n_blocks;
    for (uint32_t k = 0; k < P.n_symb * P.n_blocks; ++k) a = a + hp[k];
    h_wb[(int64_t)blockIdx.x * P.n_ap + tid] = P.inv_wb * a;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    part_n += __shfl_xor(part_n, off);
    part_e += __shfl_xor(part_e, off);
  }
  if ((tid & 63u) == 0u) {
    wave_sum[tid >> 6] = part_n;
    wave_sum[4 + (tid >> 6)] = part_e;
  }
  __syncthreads();
  if (tid == 0u) {
    noise[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3])) * P.inv_dof;
    epre[blockIdx.x] = ((wave_sum[4] + wave_sum[5]) + (wave_sum[6] + wave_sum[7])) * P.inv_re;
  }
}

// ---- host derivation: integers only (the sequence integers are ce_dmrs_lp.hip's, restated) ----

struct SrsHost {
  SrsDev dev{};
  ce_tp_host_view view{};
  int32_t info[SRS_INFO_LEN] = {0};
  int32_t port_comb[SRS_MAX_AP] = {0}, port_cs[SRS_MAX_AP] = {0};
  std::vector<int32_t> q;        // [30][2]
  std::vector<uint16_t> tri;     // [M]
  std::vector<uint8_t> code;     // table form: [30][M]
  std::vector<uint32_t> hop;     // [32][nw]
};

int srs_largest_prime_below(int m) {
  for (int n = m - 1; n >= 2; --n) {
    bool prime = true;
    for (int d = 2; d * d <= n && prime; ++d) prime = n % d != 0;
    if (prime) return n;
  }
  return 0;
}

// The comb geometry: validation of k_tc, n_ap, n_cs, k_bar, m_srs and the ports' (comb, cs) into H.
int srs_derive_ports(int32_t k_tc, int32_t n_ap, int32_t n_cs, int32_t k_bar, int32_t m_srs, SrsHost* H) {
  if (k_tc != 2 && k_tc != 4) return ce_fail(CE_ERR_INVALID, "k_tc=%d is not 2 or 4", k_tc);
  if (n_ap != 1 && n_ap != 2 && n_ap != 4) return ce_fail(CE_ERR_INVALID, "n_ap=%d is not 1, 2 or 4", n_ap);
  const int n_cs_max = k_tc == 2 ? 8 : 12;
  if (n_cs < 0 || n_cs >= n_cs_max) return ce_fail(CE_ERR_INVALID, "n_cs=%d outside 0..%d", n_cs, n_cs_max - 1);
  if (k_bar < 0 || k_bar >= k_tc) return ce_fail(CE_ERR_INVALID, "k_bar=%d outside 0..%d", k_bar, k_tc - 1);
  if (m_srs < 4 || m_srs > 272 || m_srs % 4) return ce_fail(CE_ERR_INVALID, "m_srs=%d is not a multiple of 4 in 4..272", m_srs);
  SrsDev& P = H->dev;
  const bool upper = n_ap == 4 && n_cs >= n_cs_max / 2;
  for (int i = 0; i < n_ap; ++i) {
    H->port_cs[i] = upper ? (n_cs + n_cs_max * (i / 2) / 2) % n_cs_max : (n_cs + n_cs_max * i / n_ap) % n_cs_max;
    H->port_comb[i] = upper && (i & 1) ? (k_bar + k_tc / 2) % k_tc : k_bar;
  }
  P.k_tc = (uint32_t)k_tc;
  P.n_ap = (uint32_t)n_ap;
  P.n_cs_max = (uint32_t)n_cs_max;
  P.m = (uint32_t)(12 * m_srs / k_tc);
  P.q_len = (uint32_t)(48 / k_tc);
  P.n_blocks = (uint32_t)(m_srs / 4);
  P.n_combs = 0;
  for (int i = 0; i < n_ap; ++i) {
    uint32_t slot = P.n_combs;
    for (uint32_t c = 0; c < P.n_combs; ++c)
      if (P.combs[c] == (uint32_t)H->port_comb[i]) slot = c;
    if (slot == P.n_combs) P.combs[P.n_combs++] = (uint32_t)H->port_comb[i];
    P.port_slot[i] = slot;
    P.port_comb[i] = (uint32_t)H->port_comb[i];
  }
  if (P.m >= 36) {
    P.form = CE_DMRS_LP_FORM_ZC;
    P.n_zc = (uint32_t)srs_largest_prime_below((int)P.m);   // > M / 2: an index wraps at most once
    P.n_zc_magic = (uint32_t)(0x100000000ull / P.n_zc);
    P.n_w = P.n_zc;
  } else {   // M = 12 or 24 (30 cannot occur: M is a multiple of 12)
    P.form = CE_DMRS_LP_FORM_PHI;
    P.n_zc = 0;
    P.n_zc_magic = 0;
    P.n_w = 4;
  }
  return CE_OK;
}

int srs_derive(int32_t k_tc, int32_t n_ap, int32_t n_cs, int32_t k_bar, int32_t m_srs, int32_t n_symb, int32_t l0, const int32_t* start_prb,
               int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot, int32_t hopping, int32_t slots_per_frame, int32_t n_fft, int32_t win_len,
               const int8_t* phi, SrsHost* H) {
  if (const int rc = srs_derive_ports(k_tc, n_ap, n_cs, k_bar, m_srs, H); rc != CE_OK) return rc;
  SrsDev& P = H->dev;
  if (n_symb != 1 && n_symb != 2 && n_symb != 4) return ce_fail(CE_ERR_INVALID, "n_symb=%d is not 1, 2 or 4", n_symb);
  if (n_symb_slot != 12 && n_symb_slot != 14) return ce_fail(CE_ERR_INVALID, "n_symb_slot=%d, expected 14 or 12", n_symb_slot);
  if (n_sym < 1 || n_sym > n_symb_slot) return ce_fail(CE_ERR_INVALID, "n_sym=%d outside 1..n_symb_slot=%d", n_sym, n_symb_slot);
  if (l0 < 0 || l0 > n_sym - n_symb) return ce_fail(CE_ERR_INVALID, "l0=%d: %d symbols from it do not lie inside the %d of the grid", l0, n_symb, n_sym);
  if (n_prb_grid < 1 || n_prb_grid > SRS_MAX_PRB_GRID) return ce_fail(CE_ERR_INVALID, "n_prb_grid=%d outside 1..%d", n_prb_grid, SRS_MAX_PRB_GRID);
  if (!start_prb) return ce_fail(CE_ERR_INVALID, "null argument");
  for (int s = 0; s < n_symb; ++s) {
    if (start_prb[s] < 0 || start_prb[s] > n_prb_grid - m_srs)
      return ce_fail(CE_ERR_INVALID, "start_prb[%d]=%d: %d PRB from it do not lie inside the grid of %d", s, start_prb[s], m_srs, n_prb_grid);
    P.start_re[s] = 12u * (uint32_t)start_prb[s];
  }
  if (hopping != CE_DMRS_LP_HOP_NEITHER && hopping != CE_DMRS_LP_HOP_GROUP && hopping != CE_DMRS_LP_HOP_SEQUENCE)
    return ce_fail(CE_ERR_INVALID, "hopping=%d is not one of neither (0), group (1), sequence (2)", hopping);
  if (slots_per_frame != 10 && slots_per_frame != 20 && slots_per_frame != 40 && slots_per_frame != 80 && slots_per_frame != 160)
    return ce_fail(CE_ERR_INVALID, "slots_per_frame=%d, expected 10, 20, 40, 80 or 160", slots_per_frame);
  if (n_fft != 128 && n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048 && n_fft != 4096)
    return ce_fail(CE_ERR_INVALID, "n_fft=%d is not 128, 256, 512, 1024, 2048 or 4096", n_fft);
  const int m = (int)P.m;
  if (n_fft <= m) return ce_fail(CE_ERR_INVALID, "n_fft=%d must exceed M=%d", n_fft, m);
  if (win_len < 1 || win_len > n_fft) return ce_fail(CE_ERR_INVALID, "win_len=%d outside 1..n_fft=%d", win_len, n_fft);
  if (!fft_derive(n_fft, 1, &H->view)) return ce_fail(CE_ERR_INVALID, "n_fft=%d has no radix sequence", n_fft);   // (not reached: powers of two)
  P.n_symb = (uint32_t)n_symb;
  P.l0 = (uint32_t)l0;
  P.hopping = (uint32_t)hopping;
  P.n_symb_slot = (uint32_t)n_symb_slot;
  P.slots_per_frame = (uint32_t)slots_per_frame;
  P.v_live = hopping == CE_DMRS_LP_HOP_SEQUENCE && m >= 72 ? 1u : 0u;
  P.win_len = (uint32_t)win_len;
  P.guard = (uint32_t)((n_fft + m - 1) / m);
  H->q.assign(60, 0);
  H->tri.assign((size_t)m, 0);
  if (P.form == CE_DMRS_LP_FORM_ZC) {
    const int n = (int)P.n_zc;
    for (int u = 0; u < 30; ++u)
      for (int v = 0; v < 2; ++v) {
        const int two_qbar = 2 * n * (u + 1);   // 31 * 2 q_bar
        H->q[2 * u + v] = (two_qbar + 31) / 62 + ((two_qbar / 31) % 2 == 0 ? v : -v);
      }
    for (int k = 0; k < m; ++k) {
      const int64_t t = k % n;
      H->tri[k] = (uint16_t)((t * (t + 1) / 2) % n);
    }
  } else {
    if (!phi) return ce_fail(CE_ERR_UNSUPPORTED, "M=%d needs the phi table of 38.211 5.2.2.2, which the caller provides", m);
    H->code.assign((size_t)30 * m, 0);
    for (int i = 0; i < 30 * m; ++i) {
      const int f = phi[i];
      if (f != -3 && f != -1 && f != 1 && f != 3) return ce_fail(CE_ERR_INVALID, "phi[%d][%d]=%d is not one of -3, -1, 1, 3", i / m, i % m, f);
      H->code[i] = (uint8_t)((f + 3) / 2);   // -3, -1, 1, 3 -> 0 .. 3
    }
  }
  const int n_pos = n_symb_slot * slots_per_frame;
  const int nw = hopping == CE_DMRS_LP_HOP_GROUP ? (n_pos + 3) / 4 : hopping == CE_DMRS_LP_HOP_SEQUENCE ? (n_pos + 31) / 32 : 0;   // <= CE_DMRS_LP_MAX_WORDS
  P.nw = (uint32_t)nw;
  H->hop.assign((size_t)32 * nw, 0u);
  if (nw) {
    ce_gold_words<false>(1u, 0, nw - 1, H->hop.data());
    for (int i = 0; i < 31; ++i) ce_gold_words<true>(1u << i, 0, nw - 1, H->hop.data() + (size_t)(1 + i) * nw);
  }
  int per_comb[4] = {0, 0, 0, 0}, fullest = 0;
  for (int i = 0; i < n_ap; ++i) fullest = ++per_comb[H->port_comb[i]] > fullest ? per_comb[H->port_comb[i]] : fullest;
  const int gap = (int)P.n_cs_max / fullest;
  const int dof = n_symb * (int)P.n_combs * m - n_symb * n_ap * (int)P.n_blocks;   // > 0: Q >= 12 > n_ap
  P.scale_m = (float)(1.0 / (double)m);
  P.inv_q = (float)(1.0 / (double)P.q_len);
  P.inv_wb = (float)(1.0 / (double)(n_symb * (int)P.n_blocks));
  P.inv_dof = (float)(1.0 / (double)dof);
  P.inv_re = (float)(1.0 / (double)(n_symb * (int)P.n_combs * m));
  P.f = fft_dev(H->view, 1);
  const int32_t info[SRS_INFO_LEN] = {m, (int32_t)P.q_len, (int32_t)P.n_blocks, (int32_t)P.n_combs, (int32_t)P.form, (int32_t)P.n_zc, (int32_t)P.guard,
                                      (int32_t)((int64_t)n_fft * gap / (int)P.n_cs_max) - (int32_t)P.guard, nw, (int32_t)P.v_live};
  memcpy(H->info, info, sizeof(info));
  return CE_OK;
}

// W_n[e] = (float32(cos th), float32(-sin th)), th = 2 pi e / n in double; W_n[0] = (1, +0): lp_twiddles of ce_dmrs_lp.hip.  The
// table form: the four values exp(j phi pi / 4), code c <-> phi = 2 c - 3.
void srs_w_table(const SrsDev& P, float* w) {
  if (P.form == CE_DMRS_LP_FORM_PHI) {
    const uint32_t neg = SRS_A | 0x80000000u, re[4] = {neg, SRS_A, SRS_A, neg}, im[4] = {neg, neg, SRS_A, SRS_A};
    for (int c = 0; c < 4; ++c) {
      memcpy(&w[2 * c], &re[c], 4);
      memcpy(&w[2 * c + 1], &im[c], 4);
    }
    return;
  }
  const int n = (int)P.n_zc;
  for (int e = 0; e < n; ++e) {
    const double th = 2.0 * M_PI * (double)e / (double)n;
    w[2 * e] = (float)cos(th);
    w[2 * e + 1] = e ? (float)-sin(th) : 0.0f;
  }
}

// rho_i[n] = exp(+j 2 pi cs_i n / n_cs_max), n < n_cs_max, in double, rounded once: [n_ap][n_cs_max] (re, im) pairs.
void srs_rho_table(const SrsHost& H, float* rho) {
  const double two_pi = 6.283185307179586476925286766559;
  const int ncs = (int)H.dev.n_cs_max;
  for (int i = 0; i < (int)H.dev.n_ap; ++i)
    for (int n = 0; n < ncs; ++n) {
      const double a = two_pi * (double)((H.port_cs[i] * n) % ncs) / (double)ncs;
      rho[2 * (i * ncs + n)] = (float)cos(a);
      rho[2 * (i * ncs + n) + 1] = (float)sin(a);
    }
}

}  // namespace

struct ce_srs_plan {
  FftPlan core;
  SrsDev dev{};
  bool stage_w = false;
  int lds_profile = 0;
  float2* w = nullptr;
  float2* rho = nullptr;
  uint16_t* qtab = nullptr;
  uint16_t* tri = nullptr;
  uint8_t* code = nullptr;
  uint32_t* hop = nullptr;
};

extern "C" int ce_srs_derive_host(int32_t k_tc, int32_t n_ap, int32_t n_cs, int32_t k_bar, int32_t m_srs, int32_t n_symb, int32_t l0,
                                  const int32_t* start_prb, int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot, int32_t hopping,
                                  int32_t slots_per_frame, int32_t n_fft, int32_t win_len, const int8_t* phi, ce_tp_host_view* view, int32_t* info,
                                  int32_t* port_comb, int32_t* port_cs, int32_t* q, int32_t* tri, uint32_t* hop_words) {
  SrsHost H;
  if (const int rc = srs_derive(k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, l0, start_prb, n_prb_grid, n_sym, n_symb_slot, hopping, slots_per_frame, n_fft,
                                win_len, phi, &H);
      rc != CE_OK)
    return rc;
  if (view) *view = H.view;
  if (info) memcpy(info, H.info, sizeof(H.info));
  if (port_comb) memcpy(port_comb, H.port_comb, sizeof(H.port_comb));
  if (port_cs) memcpy(port_cs, H.port_cs, sizeof(H.port_cs));
  if (q) memcpy(q, H.q.data(), 60 * sizeof(int32_t));
  if (tri)
    for (uint32_t k = 0; k < H.dev.m; ++k) tri[k] = H.tri[k];
  if (hop_words && !H.hop.empty()) memcpy(hop_words, H.hop.data(), H.hop.size() * sizeof(uint32_t));
  return CE_OK;
}

extern "C" int ce_srs_copy_tables(int32_t k_tc, int32_t n_ap, int32_t n_cs, int32_t k_bar, int32_t m_srs, int32_t n_fft, float* twiddles, float* w_zc,
                                  float* rho) {
  SrsHost H;
  if (const int rc = srs_derive_ports(k_tc, n_ap, n_cs, k_bar, m_srs, &H); rc != CE_OK) return rc;
  if (twiddles) {
    ce_tp_host_view v;
    if (n_fft < 128 || n_fft > 4096 || (n_fft & (n_fft - 1)) || !fft_derive(n_fft, 1, &v))
      return ce_fail(CE_ERR_INVALID, "n_fft=%d is not 128, 256, 512, 1024, 2048 or 4096", n_fft);
    fft_twiddles(n_fft, twiddles);
  }
  if (w_zc) srs_w_table(H.dev, w_zc);
  if (rho) srs_rho_table(H, rho);
  return CE_OK;
}

extern "C" void ce_srs_plan_destroy(ce_srs_plan* p) {
  if (!p) return;
  if (p->w) (void)hipFree(p->w);
  if (p->rho) (void)hipFree(p->rho);
  if (p->qtab) (void)hipFree(p->qtab);
  if (p->tri) (void)hipFree(p->tri);
  if (p->code) (void)hipFree(p->code);
  if (p->hop) (void)hipFree(p->hop);
  fft_plan_destroy(p);
}

extern "C" int ce_srs_plan_create(int32_t abi_version, int32_t device, int32_t k_tc, int32_t n_ap, int32_t n_cs, int32_t k_bar, int32_t m_srs,
                                  int32_t n_symb, int32_t l0, const int32_t* start_prb, int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot,
                                  int32_t hopping, int32_t slots_per_frame, int32_t n_fft, int32_t win_len, const int8_t* phi, ce_srs_plan** out) {
  if (!out) return ce_fail(CE_ERR_INVALID, "null argument");
  if (abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", abi_version, CE_ABI_VERSION);
  SrsHost H;
  if (const int rc = srs_derive(k_tc, n_ap, n_cs, k_bar, m_srs, n_symb, l0, start_prb, n_prb_grid, n_sym, n_symb_slot, hopping, slots_per_frame, n_fft,
                                win_len, phi, &H);
      rc != CE_OK)
    return rc;
  auto p = ce_new_plan<ce_srs_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->dev = H.dev;
  const SrsDev& P = H.dev;
  p->stage_w = H.view.lds_bytes + 8 * (int)P.n_w <= 65536;   // N = 4096 fills the 64 KiB with its buffers
  p->lds_profile = H.view.lds_bytes + (p->stage_w ? 8 * (int)P.n_w : 0);
  std::vector<float> w(2 * (size_t)P.n_w), rho(2 * (size_t)P.n_ap * P.n_cs_max);
  srs_w_table(P, w.data());
  srs_rho_table(H, rho.data());
  std::vector<uint16_t> qtab(60);
  for (int i = 0; i < 60; ++i) qtab[i] = (uint16_t)H.q[i];   // 0 <= q <= N_ZC
  if (H.code.empty()) H.code.assign(1, 0);                    // every table has an allocation behind its pointer
  if (H.hop.empty()) H.hop.assign(1, 0u);
  hipError_t e = fft_plan_upload(&p->core, device, H.view);
  {
    CeDeviceScope scope(device);
    if (e == hipSuccess) e = scope.err;
    e = ce_upload(e, &p->w, w.data(), w.size() * sizeof(float));
    e = ce_upload(e, &p->rho, rho.data(), rho.size() * sizeof(float));
    e = ce_upload(e, &p->qtab, qtab.data(), qtab.size() * sizeof(uint16_t));
    e = ce_upload(e, &p->tri, H.tri.data(), H.tri.size() * sizeof(uint16_t));
    e = ce_upload(e, &p->code, H.code.data(), H.code.size());
    e = ce_upload(e, &p->hop, H.hop.data(), H.hop.size() * sizeof(uint32_t));
  }
  if (e != hipSuccess) {
    ce_srs_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "SRS estimator plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

namespace {

// What both launches check alike; *n_wg: the workgroups of the launch (0: nothing to do).
int srs_check_launch(const ce_srs_plan* p, const void* y, int64_t st_b, int64_t st_r, int64_t st_sym, int64_t n_items, int32_t n_rx, const int32_t* slot,
                     int64_t slot_stride, const int32_t* n_id, int64_t n_id_stride, int64_t* n_wg) {
  *n_wg = 0;
  if (!p) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_items < 0) return ce_fail(CE_ERR_INVALID, "n_items=%lld", (long long)n_items);
  if (n_rx < 1 || n_rx > SRS_MAX_RX) return ce_fail(CE_ERR_INVALID, "n_rx=%d outside 1..%d", n_rx, SRS_MAX_RX);
  if (n_items == 0) return CE_OK;
  if (!y || !slot || !n_id) return ce_fail(CE_ERR_INVALID, "null argument");
  if (st_b < 0 || st_r < 0 || st_sym < 0 || slot_stride < 0 || n_id_stride < 0)
    return ce_fail(CE_ERR_INVALID, "item_stride=%lld, port_stride=%lld, symbol_stride=%lld, slot_stride=%lld and n_id_stride=%lld must be >= 0",
                   (long long)st_b, (long long)st_r, (long long)st_sym, (long long)slot_stride, (long long)n_id_stride);
  if (reinterpret_cast<uintptr_t>(y) & 7u) return ce_fail(CE_ERR_INVALID, "y must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(n_id)) & 3u) return ce_fail(CE_ERR_INVALID, "slot and n_id must be 4-byte aligned");
  if (const int rc = ce_rows_workgroups(n_items, (int64_t)n_rx, 1, n_wg); rc != CE_OK) {
    *n_wg = 0;
    return rc;
  }
  const int64_t room = INT64_MAX >> 6;
  if (st_b > room / n_items || st_r > room / n_rx || st_sym > room / 16 || slot_stride > room / n_items || n_id_stride > room / n_items) {
    *n_wg = 0;
    return ce_fail(CE_ERR_INVALID, "item_stride=%lld, port_stride=%lld, symbol_stride=%lld: the extent of y exceeds the address space", (long long)st_b,
                   (long long)st_r, (long long)st_sym);
  }
  return CE_OK;
}

SrsTables srs_tables(const ce_srs_plan* p) { return {p->w, p->rho, p->qtab, p->tri, p->code, p->hop}; }

}  // namespace

extern "C" int ce_srs_profile(const ce_srs_plan* p, const void* y, int64_t item_stride, int64_t port_stride, int64_t symbol_stride, int64_t n_items,
                              int32_t n_rx, const int32_t* slot, int64_t slot_stride, const int32_t* n_id, int64_t n_id_stride, float* profile,
                              void* stream) {
  int64_t n_wg;
  if (const int rc = srs_check_launch(p, y, item_stride, port_stride, symbol_stride, n_items, n_rx, slot, slot_stride, n_id, n_id_stride, &n_wg); rc != CE_OK)
    return rc;
  if (n_wg == 0) return CE_OK;
  if (!profile) return ce_fail(CE_ERR_INVALID, "null argument");
  if (reinterpret_cast<uintptr_t>(profile) & 3u) return ce_fail(CE_ERR_INVALID, "profile must be 4-byte aligned");
  CeDeviceScope scope(p->core.device);
  if (scope.err != hipSuccess) return ce_device_fail(p->core.device, scope.err);
  const float2* yy = reinterpret_cast<const float2*>(y);
  const hipStream_t st = (hipStream_t)stream;
  if (p->stage_w)
    hipLaunchKernelGGL((ce_srs_profile_kernel<true>), dim3((unsigned)n_wg), dim3(TP_NT), (size_t)p->lds_profile, st, p->dev, srs_tables(p), p->core.tw, yy,
                       item_stride, port_stride, symbol_stride, (uint32_t)n_rx, slot, n_id, slot_stride, n_id_stride, profile);
  else
    hipLaunchKernelGGL((ce_srs_profile_kernel<false>), dim3((unsigned)n_wg), dim3(TP_NT), (size_t)p->lds_profile, st, p->dev, srs_tables(p), p->core.tw, yy,
                       item_stride, port_stride, symbol_stride, (uint32_t)n_rx, slot, n_id, slot_stride, n_id_stride, profile);
  return ce_launch_status("SRS delay profile");
}

extern "C" int ce_srs_estimate(const ce_srs_plan* p, const void* y, int64_t item_stride, int64_t port_stride, int64_t symbol_stride, int64_t n_items,
                               int32_t n_rx, const int32_t* slot, int64_t slot_stride, const int32_t* n_id, int64_t n_id_stride, const int32_t* delay,
                               int64_t delay_stride, void* h_sb, void* h_wb, float* noise, float* epre, void* stream) {
  int64_t n_wg;
  if (const int rc = srs_check_launch(p, y, item_stride, port_stride, symbol_stride, n_items, n_rx, slot, slot_stride, n_id, n_id_stride, &n_wg); rc != CE_OK)
    return rc;
  if (n_wg == 0) return CE_OK;
  if (!h_sb || !h_wb || !noise || !epre) return ce_fail(CE_ERR_INVALID, "null argument");
  if (delay_stride < 0 || delay_stride > (INT64_MAX >> 6) / n_items) return ce_fail(CE_ERR_INVALID, "delay_stride=%lld must be >= 0 and inside the address space", (long long)delay_stride);
  if (reinterpret_cast<uintptr_t>(delay) & 3u) return ce_fail(CE_ERR_INVALID, "delay must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(h_sb) | reinterpret_cast<uintptr_t>(h_wb)) & 7u) return ce_fail(CE_ERR_INVALID, "h_sb and h_wb must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(noise) | reinterpret_cast<uintptr_t>(epre)) & 3u) return ce_fail(CE_ERR_INVALID, "noise and epre must be 4-byte aligned");
  CeDeviceScope scope(p->core.device);
  if (scope.err != hipSuccess) return ce_device_fail(p->core.device, scope.err);
  hipLaunchKernelGGL(ce_srs_estimate_kernel, dim3((unsigned)n_wg), dim3(TP_NT), 0, (hipStream_t)stream, p->dev, srs_tables(p), p->core.tw,
                     reinterpret_cast<const float2*>(y), item_stride, port_stride, symbol_stride, (uint32_t)n_rx, slot, n_id, slot_stride, n_id_stride, delay,
                     delay_stride, reinterpret_cast<float2*>(h_sb), reinterpret_cast<float2*>(h_wb), noise, epre);
  return ce_launch_status("SRS estimate");
}

// EXTENSION (no reference counterpart, see include/ce_eq.h): noise-whitened unbiased LMMSE equalizer over the PUSCH data
// REs, consuming ce_estimate_batch's ch_est [slot][port][sc][sym][layer] and noise [slot][port].
//
// Kernel: one 256-thread workgroup per (slot, chunk of EQ_CH = 36 subcarriers over all symbols); only the chunks the
// hops' PRBs touch are launched.
//   1. rx of the chunk's data REs goes into the LDS, [port][sym][sc] with rows padded by one element.  The load loop
//      runs subcarrier-fastest (or symbol-fastest where that is rx's unit stride), so the [slot][port][sym][sc] layout
//      is read in runs of consecutive addresses; any other element strides are merely slower.
//   2. barrier.  A slot's ch_est item is contiguous in (sc, sym, layer): thread t owns flat elements t and t + 256 of the
//      chunk, e = sc * n_sym + sym, so a port's h is 8 L contiguous bytes per lane and consecutive lanes read consecutive
//      addresses (8-byte loads for L = 1 and 3, 16-byte loads for L = 2 and 4).  y comes back from the LDS transposed.
//      A and z accumulate port by port in registers; Cholesky, the inverse of the factor and the two outputs follow.
//   3. barrier, results into the LDS (over the rx region), barrier, and out in output order: lanes walk a symbol's
//      subcarriers, each storing the L layers of one row, so a symbol's chunk leaves as one contiguous run.
// Every address is built from the block index, the thread index and the host-derived per-symbol table (the host has
// walked every data RE through the same row formula against n_data_re); noise and tensor values only enter arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <memory>

#include "ce_eq.h"
#include "ce_remap.h"
#include "ce_stage.h"

namespace {

constexpr int EQ_NT = 256;
constexpr int EQ_CH = CE_EQ_CHUNK_SC;
constexpr int EQ_RXROW = EQ_CH + 1;   // LDS row of one (port, symbol): padded so the transposed read spreads over the banks
static_assert(EQ_CH % 12 == 0 && EQ_CH * CE_MAX_SYMBOLS <= 2 * EQ_NT, "two REs per thread cover a chunk");

// per symbol (ce_remap_entry): x = first subcarrier of the hop's PRBs | one past the last << 16, y = data mask | data REs
// per PRB << 16, z = first output row, w unused.  No hop on the symbol: all zero.
struct EqDev {
  uint32_t n_sym, n_sc, n_elem;   // n_elem = EQ_CH * n_sym
  uint32_t sym_magic;             // floor(2^16 / n_sym) + 1: e / n_sym = (e * sym_magic) >> 16 for e < 2 * EQ_NT (host-checked)
  uint32_t chunk0, n_chunks;      // chunks launched per slot: chunk0 .. chunk0 + n_chunks - 1
  uint32_t n_data_re;
};

}  // namespace

struct ce_eq_plan {
  int device = 0;
  int n_layers = 0;
  ce_eq_info info{};
  EqDev dev{};
  uint4* symtab = nullptr;   // [CE_MAX_SYMBOLS]
};

namespace {

struct EqSym {
  uint32_t lo, hi, mask, dpp, first_row;
};

__device__ __forceinline__ EqSym eq_sym(const uint4* st, uint32_t s) {
  const uint4 t = st[s];
  return {t.x & 0xFFFFu, t.x >> 16, t.y & 0xFFFFu, t.y >> 16, t.z};
}

// RE (sc0 + sc_l, symbol of `y`) carries data
__device__ __forceinline__ bool eq_is_data(const EqSym& y, uint32_t sc0, uint32_t sc_l) {
  const uint32_t sc = sc0 + sc_l;
  return sc >= y.lo && sc < y.hi && ((y.mask >> (sc_l % 12u)) & 1u);   // sc0 is a multiple of 12
}

template <int L>
__device__ __forceinline__ void eq_load_h(const float2* __restrict__ p, float2 (&h)[L]) {
  if constexpr (L == 2 || L == 4) {
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);   // ch_est 16-byte aligned (host), 8 L bytes per element
#pragma unroll
    for (int i = 0; i < L / 2; ++i) {
      const float4 v = p4[i];
      h[2 * i] = make_float2(v.x, v.y);
      h[2 * i + 1] = make_float2(v.z, v.w);
    }
  } else {
#pragma unroll
    for (int i = 0; i < L; ++i) h[i] = p[i];
  }
}

// One RE: A = I + sum_r w_r h_r^H h_r and z = sum_r w_r h_r^H y_r over the ports, then x_hat and nvar.
template <int L>
__device__ __forceinline__ void eq_solve(const float2* __restrict__ ch, int64_t port_stride, const float2* lrx, uint32_t rx_port_stride,
                                         const float* w_s, uint32_t R, float2 (&x)[L], float (&nv)[L]) {
  float ar[L][L], ai[L][L], zr[L], zi[L];   // lower triangle of A (row i, column j <= i)
#pragma unroll
  for (int i = 0; i < L; ++i) {
    zr[i] = zi[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < L; ++j) ar[i][j] = ai[i][j] = 0.0f;
  }
#pragma unroll 4
  for (uint32_t r = 0; r < R; ++r) {
    float2 h[L];
    eq_load_h<L>(ch + r * port_stride, h);
    const float2 y = lrx[r * rx_port_stride];
    const float w = w_s[r];
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const float cr = w * h[i].x, ci = -w * h[i].y;   // w conj(h_i)
      zr[i] += cr * y.x - ci * y.y;
      zi[i] += cr * y.y + ci * y.x;
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        ar[i][j] += cr * h[j].x - ci * h[j].y;
        if (j < i) ai[i][j] += cr * h[j].y + ci * h[j].x;
      }
    }
  }
  const float inf = __builtin_inff();
  if constexpr (L == 1) {
    const float g = ar[0][0];
    const bool ok = g > 0.0f;
    const float ig = 1.0f / g;
    x[0] = ok ? make_float2(zr[0] / g, zi[0] / g) : make_float2(0.0f, 0.0f);
    nv[0] = ok ? ig : inf;
  } else {
    // A = G G^H, G lower with a real positive diagonal (A >= I: no pivoting); M = G^-1
    float gr[L][L], gi[L][L], mr[L][L], mi[L][L], inv[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      float dj = 1.0f + ar[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) dj -= gr[j][k] * gr[j][k] + gi[j][k] * gi[j][k];
      inv[j] = 1.0f / sqrtf(dj);
#pragma unroll
      for (int i = j + 1; i < L; ++i) {
        float sr = ar[i][j], si = ai[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) {   // G[i][k] conj(G[j][k])
          sr -= gr[i][k] * gr[j][k] + gi[i][k] * gi[j][k];
          si -= gi[i][k] * gr[j][k] - gr[i][k] * gi[j][k];
        }
        gr[i][j] = sr * inv[j];
        gi[i][j] = si * inv[j];
      }
    }
#pragma unroll
    for (int j = 0; j < L; ++j) {
      mr[j][j] = inv[j];
      mi[j][j] = 0.0f;
#pragma unroll
      for (int i = j + 1; i < L; ++i) {
        float sr = 0.0f, si = 0.0f;
#pragma unroll
        for (int k = j; k < i; ++k) {
          sr += gr[i][k] * mr[k][j] - gi[i][k] * mi[k][j];
          si += gr[i][k] * mi[k][j] + gi[i][k] * mr[k][j];
        }
        mr[i][j] = -inv[i] * sr;
        mi[i][j] = -inv[i] * si;
      }
    }
    float ur[L], ui[L];   // u = M z
#pragma unroll
    for (int i = 0; i < L; ++i) {
      float sr = 0.0f, si = 0.0f;
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        sr += mr[i][j] * zr[j] - mi[i][j] * zi[j];
        si += mr[i][j] * zi[j] + mi[i][j] * zr[j];
      }
      ur[i] = sr;
      ui[i] = si;
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {   // A^-1 z = M^H u, [A^-1]_ll = sum_k |M[k][l]|^2
      float vr = 0.0f, vi = 0.0f, d = 0.0f;
#pragma unroll
      for (int k = l; k < L; ++k) {
        vr += mr[k][l] * ur[k] + mi[k][l] * ui[k];
        vi += mr[k][l] * ui[k] - mi[k][l] * ur[k];
        d += mr[k][l] * mr[k][l] + mi[k][l] * mi[k][l];
      }
      const float b = 1.0f - d;
      const bool ok = b > 0.0f;
      x[l] = ok ? make_float2(vr / b, vi / b) : make_float2(0.0f, 0.0f);
      nv[l] = ok ? d / b : inf;
    }
  }
}

template <int L>
__global__ __launch_bounds__(EQ_NT) void ce_eq_kernel(EqDev P, const uint4* __restrict__ symtab, const float2* __restrict__ rx, int64_t st_slot,
                                                      int64_t st_port, int64_t st_sc, int64_t st_sym, uint32_t sym_fast,
                                                      const float2* __restrict__ ch, const double* __restrict__ noise, uint32_t R,
                                                      float2* __restrict__ xo, float* __restrict__ no) {
  extern __shared__ __align__(16) unsigned char eq_lds[];
  __shared__ uint4 st_s[16];   // entries from n_sym on are zero: no data
  __shared__ float w_s[CE_EQ_MAX_PORTS];
  const uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x / P.n_chunks;
  const uint32_t sc0 = (P.chunk0 + (blockIdx.x - b * P.n_chunks)) * EQ_CH;
  if (tid < 16) st_s[tid] = tid < P.n_sym ? symtab[tid] : make_uint4(0u, 0u, 0u, 0u);
  if (tid >= 64 && tid < 64 + R) {
    const float n = (float)noise[(int64_t)b * R + (tid - 64)];
    w_s[tid - 64] = (n > 0.0f && n < __builtin_inff()) ? 1.0f / n : 0.0f;
  }
  __syncthreads();

  float2* lrx = reinterpret_cast<float2*>(eq_lds);   // [R][n_sym][EQ_RXROW]
  const uint32_t rx_port = P.n_sym * EQ_RXROW;
  {
    uint32_t li[2];
    int64_t off[2];
    bool live[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const uint32_t q = tid + it * EQ_NT;
      uint32_t s, sc_l;
      if (sym_fast) {
        sc_l = (q * P.sym_magic) >> 16;
        s = q - sc_l * P.n_sym;
      } else {
        s = q / EQ_CH;
        sc_l = q - s * EQ_CH;
      }
      live[it] = q < P.n_elem && eq_is_data(eq_sym(st_s, s), sc0, sc_l);
      li[it] = s * EQ_RXROW + sc_l;
      off[it] = (int64_t)(sc0 + sc_l) * st_sc + (int64_t)s * st_sym;
    }
    const float2* __restrict__ rxb = rx + (int64_t)b * st_slot;
#pragma unroll 4
    for (uint32_t r = 0; r < R; ++r) {
      const float2* __restrict__ p = rxb + (int64_t)r * st_port;
#pragma unroll
      for (int it = 0; it < 2; ++it)
        if (live[it]) lrx[r * rx_port + li[it]] = p[off[it]];
    }
  }
  __syncthreads();

  float2 x[2][L];
  float nv[2][L];
  bool data[2];
  const int64_t port_stride = (int64_t)P.n_sc * P.n_sym * L;
  const float2* __restrict__ chb = ch + ((int64_t)b * R * P.n_sc + sc0) * (int64_t)(P.n_sym * L);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const uint32_t e = tid + it * EQ_NT;
    const uint32_t sc_l = (e * P.sym_magic) >> 16;
    const uint32_t s = e - sc_l * P.n_sym;
    data[it] = e < P.n_elem && eq_is_data(eq_sym(st_s, s), sc0, sc_l);
    if (data[it]) eq_solve<L>(chb + (int64_t)e * L, port_stride, lrx + s * EQ_RXROW + sc_l, rx_port, w_s, R, x[it], nv[it]);
  }
  __syncthreads();   // every y has been read: the results go over the rx region

  float2* lx = reinterpret_cast<float2*>(eq_lds);                                        // [n_elem][L]
  float* ln = reinterpret_cast<float*>(eq_lds + (size_t)P.n_elem * L * sizeof(float2));  // [n_elem][L]; the offset is a multiple of 16
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const uint32_t e = tid + it * EQ_NT;
    if (data[it]) {
#pragma unroll
      for (int l = 0; l < L; ++l) {
        lx[e * L + l] = x[it][l];
        ln[e * L + l] = nv[it][l];
      }
    }
  }
  __syncthreads();

  float2* __restrict__ xb = xo + (int64_t)b * P.n_data_re * L;
  float* __restrict__ nb = no + (int64_t)b * P.n_data_re * L;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const uint32_t q = tid + it * EQ_NT;
    const uint32_t s = q / EQ_CH, sc_l = q - s * EQ_CH;
    if (q >= P.n_elem) continue;
    const EqSym y = eq_sym(st_s, s);
    if (!eq_is_data(y, sc0, sc_l)) continue;
    const uint32_t re = sc_l % 12u;
    const uint32_t row = y.first_row + ((sc0 + sc_l - re - y.lo) / 12u) * y.dpp + __popc(y.mask & ((1u << re) - 1u));
    const uint32_t e = sc_l * P.n_sym + s;
    if constexpr (L == 2 || L == 4) {   // x_hat and nvar 16-byte aligned (host): a row is 8 L / 4 L bytes
      const float4* lx4 = reinterpret_cast<const float4*>(lx + e * L);
      float4* __restrict__ o4 = reinterpret_cast<float4*>(xb + (int64_t)row * L);
#pragma unroll
      for (int i = 0; i < L / 2; ++i) o4[i] = lx4[i];
      if constexpr (L == 4)
        *reinterpret_cast<float4*>(nb + (int64_t)row * L) = *reinterpret_cast<const float4*>(ln + e * L);
      else
        *reinterpret_cast<float2*>(nb + (int64_t)row * L) = *reinterpret_cast<const float2*>(ln + e * L);
    } else {
#pragma unroll
      for (int l = 0; l < L; ++l) {
        xb[(int64_t)row * L + l] = lx[e * L + l];
        nb[(int64_t)row * L + l] = ln[e * L + l];
      }
    }
  }
}

size_t eq_lds_bytes(const EqDev& P, int L, int R) {
  const size_t rx = (size_t)R * P.n_sym * EQ_RXROW * sizeof(float2), out = (size_t)P.n_elem * L * (sizeof(float2) + sizeof(float));
  return rx > out ? rx : out;   // <= 8 * 14 * 37 * 8 = 33152
}

template <int L>
void eq_launch(const ce_eq_plan* p, unsigned n_wg, size_t lds, const float2* rx, const int64_t* st, uint32_t sym_fast, const float2* ch,
               const double* noise, uint32_t R, float2* xo, float* no, hipStream_t stream) {
  hipLaunchKernelGGL((ce_eq_kernel<L>), dim3(n_wg), dim3(EQ_NT), lds, stream, p->dev, p->symtab, rx, st[0], st[1], st[2], st[3], sym_fast, ch, noise,
                     R, xo, no);
}

// ---- host derivation: integers only ----

int eq_derive(const ce_eq_desc* d, ce_eq_host_view* v) {
  memset(v, 0, sizeof(*v));
  for (int s = 0; s < CE_MAX_SYMBOLS; ++s) v->sym_hop[s] = -1;
  if (d->abi_version != CE_ABI_VERSION) return ce_fail(CE_ERR_INVALID, "ABI version %d != %d", d->abi_version, CE_ABI_VERSION);
  return ce_remap_derive(*d, v);   // every other check, and the output order: symbol ascending, subcarrier ascending
}

}  // namespace

extern "C" int ce_eq_derive_host(const ce_eq_desc* d, ce_eq_host_view* v) {
  if (!d || !v) return ce_fail(CE_ERR_INVALID, "null argument");
  return eq_derive(d, v);
}

extern "C" int ce_eq_plan_create(const ce_eq_desc* d, ce_eq_plan** out) {
  if (!d || !out) return ce_fail(CE_ERR_INVALID, "null argument");
  ce_eq_host_view v;
  if (const int rc = eq_derive(d, &v); rc != CE_OK) return rc;
  auto p = ce_new_plan<ce_eq_plan>();
  if (!p) return ce_fail(CE_ERR_NOMEM, "out of host memory");
  p->device = d->device;
  p->n_layers = d->n_layers;
  p->info.n_data_re = v.n_data_re;
  p->info.bytes_per_slot = (int64_t)v.n_data_re * d->n_layers * 12;
  EqDev& P = p->dev;
  P.n_sym = (uint32_t)d->n_sym;
  P.n_sc = 12u * (uint32_t)d->n_prb_grid;
  P.n_elem = (uint32_t)EQ_CH * P.n_sym;
  P.sym_magic = 65536u / P.n_sym + 1u;
  for (uint32_t e = 0; e < 2u * EQ_NT; ++e)   // the kernel's division by multiplication, for every element index it forms
    if (((e * P.sym_magic) >> 16) != e / P.n_sym) return ce_fail(CE_ERR_UNSUPPORTED, "n_sym=%u: magic division fails at %u", P.n_sym, e);
  P.n_data_re = (uint32_t)v.n_data_re;
  uint4 tab[CE_MAX_SYMBOLS];
  memset(tab, 0, sizeof(tab));
  uint32_t sc_lo = P.n_sc, sc_hi = 0;
  for (int s = 0; s < d->n_sym; ++s) {
    if (v.sym_hop[s] < 0) continue;
    tab[s] = ce_remap_entry(v, s, d->hop[v.sym_hop[s]]);
    const uint32_t lo = tab[s].x & 0xFFFFu, hi = tab[s].x >> 16;
    sc_lo = lo < sc_lo ? lo : sc_lo;
    sc_hi = hi > sc_hi ? hi : sc_hi;
  }
  P.chunk0 = sc_lo / EQ_CH;
  P.n_chunks = (sc_hi + EQ_CH - 1) / EQ_CH - P.chunk0;
  CeDeviceScope scope(d->device);
  const hipError_t e = ce_upload(scope.err, &p->symtab, tab, sizeof(tab));
  if (e != hipSuccess) {
    ce_eq_plan_destroy(p.release());
    return ce_fail(CE_ERR_HIP, "equalizer plan upload: %s", hipGetErrorString(e));
  }
  *out = p.release();
  return CE_OK;
}

extern "C" void ce_eq_plan_destroy(ce_eq_plan* p) {
  if (!p) return;
  if (p->symtab) (void)hipFree(p->symtab);
  delete p;
}

extern "C" int ce_eq_plan_get_info(const ce_eq_plan* p, ce_eq_info* info) { return ce_get_info(p, info); }

extern "C" int ce_eq_equalize(const ce_eq_plan* p, const void* rx, const int64_t rx_strides[4], const void* ch_est, const double* noise,
                              int64_t n_slots, int32_t n_ports, void* x_hat, float* nvar, void* stream) {
  if (!p || !rx_strides) return ce_fail(CE_ERR_INVALID, "null argument");
  if (n_slots < 0) return ce_fail(CE_ERR_INVALID, "n_slots=%lld", (long long)n_slots);
  if (n_ports < 1 || n_ports > CE_EQ_MAX_PORTS) return ce_fail(CE_ERR_INVALID, "n_ports=%d outside 1..%d", n_ports, CE_EQ_MAX_PORTS);
  if (n_slots == 0) return CE_OK;
  if (!rx || !ch_est || !noise || !x_hat || !nvar) return ce_fail(CE_ERR_INVALID, "null argument");
  for (int i = 0; i < 4; ++i)
    if (rx_strides[i] < 0) return ce_fail(CE_ERR_INVALID, "negative strides are not supported");
  if ((reinterpret_cast<uintptr_t>(ch_est) | reinterpret_cast<uintptr_t>(x_hat) | reinterpret_cast<uintptr_t>(nvar)) & 15u)
    return ce_fail(CE_ERR_INVALID, "ch_est, x_hat and nvar must be 16-byte aligned");
  if (n_slots * (int64_t)p->dev.n_chunks > 0x7FFFFFFFll) return ce_fail(CE_ERR_UNSUPPORTED, "more than 2^31-1 workgroups in one launch");
  CeDeviceScope scope(p->device);
  if (scope.err != hipSuccess) return ce_device_fail(p->device, scope.err);
  const unsigned n_wg = (unsigned)(n_slots * (int64_t)p->dev.n_chunks);
  const size_t lds = eq_lds_bytes(p->dev, p->n_layers, n_ports);
  const uint32_t sym_fast = rx_strides[3] < rx_strides[2] ? 1u : 0u;   // walk rx along its shorter stride
  const float2* rxp = reinterpret_cast<const float2*>(rx);
  const float2* chp = reinterpret_cast<const float2*>(ch_est);
  float2* xo = reinterpret_cast<float2*>(x_hat);
  const hipStream_t st = (hipStream_t)stream;
  switch (p->n_layers) {
    case 1: eq_launch<1>(p, n_wg, lds, rxp, rx_strides, sym_fast, chp, noise, (uint32_t)n_ports, xo, nvar, st); break;
    case 2: eq_launch<2>(p, n_wg, lds, rxp, rx_strides, sym_fast, chp, noise, (uint32_t)n_ports, xo, nvar, st); break;
    case 3: eq_launch<3>(p, n_wg, lds, rxp, rx_strides, sym_fast, chp, noise, (uint32_t)n_ports, xo, nvar, st); break;
    default: eq_launch<4>(p, n_wg, lds, rxp, rx_strides, sym_fast, chp, noise, (uint32_t)n_ports, xo, nvar, st); break;
  }
  return ce_launch_status("equalizer");
}

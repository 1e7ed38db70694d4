// Dev microbenchmark (GPU box): does the ORDER in which a fused kernel's workgroups write their items move the store rate?
// The headline's write geometry exactly: 32 768 items of 366 912 B in one dense buffer, one 256-thread workgroup per item,
// 252 lanes x 16 B = 4032 B per workgroup iteration, 91 iterations per item, two workgroups per CU (dynamic LDS padded to
// 64 KB, as the 191-VGPR headline kernel gets), the estimator's `item_of` XCD deal as the base map.  Every order below is
// a fixed function of the workgroup index (no inter-workgroup communication) that writes every element exactly once;
// `check_orders()` proves that on the host before anything is launched.  Each order is timed write only and as
// "read the two DM-RS rows + pilots, reduce, then write" (rwmix<true, true>'s read form); a grid-stride sweep with 256 /
// 768 workgroups is the ceiling.  All orders run interleaved in one process, three passes.
// hipcc --offload-arch=gfx950 -O3 -o build/storeorder tools/micro/storeorder.hip && build/storeorder   (tools/micro/storeorder.sh)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

constexpr int N_SC = 3276, N_SYM = 14, N_RE = 1638, ROW4 = 7, ACTIVE = 252, NCH = N_SC * ROW4 / ACTIVE;  // 91 chunks of 4032 B
static_assert(NCH * ACTIVE == N_SC * ROW4, "item = whole chunks");
constexpr int N_SLOTS = 8192, N_PORTS = 4, N_ITEMS = N_SLOTS * N_PORTS, LDS_PAD = 64 * 1024;

// map: which item workgroup b writes (which items are resident together)
enum { MAP_XCD = 0,        // item_of: adjacent slots, a slot's 4 ports 8 workgroups apart = one XCD (today)
       MAP_IDENT,          // adjacent slots, a slot's ports on 4 consecutive workgroups = 4 XCDs
       MAP_FAR_XCD,        // item_of's blocks of 32 workgroups (8 slots) transposed K x (1024 / K): consecutive blocks 1024 / K blocks apart
       MAP_FAR_IDENT,      // the same with the ports spread over XCDs
       MAP_FAR_SLOT };     // item_of's deal, then the slots transposed K x (8192 / K): a block's 8 slots 8192 / K slots apart
// rot: start chunk phi of the item's 91 chunks, written (c + phi) mod 91
enum { ROT_NONE = 0, ROT_ITEM, ROT_ITEM11, ROT_SLOT23, ROT_XCD, ROT_XCDWG };
struct Order { const char* name; int map, k, rot, backodd, halves; };

__host__ __device__ inline int item_for(int b, int map, int k) {
  const int per = 8 * N_PORTS;
  if (map == MAP_FAR_XCD || map == MAP_FAR_IDENT) {  // 1024 blocks of 32 workgroups, transposed k x (1024 / k)
    const int g = b / per, j = b - g * per, ng = N_ITEMS / per;
    b = ((g % k) * (ng / k) + g / k) * per + j;
  }
  if (map == MAP_XCD || map == MAP_FAR_XCD || map == MAP_FAR_SLOT) {
    const int g = b / per, j = b - g * per;
    int slot = g * 8 + (j & 7);
    if (map == MAP_FAR_SLOT) slot = (slot % k) * (N_SLOTS / k) + slot / k;
    return slot * N_PORTS + (j >> 3);
  }
  return b;
}
__host__ __device__ inline int phi_for(int b, int item, int rot) {
  switch (rot) {
    case ROT_ITEM: return item % NCH;                 // item-proportional, 1 chunk per item
    case ROT_ITEM11: return (item * 11) % NCH;        // item-proportional, about an eighth of an item per item
    case ROT_SLOT23: return (item / N_PORTS * 23) % NCH;  // slot-proportional: a slot's ports start together
    case ROT_XCD: return (b & 7) * 11;                // the eight XCDs start at eight different eighths
    case ROT_XCDWG: return ((b >> 3) * 11) % NCH;     // inside an XCD, consecutive workgroups an eighth apart
    default: return 0;
  }
}
// chunk written at iteration k (0 <= k < 91)
__host__ __device__ inline int chunk_at(int k, int item, int phi, int backodd, int halves) {
  int c = halves ? ((k & 1) ? (NCH + 1) / 2 + (k >> 1) : (k >> 1)) : k;  // two half-streams, iterations alternate
  c += phi;
  c = c >= NCH ? c - NCH : c;
  return (backodd && (item & 1)) ? NCH - 1 - c : c;
}

template <bool READ>
__global__ __launch_bounds__(256) void storeorder(const float2* __restrict__ rx, const float2* __restrict__ pil, float4* __restrict__ out,
                                                  int map, int k, int rot, int backodd, int halves) {
  extern __shared__ float red[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int item = item_for(b, map, k), slot = item / N_PORTS, phi = phi_for(b, item, rot);
  float v = 1.f;
  if (READ) {  // rwmix<true, true>: the two comb-2 DM-RS rows of the item + the slot's pilots, block-reduced: every store depends on them
    const float2* r = rx + (size_t)item * N_SC * N_SYM;
    float acc = 0.f;
    for (int k = tid; k < N_RE; k += 256) {
      const float2 a = r[2 * N_SC + 2 * k], c = r[11 * N_SC + 2 * k];
      const float2 p = pil[(size_t)slot * N_RE * 2 + k], q = pil[(size_t)slot * N_RE * 2 + N_RE + k];
      acc += a.x * p.x + a.y * p.y + c.x * q.x + c.y * q.y;
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    v = red[0];
  }
  if (tid < ACTIVE) {
    float4* o = out + (size_t)item * (N_SC * ROW4) + tid;
    const float4 val = make_float4(v, v + 1.f, v + 2.f, (float)item);
#pragma unroll 4
    for (int k = 0; k < NCH; ++k) o[chunk_at(k, item, phi, backodd, halves) * ACTIVE] = val;
  }
}
// ceiling: the chip sweeps the buffer front to back (fillpat's pattern G)
__global__ __launch_bounds__(256) void sweep(float4* p, size_t n4) {
  const float4 v = make_float4(1.f, 2.f, 3.f, 4.f);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

static const Order kOrders[] = {
    {"a  today: item_of, chunks 0..90", MAP_XCD, 1, ROT_NONE, 0, 0},
    {"b1 rotate phi = item", MAP_XCD, 1, ROT_ITEM, 0, 0},
    {"b2 rotate phi = 11 item", MAP_XCD, 1, ROT_ITEM11, 0, 0},
    {"b3 rotate phi = 23 slot", MAP_XCD, 1, ROT_SLOT23, 0, 0},
    {"b4 rotate phi = 11 xcd", MAP_XCD, 1, ROT_XCD, 0, 0},
    {"b5 rotate phi = 11 (wg in xcd)", MAP_XCD, 1, ROT_XCDWG, 0, 0},
    {"c1 adjacent slots, ports over XCDs", MAP_IDENT, 1, ROT_NONE, 0, 0},
    {"c2 far slots, ports on one XCD", MAP_FAR_XCD, 64, ROT_NONE, 0, 0},
    {"c3 far slots, ports over XCDs", MAP_FAR_IDENT, 64, ROT_NONE, 0, 0},
    {"d  odd items back to front", MAP_XCD, 1, ROT_NONE, 1, 0},
    {"e  two interleaved half-streams", MAP_XCD, 1, ROT_NONE, 0, 1},
    {"e2 half-streams + phi = 11 xcd", MAP_XCD, 1, ROT_XCD, 0, 1},
    // how far apart: c2's block transpose with K = 2 .. 512 (resident blocks 1024 / K blocks = 1024 / K x 11.7 MB apart)
    {"c2 K=2    (blocks 512 apart)", MAP_FAR_XCD, 2, ROT_NONE, 0, 0},
    {"c2 K=4    (blocks 256 apart)", MAP_FAR_XCD, 4, ROT_NONE, 0, 0},
    {"c2 K=8    (blocks 128 apart)", MAP_FAR_XCD, 8, ROT_NONE, 0, 0},
    {"c2 K=16   (blocks 64 apart)", MAP_FAR_XCD, 16, ROT_NONE, 0, 0},
    {"c2 K=32   (blocks 32 apart)", MAP_FAR_XCD, 32, ROT_NONE, 0, 0},
    {"c2 K=128  (blocks 8 apart)", MAP_FAR_XCD, 128, ROT_NONE, 0, 0},
    {"c2 K=256  (blocks 4 apart)", MAP_FAR_XCD, 256, ROT_NONE, 0, 0},
    {"c2 K=512  (blocks 2 apart)", MAP_FAR_XCD, 512, ROT_NONE, 0, 0},
    // the same at slot granularity: a block's 8 slots (one per XCD) 8192 / K slots apart
    {"s  K=512  (slots 16 apart)", MAP_FAR_SLOT, 512, ROT_NONE, 0, 0},
    {"s  K=128  (slots 64 apart)", MAP_FAR_SLOT, 128, ROT_NONE, 0, 0},
    {"s  K=64   (slots 128 apart)", MAP_FAR_SLOT, 64, ROT_NONE, 0, 0},
    {"s  K=16   (slots 512 apart)", MAP_FAR_SLOT, 16, ROT_NONE, 0, 0},
    {"s  K=32   (slots 256 apart)", MAP_FAR_SLOT, 32, ROT_NONE, 0, 0},
    {"s  K=8    (each XCD its own eighth)", MAP_FAR_SLOT, 8, ROT_NONE, 0, 0},
    {"s  K=4    (slots 2048 apart)", MAP_FAR_SLOT, 4, ROT_NONE, 0, 0},
    {"s  K=2    (slots 4096 apart)", MAP_FAR_SLOT, 2, ROT_NONE, 0, 0},
};
constexpr int N_ORD = sizeof(kOrders) / sizeof(kOrders[0]);

// every order: the item map is a permutation of the items, and every item's chunk sequence a permutation of 0..90
static bool check_orders() {
  std::vector<unsigned char> seen(N_ITEMS);
  for (const Order& o : kOrders) {
    memset(seen.data(), 0, seen.size());
    for (int b = 0; b < N_ITEMS; ++b) {
      const int it = item_for(b, o.map, o.k);
      if (it < 0 || it >= N_ITEMS || seen[it]++) { printf("%s: item map is not a permutation (b %d -> %d)\n", o.name, b, it); return false; }
      unsigned char ch[NCH] = {};
      const int phi = phi_for(b, it, o.rot);
      for (int k = 0; k < NCH; ++k) {
        const int c = chunk_at(k, it, phi, o.backodd, o.halves);
        if (c < 0 || c >= NCH || ch[c]++) { printf("%s: chunk order of item %d is not a permutation\n", o.name, it); return false; }
      }
    }
  }
  return true;
}

template <typename F> double time_ms(F f, int iters) {
  hipEvent_t a, b; CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
  f(); f();
  CHECK(hipEventRecord(a));
  for (int i = 0; i < iters; ++i) f();
  CHECK(hipEventRecord(b)); CHECK(hipEventSynchronize(b));
  CHECK(hipGetLastError());
  float ms; CHECK(hipEventElapsedTime(&ms, a, b));
  CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(b));
  return ms / iters;
}

int main() {
  if (!check_orders()) return 1;
  hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
  printf("# device %s (%s), %d CUs; %d items x %d B, %d chunks of %d B, %d KB LDS per workgroup\n", prop.name, prop.gcnArchName,
         prop.multiProcessorCount, N_ITEMS, N_SC * ROW4 * 16, NCH, ACTIVE * 16, LDS_PAD / 1024);
  const size_t out_bytes = (size_t)N_ITEMS * N_SC * ROW4 * 16, rx_bytes = (size_t)N_ITEMS * N_SC * N_SYM * 8, pil_bytes = (size_t)N_SLOTS * N_RE * 2 * 8;
  float2 *rx, *pil; float4* out;
  CHECK(hipMalloc(&rx, rx_bytes)); CHECK(hipMalloc(&pil, pil_bytes)); CHECK(hipMalloc(&out, out_bytes));
  CHECK(hipMemset(rx, 0, rx_bytes)); CHECK(hipMemset(pil, 0, pil_bytes));
  CHECK(hipFuncSetAttribute((const void*)storeorder<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_PAD));
  CHECK(hipFuncSetAttribute((const void*)storeorder<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_PAD));
  const int ITERS = 20, PASSES = 3;
  double w[PASSES][N_ORD], rw[PASSES][N_ORD], g[PASSES][2];
  for (int pass = 0; pass < PASSES; ++pass) {
    printf("## pass %d (ms per launch: mean of %d launches after two warm-up launches)\n", pass + 1, ITERS);
    for (int i = 0; i < 2; ++i) {
      const int nwg = i ? 768 : 256;
      g[pass][i] = time_ms([&] { sweep<<<nwg, 256>>>(out, out_bytes / 16); }, ITERS);
      printf("G sweep, %3d workgroups            write only %.3f ms %5.0f GB/s\n", nwg, g[pass][i], out_bytes / g[pass][i] / 1e6);
    }
    for (int o = 0; o < N_ORD; ++o) {
      const Order& d = kOrders[o];
      w[pass][o] = time_ms([&] { storeorder<false><<<N_ITEMS, 256, LDS_PAD>>>(rx, pil, out, d.map, d.k, d.rot, d.backodd, d.halves); }, ITERS);
      rw[pass][o] = time_ms([&] { storeorder<true><<<N_ITEMS, 256, LDS_PAD>>>(rx, pil, out, d.map, d.k, d.rot, d.backodd, d.halves); }, ITERS);
      printf("%-34s write only %.3f ms %5.0f GB/s   read then write %.3f ms\n", d.name, w[pass][o], out_bytes / w[pass][o] / 1e6, rw[pass][o]);
    }
  }
  printf("## gain over (a) per pass, read then write | write only (positive = faster); gate: >= 4 %% read then write in all passes\n");
  bool any = false;
  for (int o = 1; o < N_ORD; ++o) {
    double mn = 1e9;
    printf("%-34s", kOrders[o].name);
    for (int p = 0; p < PASSES; ++p) { const double x = 100.0 * (rw[p][0] / rw[p][o] - 1.0); mn = x < mn ? x : mn; printf(" %+5.1f", x); }
    printf("  |");
    for (int p = 0; p < PASSES; ++p) printf(" %+5.1f", 100.0 * (w[p][0] / w[p][o] - 1.0));
    printf("   min %+5.1f %%%s\n", mn, mn >= 4.0 ? "  PASSES THE GATE" : "");
    any |= mn >= 4.0;
  }
  printf("G sweep over (a) write only:");
  for (int p = 0; p < PASSES; ++p) printf("  %+5.1f / %+5.1f %%", 100.0 * (w[p][0] / g[p][0] - 1.0), 100.0 * (w[p][0] / g[p][1] - 1.0));
  printf("  (256 / 768 workgroups)\ngate: %s\n", any ? "an order passes" : "no order passes");
  CHECK(hipFree(rx)); CHECK(hipFree(pil)); CHECK(hipFree(out));
  return 0;
}

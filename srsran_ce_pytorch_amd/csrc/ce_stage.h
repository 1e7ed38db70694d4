// What the stages around the estimator (ce_dmrs, ce_eq, ce_demod, ce_rm, ce_denoise) share on the host: the steps of plan
// creation and of a launch that do not depend on the stage.  Plain functions, called where the stage's own code was.
// What two stages derive alike has a header of its own: ce_remap.h (the data-RE map), ce_ratematch.h (rate matching),
// ce_segment.h, ce_gold.h, ce_crc.h, ce_fft.h.
#pragma once
#include <memory>
#include <new>

#include "ce_plan.h"

// A default-constructed plan, or null (the caller reports CE_ERR_NOMEM).
template <class Plan>
std::unique_ptr<Plan> ce_new_plan() {
  return std::unique_ptr<Plan>(new (std::nothrow) Plan);
}

// The next link of a plan's `hipError_t` chain: allocates *dst on the current device and copies `bytes` of host memory
// into it; does nothing once the chain holds an error.  *dst stays the plan's to free either way.
template <class T>
hipError_t ce_upload(hipError_t e, T** dst, const void* src, size_t bytes) {
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(dst), bytes);
  if (e == hipSuccess) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  return e;
}

// A CeDeviceScope that could not make the plan's device current.
inline int ce_device_fail(int device, hipError_t e) { return ce_fail(CE_ERR_HIP, "device %d: %s", device, hipGetErrorString(e)); }

// After hipLaunchKernelGGL: CE_OK, or the launch error as "<what> launch: ...".
inline int ce_launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CE_OK : ce_fail(CE_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
}

// Rows of samples [slot][port][>= len] addressed by two strides in elements (ce_ofdm.hip, ce_chan.hip), non-empty batch.
// The workgroup count of a launch with wg_per_item workgroups per (slot, port), into *n_wg: at most 2^31 - 1.
inline int ce_rows_workgroups(int64_t n_slots, int64_t n_ports, int64_t wg_per_item, int64_t* n_wg) {
  const int64_t lim = 0x7FFFFFFFll;
  if (n_slots > lim || n_ports > lim || wg_per_item > lim || n_slots * n_ports > lim / wg_per_item)
    return ce_fail(CE_ERR_UNSUPPORTED, "%lld slots x %lld ports of %lld workgroups: more than 2^31-1 workgroups in one launch", (long long)n_slots,
                   (long long)n_ports, (long long)wg_per_item);
  *n_wg = n_slots * n_ports * wg_per_item;
  return CE_OK;
}

// The extent of the strided tensor, in bytes, stays inside 64 bits (n_slots, n_ports < 2^31).
inline int ce_rows_extent(int64_t n_slots, int64_t n_ports, int64_t slot_stride, int64_t port_stride) {
  const int64_t room = INT64_MAX >> 6;
  if (slot_stride > room / n_slots || port_stride > room / n_ports)
    return ce_fail(CE_ERR_INVALID, "slot_stride=%lld and port_stride=%lld: the extent of %lld slots x %lld ports exceeds the address space",
                   (long long)slot_stride, (long long)port_stride, (long long)n_slots, (long long)n_ports);
  return CE_OK;
}

// Every sample of the rows of `len` samples is written by one workgroup only: the rows pairwise disjoint, the ports inside a
// slot or the slots inside a port (one continuous stream per port).
inline int ce_rows_disjoint(int64_t n_slots, int64_t n_ports, int64_t slot_stride, int64_t port_stride, int64_t len) {
  const bool port_inner = (n_ports == 1 || port_stride >= len) && (n_slots == 1 || slot_stride >= (n_ports - 1) * port_stride + len);
  const bool slot_inner = (n_slots == 1 || slot_stride >= len) && (n_ports == 1 || port_stride >= (n_slots - 1) * slot_stride + len);
  if (!port_inner && !slot_inner)
    return ce_fail(CE_ERR_INVALID, "slot_stride=%lld and port_stride=%lld: the rows of %lld samples of %lld slots x %lld ports overlap",
                   (long long)slot_stride, (long long)port_stride, (long long)len, (long long)n_slots, (long long)n_ports);
  return CE_OK;
}

// *_plan_get_info of a plan that keeps its info block in `info`.
template <class Plan, class Info>
int ce_get_info(const Plan* p, Info* info) {
  if (!p || !info) return ce_fail(CE_ERR_INVALID, "null argument");
  *info = p->info;
  return CE_OK;
}

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

// *_plan_get_info of a plan that keeps its info block in `info`.
template <class Plan, class Info>
int ce_get_info(const Plan* p, Info* info) {
  if (!p || !info) return ce_fail(CE_ERR_INVALID, "null argument");
  *info = p->info;
  return CE_OK;
}

// pgm_hip_common.h — what the HIP units (pgmhip.hip, pgmrows.hip, pgmfit.hip, pgmsample.hip, pgmgibbs.hip,
// pgmpm.cpp) share: the HIP error check of a C-ABI entry point and the stream cast; and for the plan handles of the
// last three the HIP side of pgm_plan_dev.h and the flagged launch.  The one error string lives in
// pgmhip.hip (pgmi_failf); the host-only plan units (pgmprim_plan.cpp with plan_contract among them) include
// none of this and report through pgmi_failf alone.
#pragma once
#include <hip/hip_runtime.h>

#include "pgmhip.h"
#include "pgm_internal.h"
#include "pgm_plan_dev.h"

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      (void)hipGetLastError();                                                                 \
      return pgmi_failf(e_ == hipErrorOutOfMemory ? PGM_ENOMEM : PGM_EDEVICE, "%s: %s", #expr, \
                        hipGetErrorString(e_));                                                \
    }                                                                                          \
  } while (0)

static inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }

// ---------------------------------------------------------------------------- a plan handle's device side
static inline int pgm_dev_current(int *device) {
  HIP_TRY(hipGetDevice(device));
  return PGM_OK;
}
static inline int pgm_dev_alloc(void **p, size_t bytes) {
  HIP_TRY(hipMalloc(p, bytes));
  return PGM_OK;
}
static inline int pgm_dev_copy(void *dst, const void *src, size_t bytes) {
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return PGM_OK;
}
static inline void pgm_dev_free(void *p) { (void)hipFree(p); }
static constexpr pgmdev::DevOps kHipDevOps = {pgm_dev_current, pgm_dev_alloc, pgm_dev_copy, pgm_dev_free};

// the pgm_*_plan_destroy of a handle type H with a PlanDev member `dev`
template <class H>
static inline int pgm_plan_destroy(void *plan) {
  if (!plan) return PGM_OK;
  H *h = static_cast<H *>(plan);
  h->dev.release(kHipDevOps);
  delete h;
  return PGM_OK;
}

// ---------------------------------------------------------------------------- the flagged launch
// A kernel that meets an input it must not index with raises bits in the handle's flag word, and the
// entry point turns them into its own status: flag_reset on the stream, the launch(es), flag_read.
static inline int flag_reset(const pgmdev::PlanDev &dev, void *stream) {
  HIP_TRY(hipMemsetAsync(dev.flag(), 0, sizeof(int32_t), S(stream)));
  return PGM_OK;
}
// the launch's own error, then the bits the kernels raised; synchronises the stream
static inline int flag_read(const pgmdev::PlanDev &dev, void *stream, int32_t *bits) {
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(bits, dev.flag(), sizeof *bits, hipMemcpyDeviceToHost, S(stream)));
  HIP_TRY(hipStreamSynchronize(S(stream)));
  return PGM_OK;
}
// One uint8 per family / column from the caller's pageable host array (modes, clamp), between flag_reset
// and the launch: staged into the handle's buffer before the call returns, ordered with the launch on the
// stream.  *on_device is what the kernel takes: nullptr when src is null or all zero (all free / none
// clamped), so no copy is made.
static inline int stage_bytes(uint8_t *buf, const uint8_t *src, size_t n, void *stream, const uint8_t **on_device) {
  *on_device = nullptr;
  bool any = false;
  for (size_t i = 0; src && i < n; ++i) any |= src[i] != 0;
  if (!any) return PGM_OK;
  HIP_TRY(hipMemcpyAsync(buf, src, n, hipMemcpyHostToDevice, S(stream)));
  *on_device = buf;
  return PGM_OK;
}

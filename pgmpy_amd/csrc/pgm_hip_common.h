// pgm_hip_common.h — what the HIP units (pgmhip.hip, pgmrows.hip) share: the HIP error check of a
// C-ABI entry point and the stream cast.  The one error string lives in pgmhip.hip (pgmi_failf).
#pragma once
#include <hip/hip_runtime.h>

#include "pgmhip.h"
#include "pgm_internal.h"

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

// pgm_lgs.h — private interface between the two units of the Gaussian structure learning calls
// (include/pgmhip.h "Gaussian structure learning"): pgmlgs_plan.cpp (host only: validation of a job batch,
// the buckets, the argument checks of pgm_lgs_pcorr / pgm_lgs_score) and pgmlgs.hip (k_lgs_lane, k_lgs_wave,
// the device side of the handle, the launches).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_LGS_LOCAL __attribute__((visibility("hidden")))

static constexpr int kLgsMaxCond = PGM_LGS_MAX_COND;
static constexpr int kLgsLaneMax = PGM_LGS_LANE_MAX;
static constexpr int kLgsMaxTargets = PGM_LGS_MAX_TARGETS;
static constexpr int kLgsBlock = 64;  // work-items of a workgroup of either path: one wave
// a pivot of the unit-diagonal conditioning block at or below this drops its column (models/_lg.py RCOND)
static constexpr double kLgsRcond = 1e-11;

// jobs of one (|K|, n_targets): order[first .. first + count) are their indices, ascending
struct LgsBucket {
  int32_t k, t, first, count;
};

struct PGM_LGS_LOCAL LgsPlan {
  std::vector<int32_t> job_off, job_cols;  // job j: job_cols[job_off[j] .. job_off[j + 1]), K first, then the targets
  std::vector<int32_t> order;              // the jobs bucket by bucket
  std::vector<LgsBucket> buckets;          // ascending (k, t)
  std::vector<uint8_t> has_ones;           // per job: K holds the ones column d
  std::vector<uint8_t> last_is_ones;       // per job: its last target is the ones column d
  int32_t n_jobs = 0, d = 0, max_cond = 0;
  int64_t n_lane_jobs = 0, n_wave_jobs = 0;
};

struct PGM_LGS_LOCAL LgsHandle {
  LgsPlan p;
  pgmdev::PlanDev dev;
  const int32_t *d_job_off = nullptr;
  const int32_t *d_job_cols = nullptr;
  const int32_t *d_order = nullptr;
};

PGM_LGS_LOCAL int lgs_plan_build(const int32_t *job_off, const int32_t *job_cols, const int32_t *n_targets, int32_t n_jobs,
                                 int32_t d, LgsPlan &out);
// the checks of the two calls (no HIP call); *launch: whether there is anything to launch
PGM_LGS_LOCAL int lgs_pcorr_check(const LgsHandle *h, const double *G, const double *shift, int32_t d, int32_t intercept,
                                  const double *coef, const double *pvalue, const int32_t *rank, bool *launch);
PGM_LGS_LOCAL int lgs_score_check(const LgsHandle *h, const double *G, const double *shift, int32_t d, int32_t kind,
                                  const double *score, const double *rss, const int32_t *rank, bool *launch);
// doubles of LDS a wave-path job of |K| = k with t targets takes
static inline size_t lgs_wave_lds_doubles(int32_t k, int32_t t) {
  const size_t m = (size_t)k + (size_t)t;
  return m * (m | 1) + 3 * m;
}

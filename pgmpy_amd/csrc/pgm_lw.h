// pgm_lw.h — private interface between the two units of the likelihood-weighted posterior
// (pgm_sample_posterior): pgmlw_plan.cpp (host only: launch geometry, the argument checks, the host-only
// query) and pgmlw.hip (the fused sample / weight / histogram kernels and the launches).  Builds on the
// sampler's plan and stream (pgm_sample.h) and the fit plan's families (pgm_fit.h).  Not part of
// include/pgmhip.h.
#pragma once
#include <cstdint>

#include "pgm_sample.h"

static constexpr int kLwChunk = PGM_LW_CHUNK;
static constexpr int kLwMaxBlock = 256;
static constexpr int kLwMaxGroups = PGM_LW_MAX_GROUPS;
static constexpr int64_t kLwMaxSamples = PGM_LW_MAX_SAMPLES;
static constexpr int32_t kLwLdsBudget = PGM_LW_LDS_BUDGET;
// the reductions' corner of LDS: one fp64 per work-item of the largest workgroup (later three uint64 sums)
static constexpr int32_t kLwRedBytes = kLwMaxBlock * 8;
static_assert(kLwMaxSamples / kLwChunk <= kLwMaxGroups, "one row's chunks fit one launch");

// dynamic LDS: [the uint64 tile, accumulating launch only][the reductions][codes: n_cols x block bytes]
static constexpr int64_t lw_lds_bytes(int64_t n_cols, int64_t total_bins, int32_t block, bool tile) {
  return (tile ? 8 * total_bins : 0) + kLwRedBytes + n_cols * block;
}

struct LwGeometry {
  int32_t block, k, lds_bytes, n_cols;
  int64_t total_bins, chunks, rows_per_launch;
};

// the geometry of a call; what: the entry point's name.  PGM_EINVAL when n_samples or block is out of
// range or no workgroup size fits the LDS budget
PGM_FIT_LOCAL int lw_geometry(const char *what, const SampleHandle *h, const FitHandle *t, int64_t n_samples,
                              int32_t block, LwGeometry *g);
// the argument checks of pgm_sample_posterior (no HIP call)
PGM_FIT_LOCAL int sample_posterior_check(const SampleHandle *h, const FitHandle *t, const double *values,
                                         const double *cdf, const uint8_t *modes, const uint8_t *evidence,
                                         int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int64_t n_samples,
                                         int64_t first_row, int32_t block, const void *acc, const void *scale,
                                         const void *post, const void *log_evidence, const void *ess, LwGeometry *g);

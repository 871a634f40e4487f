// pgm_sample.h — private interface between the two units of forward sampling: pgmsample_plan.cpp (host
// only: family validation on top of the fit plan's layout, the argument checks of the pgm_sample_* entry
// points) and pgmsample.hip (the running-sum and sampling kernels, the device side of the handle, the
// launches); and the counter-based random stream both sides and the host self-test compile.  Not part of
// include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_fit.h"
#include "pgmhip.h"

#if defined(__HIPCC__)
#define PGM_HD __host__ __device__ inline
#else
#define PGM_HD inline
#endif

// Launch geometry of the sampling kernel: a workgroup of kSampleBlock work-items draws kSampleRowsPerBlock
// consecutive rows; on the four-rows-per-lane path that is one dword of codes per lane and column.
static constexpr int kSampleBlock = 256;
static constexpr int kSampleRowsPerBlock = 1024;

// ---------------------------------------------------------------------------- the random stream
// Philox4x32-10 (Salmon et al., SC'11).  One call per (stream row, column pair): counter
// (row & 0xffffffff, row >> 32, column >> 1, 0), key (seed & 0xffffffff, seed >> 32).
PGM_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t x[4]) {
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// The uniform of stream row `chain`, code column `col` and sweep `sweep`: 53 bits in [0, 1); columns 2k and
// 2k + 1 share a call.  The sweep, the fourth counter word, is for samplers that revisit a column (Gibbs):
// 1 <= sweep < 2^32.  Sweep 0 is the forward sampler's stream (sample_uniform), so the state "after sweep 0"
// is the forward-sampled state of the same seed and no uniform is used twice.
PGM_HD double sample_uniform3(uint64_t seed, uint64_t chain, uint32_t col, uint32_t sweep) {
  uint32_t x[4];
  philox4x32_10((uint32_t)chain, (uint32_t)(chain >> 32), col >> 1, sweep, (uint32_t)seed, (uint32_t)(seed >> 32), x);
  const uint32_t hi = col & 1u ? x[2] : x[0], lo = col & 1u ? x[3] : x[1];
  return (double)(((uint64_t)hi << 21) | (lo >> 11)) * 0x1.0p-53;
}
PGM_HD double sample_uniform(uint64_t seed, uint64_t row, uint32_t col) { return sample_uniform3(seed, row, col, 0u); }

// The state a uniform selects in one CPD column: c is the column's running sums (entry k at c[k * ncol]).
// With t = u * total the state is min{k : c_k > t}; if u * total rounded up to the total there is none, and
// it is the first state that reaches the total.  Shared by pgm_sample_forward and pgm_sample_posterior.
PGM_HD int32_t sample_select(const double *c, int32_t card, int64_t ncol, double u) {
  const double total = c[(int64_t)(card - 1) * ncol];
  const double t = u * total;
  int32_t k = 0;
  while (k < card && !(c[(int64_t)k * ncol] > t)) ++k;
  if (k == card) {  // u * total rounded up to the total: the first state that reaches it
    k = 0;
    while (k < card - 1 && !(c[(int64_t)k * ncol] == total)) ++k;
  }
  return k;
}

// ---------------------------------------------------------------------------- the plan
// the families of a fit plan (same descriptors, same flat table layout) given in a topological order
struct PGM_FIT_LOCAL SamplePlan {
  FitPlan fit;
};

// the handle behind pgm_sample_plan_create: the plan plus its lazily uploaded device copy (dev owns what
// the d_* point to and sets them: pgmsample.hip sample_use)
struct PGM_FIT_LOCAL SampleHandle {
  SamplePlan p;
  pgmdev::PlanDev dev;
  const FitFam *d_fams = nullptr;
  const int64_t *d_col_off = nullptr;
  uint8_t *d_modes = nullptr;  // the staging buffer of a call's modes: one byte per family
  // the posterior stage (pgmlw.hip): one fp64 maximum per (row, chunk) workgroup, three uint64 sums per row
  double *d_lw_max = nullptr;
  unsigned long long *d_lw_sums = nullptr;
};

// The descriptors and the modes' staging buffer on the current device, and with kSamplePosterior what only
// pgm_sample_posterior needs (pgmsample.hip; pgmlw.hip shares it).
enum { kSampleNoStage = -1, kSamplePosterior = 0 };
PGM_FIT_LOCAL int sample_use(SampleHandle *h, int stage = kSampleNoStage);

// validate the families (fit_plan_build's layout + the sampler's ordering rules); PGM_OK, or PGM_EINVAL
// with pgm_last_error set
PGM_FIT_LOCAL int sample_plan_build(const pgm_fit_family *fams, int32_t n, SamplePlan &out);
PGM_FIT_LOCAL int sample_cdf_check(const SampleHandle *h, const double *values, const double *cdf);
// the argument checks of pgm_sample_forward (no HIP call); *blocks: workgroups of the launch
PGM_FIT_LOCAL int sample_forward_check(const SampleHandle *h, const double *values, const double *cdf,
                                       const uint8_t *modes, const uint8_t *codes, int32_t n_cols, int64_t ld,
                                       int64_t row0, int64_t n_rows, int64_t first_row, const double *weights,
                                       int64_t *blocks);

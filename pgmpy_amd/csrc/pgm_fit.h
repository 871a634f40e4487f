// pgm_fit.h — private interface between the two units of parameter learning: pgmfit_plan.cpp (host only:
// family validation, table layout, grouping of families per workgroup, the argument checks of the
// pgm_fit_* entry points), pgmfit.hip (the counting and finishing kernels, the device side of the
// handle, the launches) and pgmlogp.hip (the per-row log-probability kernels); at the end, the host checks the sampling units share with it.  Not part of
// include/pgmhip.h.
#pragma once
#include <cstdint>
#include <new>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

// internal to the library: not in its dynamic symbol table
#define PGM_FIT_LOCAL __attribute__((visibility("hidden")))

// Launch geometry of the counting kernel.  A workgroup of kFitBlock work-items takes kFitRowsPerBlock
// rows for one group of families whose count tables, laid end to end, fill at most kFitTileBins bins of
// LDS: 4,096 uint32 bins are 16 KiB, so the 8 workgroups of 256 that fill a CU's 32 wave slots take
// 128 KiB of its 160 KiB (the fp64 bins of the weighted kernel take 32 KiB: 5 workgroups, 20 waves per
// CU).  A workgroup adds at most kFitRowsPerBlock to a bin, so a uint32 bin cannot wrap.
static constexpr int kFitBlock = 256;
static constexpr int kFitTileBins = 4096;
static constexpr int kFitRowsPerBlock = 4096;
// The score kernel: one workgroup of kScoreChunk work-items per chunk of kScoreChunk CPD columns of one
// family, chunks counted from the family's own column 0 (so a family's partial sums do not depend on
// the families around it); the second launch sums a family's chunk partials with kScoreSumBlock work-items.
static constexpr int kScoreChunk = PGM_SCORE_CHUNK;
static constexpr int kScoreSumBlock = 64;
// The CI-test kernels (pgm_fit_citest): one workgroup of kCiChunk work-items per chunk of kCiChunk strata
// (Z configurations) of one test, chunks counted from the test's own stratum 0.  A table with
// rx + ry <= kCiSmall (every table up to 8 x 8) takes one work-item per stratum with its marginals in LDS:
// kCiSmall int64 per work-item, 16 KiB, plus 2 KiB for the tree: 18 KiB per workgroup, so 8 workgroups (16
// waves) share a CU's 160 KiB, which is also what the kernel's registers allow (4 waves per SIMD).
// Small tests without Z (one stratum) are packed kCiChunk to a workgroup instead of one workgroup each.
static constexpr int kCiChunk = PGM_CI_CHUNK;
static constexpr int kCiSmall = 16;
// The log-probability kernel (pgm_fit_logprob): a workgroup of kLogpBlock work-items takes kLogpRowsPerBlock
// consecutive rows, one dword of four codes per lane and column on the four-rows-per-lane path, and leaves
// one fp64 partial and one int32 count of skipped rows; the second launch adds the partials with one
// workgroup of kLogpBlock.  The handle keeps kLogpMaxBlocks partials (768 KiB), built by the first call.
static constexpr int kLogpBlock = PGM_LOGP_BLOCK;
static constexpr int kLogpRowsPerBlock = PGM_LOGP_ROWS_PER_BLOCK;
static constexpr int kLogpMaxBlocks = PGM_LOGP_MAX_BLOCKS;
static_assert(kLogpRowsPerBlock == 4 * kLogpBlock, "a lane owns four rows of its workgroup");

// one family as the kernels read it (device memory; every field is workgroup-uniform: scalar loads)
struct FitFam {
  int64_t off;                   // first bin of the table in the flat count buffer
  int32_t size, n_vars;          // bins = product of the cardinalities; 1 + parents
  int32_t col[PGM_MAX_DIMS];     // code column of the node, then of each parent
  int32_t card[PGM_MAX_DIMS];
  int32_t stride[PGM_MAX_DIMS];  // the CPD's layout [node][parents in C order]: last parent fastest
};
// consecutive families one workgroup counts together: their tables are one contiguous run of bins
struct FitGroup {
  int64_t off;                 // first bin of the run
  int32_t fam_begin, fam_end;  // families [fam_begin, fam_end)
  int32_t bins;                // bins of the run (<= kFitTileBins unless global)
  int32_t global;              // 1: a single family larger than the tile, counted straight into global memory
};
static_assert(sizeof(FitFam) % 8 == 0 && sizeof(FitGroup) == 24, "descriptor packing");

// a validated set of families: everything the kernels need, before anything touches a device
struct PGM_FIT_LOCAL FitPlan {
  std::vector<FitFam> fams;
  std::vector<FitGroup> groups;
  std::vector<int32_t> group_of;  // group of each family
  std::vector<int64_t> col_off;   // first CPD column (parent configuration) of each family, + the total
  std::vector<int64_t> chunk_off;  // first score chunk (kScoreChunk columns) of each family, + the total
  // the CI-test work lists: a family (X, Y, Z...) has qz = size / (rx ry) strata in ceil(qz / kCiChunk) chunks
  std::vector<int64_t> ci_off;        // first chunk partial of each family, + the total
  std::vector<int64_t> ci_multi_off;  // first workgroup of each family in the chunk launch (packed families: none)
  std::vector<int32_t> ci_single;     // the packed families: qz = 1 and rx + ry <= kCiSmall
  int32_t ci_bad = -1;                // first family with fewer than two variables (no CI test), or -1
  int64_t total_bins = 0;
  int n_cols = 0;  // 1 + the largest code column read
};

// the handle behind pgm_fit_plan_create: the plan plus its lazily uploaded device copy (dev owns what the
// d_* point to and sets them: pgmfit.hip fit_use)
struct PGM_FIT_LOCAL FitHandle {
  FitPlan p;
  pgmdev::PlanDev dev;
  const FitFam *d_fams = nullptr;
  const FitGroup *d_groups = nullptr;
  const int64_t *d_col_off = nullptr;
  // the score stage: chunk_off, and one fp64 partial + one int64 observed-column count per chunk
  const int64_t *d_chunk_off = nullptr;
  double *d_part = nullptr;
  int64_t *d_part_obs = nullptr;
  // the CI stage: the three work lists, and one fp64 statistic + one int64 dof per chunk
  const int64_t *d_ci_off = nullptr, *d_ci_multi_off = nullptr;
  const int32_t *d_ci_single = nullptr;
  double *d_ci_part = nullptr;
  int64_t *d_ci_dof = nullptr;
  // the log-probability stage: one fp64 partial + one int32 count of skipped rows per workgroup
  double *d_logp_part = nullptr;
  int32_t *d_logp_skip = nullptr;
};

// The descriptors on the current device, and with a stage what only the score / CI / log-probability
// launches need (pgmfit.hip; pgmlogp.hip shares it).
enum { kFitNoStage = -1, kFitScore = 0, kFitCi = 1, kFitLogp = 2 };
PGM_FIT_LOCAL int fit_use(FitHandle *h, int stage = kFitNoStage);

// validate the families and lay the tables out; PGM_OK, or PGM_EINVAL with pgm_last_error set
PGM_FIT_LOCAL int fit_plan_build(const pgm_fit_family *fams, int32_t n, FitPlan &out);
// the argument checks of pgm_fit_count / pgm_fit_finish (no HIP call); *blocks: workgroups of the launch
PGM_FIT_LOCAL int fit_count_check(const FitHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                                  int64_t n_rows, const void *tables, int64_t *blocks);
PGM_FIT_LOCAL int fit_finish_check(const FitHandle *h, const void *counts, int32_t mode, const double *values);
// the argument checks of pgm_fit_score (no HIP call); *blocks: workgroups of the chunk launch
PGM_FIT_LOCAL int fit_score_check(const FitHandle *h, const int64_t *counts, int32_t mode, const double *alpha,
                                  const double *beta, const double *scores, int64_t *blocks);
// the argument checks of pgm_fit_citest (no HIP call); *blocks: workgroups of the chunk launch (may be 0)
PGM_FIT_LOCAL int fit_citest_check(const FitHandle *h, const int64_t *counts, double lambda, int32_t flags,
                                   const double *stat, const int64_t *dof, const double *pvalue, int64_t *blocks);
// The latent side of one pgm_fit_estep call, passed to the kernel by value (every field is
// workgroup-uniform: scalar loads from the kernarg segment).  Latent configuration l is the mixed-radix
// number of the latents' states in the order of latent_cols, the last one fastest.
struct EmSpec {
  int32_t n_latent, n_configs;  // L = n_configs = the product of card[]
  int32_t n_lat_fam, n_fam;     // families with a latent in scope; families of the plan
  int32_t col[PGM_EM_MAX_LATENT], card[PGM_EM_MAX_LATENT];
  int32_t fam[PGM_EM_MAX_FAMILIES];                        // the families with a latent, ascending
  int32_t stride[PGM_EM_MAX_FAMILIES][PGM_EM_MAX_LATENT];  // table stride of latent j in fam[k] (0: not in scope)
};
// dynamic LDS of the E-step launch: the fp64 tile, then the [family][work-item] scratch of observed indices
static constexpr int32_t fit_estep_lds(int32_t n_lat_fam) {
  return kFitTileBins * (int32_t)sizeof(double) + n_lat_fam * kFitBlock * (int32_t)sizeof(int32_t);
}
// the latent columns of pgm_fit_estep(_info) against the plan (no HIP call); what: the entry point's name
PGM_FIT_LOCAL int fit_estep_spec(const FitHandle *h, const int32_t *latent_cols, int32_t n_latent, const char *what,
                                 EmSpec *spec, int32_t *n_obs_cols);
// the argument checks of pgm_fit_estep (no HIP call); *blocks: workgroups of the launch
PGM_FIT_LOCAL int fit_estep_check(const FitHandle *h, const int32_t *latent_cols, int32_t n_latent, const double *values,
                                  const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                                  const double *tables, EmSpec *spec, int64_t *blocks);
PGM_FIT_LOCAL int fit_states_check(const FitHandle *h, const int64_t *counts, const int64_t *n_states);
// the argument checks of pgm_fit_log_values (no HIP call); *blocks: workgroups of the launch
PGM_FIT_LOCAL int fit_log_values_check(const FitHandle *h, const double *values, const double *logv, int64_t *blocks);
// the argument checks of pgm_fit_logprob (no HIP call); *blocks: workgroups of the row launch = block partials
PGM_FIT_LOCAL int fit_logprob_check(const FitHandle *h, const double *logv, const uint8_t *codes, int32_t n_cols,
                                    int64_t ld, int64_t row0, int64_t n_rows, const double *logp, const double *total,
                                    const int64_t *n_skipped, int64_t *blocks);

// ---------------------------------------------------------------------------- shared with the other plan units
// (pgmsample_plan.cpp, pgmgibbs_plan.cpp and their .hip units; defined in pgmfit_plan.cpp, which they link)
// whether a launch over a code window takes the four-rows-per-lane kernel: a lane's dword of 4 codes must be
// aligned in every column (codes, ld and row0 multiples of 4); else the one-row kernel runs
PGM_FIT_LOCAL bool codes_vec4(const void *codes, int64_t ld, int64_t row0);
// The window [row0, row0 + n) of a code matrix with ld rows per column, and the stream range [first,
// first + n) it stands for (0 for an entry point without a stream).  what: the entry point's name; noun:
// what it calls a row ("rows", "chains").
PGM_FIT_LOCAL int window_check(const char *what, const char *noun, int64_t ld, int64_t row0, int64_t n, int64_t first);
// the body of a pgm_*_plan_create: a new handle H filled by build(h->p); what: the entry point's name
template <class H, class Build>
int plan_create(const char *what, void **plan, Build build) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "%s: null plan", what);
  *plan = nullptr;
  H *h = new (std::nothrow) H();
  if (!h) return pgmi_failf(PGM_ENOMEM, "%s: out of memory", what);
  const int st = build(h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}
// the per-family offsets / sizes of a pgm_*_plan_info (either may be NULL)
PGM_FIT_LOCAL void plan_info_layout(const FitPlan &p, int64_t *offsets, int64_t *sizes);

// pgm_gibbs.h — private interface between the two units of Gibbs sampling: pgmgibbs_plan.cpp (host only:
// factor validation on top of the fit plan's layout, the incidence lists, the argument checks of the
// pgm_gibbs_* entry points, the choice of the kernel path) and pgmgibbs.hip (the sweep and start kernels,
// the device side of the handle, the launches).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_fit.h"
#include "pgm_sample.h"
#include "pgmhip.h"

// Launch geometry of the sweep kernel: a workgroup of kGibbsBlock work-items owns kGibbsBlock chains, one
// per lane.  On the LDS path the chains' codes live in LDS as [column][lane] bytes for the whole launch:
// n_cols * kGibbsBlock bytes, taken when they fit kGibbsLdsBudget (64 KiB, what a launch may ask for
// without opting in; alarm's 37 columns are 9.25 KiB, so LDS does not bound the occupancy there).
static constexpr int kGibbsBlock = 256;
static constexpr int kGibbsLdsBudget = 64 * 1024;
// cardinalities up to this keep the K weights of a conditional in registers; larger ones recompute them
// in a second pass (the same operations in the same order: the same bits)
static constexpr int kGibbsRegCard = 8;

// one (column, incident factor) pair as the kernel reads it (workgroup-uniform: scalar loads)
struct GibbsInc {
  int64_t off;                     // first entry of the factor's table in the flat values
  int32_t stride;                  // table stride of the column in this factor
  int32_t factor;                  // the factor (ascending within a column's list)
  int32_t other_begin, other_end;  // the factor's other columns: others[other_begin .. other_end)
};
// a column of an incident factor other than the one being drawn
struct GibbsOther {
  int32_t col, stride;
};
static_assert(sizeof(GibbsInc) == 24 && sizeof(GibbsOther) == 8, "descriptor packing");

// a validated set of factors: everything the kernel needs, before anything touches a device
struct PGM_FIT_LOCAL GibbsPlan {
  FitPlan fit;                     // the factors as families: off, size, col, card, stride
  int32_t n_cols = 0;
  std::vector<int32_t> card;       // per column
  std::vector<int32_t> inc_off;    // CSR over columns: inc[inc_off[c] .. inc_off[c + 1])
  std::vector<GibbsInc> inc;
  std::vector<int32_t> inc_pos;    // position of the column in inc[e].factor (the host-side query)
  std::vector<GibbsOther> others;
  int32_t max_degree = 0, max_card = 0;
};

// the handle behind pgm_gibbs_plan_create: the plan plus its lazily uploaded device copy (dev owns what
// the d_* point to and sets them: pgmgibbs.hip gibbs_use)
struct PGM_FIT_LOCAL GibbsHandle {
  GibbsPlan p;
  pgmdev::PlanDev dev;
  const int32_t *d_card = nullptr, *d_inc_off = nullptr;
  const GibbsInc *d_inc = nullptr;
  const GibbsOther *d_others = nullptr;
  uint8_t *d_clamp = nullptr;  // the staging buffer of a call's clamp: one byte per column
};

// validate the factors and build the incidence lists; PGM_OK, or PGM_EINVAL with pgm_last_error set
PGM_FIT_LOCAL int gibbs_plan_build(const pgm_fit_family *factors, int32_t n, const int32_t *card, int32_t n_cols,
                                   GibbsPlan &out);
// whether a launch keeps the chains' codes in LDS (else they stay in the code matrix)
PGM_FIT_LOCAL bool gibbs_lds_path(const GibbsPlan &p);
// the argument checks of pgm_gibbs_sweep (no HIP call); *blocks: workgroups of the launch
PGM_FIT_LOCAL int gibbs_sweep_check(const GibbsHandle *h, const double *values, const uint8_t *codes, int32_t n_cols,
                                    int64_t ld, int64_t row0, int64_t n_chains, int64_t first_chain,
                                    int64_t first_sweep, int64_t n_sweeps, const uint8_t *trace, int64_t ld_trace,
                                    int64_t thin, int64_t *blocks);
// the argument checks of pgm_gibbs_start (no HIP call)
PGM_FIT_LOCAL int gibbs_start_check(const GibbsHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld,
                                    int64_t row0, int64_t n_chains, int64_t first_chain, int64_t *blocks);

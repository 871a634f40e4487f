// pgm_md.h — private interface between the two units of the mirror-descent fit of junction-tree potentials
// (include/pgmhip.h "Junction-tree potentials by mirror descent"): pgmmd_plan.cpp (host only: validation of the
// cliques, the tree and the marginals, the rooted tree and its levels, the reduction jobs and projections of every
// phase of a calibration, the item lists, the offsets, the LDS layout and the tier, the argument checks of pgm_md_run)
// and pgmmd.hip (k_md, the device side of the handle, the launch).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_lbp.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_MD_LOCAL __attribute__((visibility("hidden")))

static constexpr int kMdMaxVars = PGM_MD_MAX_VARS;  // variables of a clique, of a separator, of a marginal
static constexpr int kMdMaxCard = 254;
static constexpr int kMdBlock = kLbpBlock;        // work-items of a workgroup, always: the reductions are laid out on it
static constexpr int64_t kMdLdsMax = kLbpLdsMax;  // the budget of k_lbp
static constexpr int kMdPadBytes = 64;            // the reduction pad: 4 wave values of two quantities
static constexpr int kMdWave = 64;                // a residual of this many cells or more is reduced by a whole wave
static constexpr int kMdTrials = PGM_MD_TRIALS;             // line-search trials of an iteration

// A log-sum-exp reduction of a clique's table onto some of its variables: the up message of an edge (the child's
// table onto the separator), the down message (the parent's table onto the separator) or a marginal (the owner's
// table onto the marginal's scope).  Output cell s = sum d_k * ks[k] over the kept variables (C order of the output)
// starts at table cell tab + sum d_k * kt[k]; residual cell r = sum e_k * rs[k] adds sum e_k * rt[k].
struct alignas(16) MdJob {
  int32_t tab;           // the clique's table in the state
  int32_t out;           // the output's offset in its array (up / down: the separator's; marginal: in a row of targets)
  int32_t n_out, n_res;  // cells of the output; cells of the table per output cell
  int32_t nk, nr;        // kept and residual variables
  int32_t item0;         // the job's first cell in the item list
  int32_t pad;
  int32_t kc[kMdMaxVars], ks[kMdMaxVars], kt[kMdMaxVars];
  int32_t rc[kMdMaxVars], rs[kMdMaxVars], rt[kMdMaxVars];
};
// Table cell x of a clique read as a cell of a smaller array over some of the clique's variables (a message of one of
// its edges, the gradient vector of one of its marginals): off + sum ((x / st[k]) % card[k]) * ss[k].
struct alignas(16) MdProj {
  int32_t off, nv, pad0, pad1;
  int32_t st[kMdMaxVars], card[kMdMaxVars], ss[kMdMaxVars];
};
// every cell of a clique's table takes the sum of the projections [p0, p1)
struct MdAdd {
  int32_t tab, size, p0, p1;
};
enum MdPhaseKind : int32_t { kMdUp = 0, kMdAddUp = 1, kMdLogZ = 2, kMdDown = 3, kMdAddDown = 4, kMdMarg = 5 };
// One step of a calibration, with a workgroup barrier behind it: the reductions of the items [lane0, lane0 + lane_n)
// (one work-item each) and [wave0, wave0 + wave_n) (one wave each), or the additions [a0, a1).
struct MdPhase {
  int32_t kind, a0, a1, lane0, lane_n, wave0, wave_n, pad;
};

struct PGM_MD_LOCAL MdPlan {
  int32_t n_vars = 0, n_cliques = 0, n_edges = 0, n_marginals = 0, depth = 0, tier = 0, forced_tier = 0;
  int64_t n_cells = 0, n_sep = 0, n_y = 0;
  int64_t state_len = 0;  // omega, the trial log-beliefs, the up and the down messages
  int64_t lds_bytes = 0;
  int32_t root_tab = 0, root_size = 0;
  std::vector<int32_t> clique_off;  // [n_cliques + 1]
  std::vector<int32_t> parent, level, owner;
  std::vector<int32_t> sep_off, y_off;  // [n_cliques + 1] by child clique (the root has none); [n_marginals + 1]
  std::vector<MdJob> jobs;          // up jobs by clique, down jobs by clique, then the marginals
  std::vector<MdProj> projs;
  std::vector<MdAdd> adds;          // the gradient gather of every clique first: [0, n_cliques)
  std::vector<MdPhase> phases;
  std::vector<int32_t> items;       // the job of every reduction cell, phase after phase, lane items before wave items
};

struct PGM_MD_LOCAL MdHandle {
  MdPlan p;
  pgmdev::PlanDev dev;
  const MdJob *d_jobs = nullptr;
  const MdProj *d_projs = nullptr;
  const MdAdd *d_adds = nullptr;
  const MdPhase *d_phases = nullptr;
  const int32_t *d_items = nullptr;
};

// The LDS of a workgroup.  PGM_MD_TIER_LDS: omega and the trial log-beliefs [n_cells] each, the up and the down
// messages [n_sep] each, then the per-marginal vectors y, g, nu2, mu2 [n_y] each (all fp64), the pad.
// PGM_MD_TIER_GLOBAL: the vectors and the pad only; the rest is the instance's slice of the scratch slab.
static inline int64_t md_lds_bytes(int32_t tier, int64_t n_cells, int64_t n_sep, int64_t n_y) {
  return 8 * ((tier == PGM_MD_TIER_LDS ? 2 * (n_cells + n_sep) : 0) + 4 * n_y) + kMdPadBytes;
}

PGM_MD_LOCAL int md_plan_build(const int32_t *card, int32_t n_vars, const int32_t *c_nvars, const int32_t *c_vars,
                               int32_t n_cliques, const int32_t *edges, int32_t n_edges, const int32_t *m_nvars,
                               const int32_t *m_vars, int32_t n_marginals, MdPlan &out);
PGM_MD_LOCAL int md_pick_tier(MdPlan &p, int32_t tier);
// the checks of pgm_md_run (no HIP call); *launch: whether there is anything to launch
PGM_MD_LOCAL int md_run_check(const MdHandle *h, const double *targets, const double *totals, const double *theta_in,
                              int64_t theta_rows, int64_t n_rows, int32_t metric, int32_t iterations, double stepsize,
                              int32_t step_mode, const double *scratch, const double *theta_out, const double *mu_out,
                              const double *values, const int32_t *trials, bool *launch);

// pgm_mplp.h — private interface between the two units of max-product linear programming on a Markov network
// (include/pgmhip.h "MAP by max-product linear programming"): pgmmplp_plan.cpp (host only: validation of the
// clusters, the intersection sets, the dependency levels and their work-item lists, the state and LDS layout, the
// argument checks of pgm_mplp_run) and pgmmplp.hip (k_mplp, the device side of the handle, the launch).  Not part
// of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_MPLP_LOCAL __attribute__((visibility("hidden")))

static constexpr int kMplpMaxVars = 3;             // variables of a cluster
static constexpr int kMplpMaxCard = 254;
static constexpr int kMplpBlock = 256;             // work-items of a workgroup, always: the reductions are laid out on it
static constexpr int64_t kMplpLdsMax = 163840 - 256;  // the CU's LDS less a static share of 256 bytes
static constexpr int kMplpPadBytes = 64;           // the reduction pad: 4 wave totals of the dual and of the primal value
static constexpr int kMplpMinStop = 16;            // the convergence test stops a run from iteration index 16 on

// A cluster as the kernel reads it (32 int32, 16-byte aligned).  Set i of the cluster: its objective at sobj[i],
// its message at smsg[i] (state offsets), and the stride of cluster variable j in the set's table at sstr[3 i + j]
// (0: the variable is not in the set).
struct alignas(16) MplpCluster {
  int32_t nv, k, size, off_obj, off_theta;
  int32_t card[3], cstride[3], var[3];
  int32_t sobj[3], smsg[3], sstr[9];
  int32_t pad[3];
};
// One (cluster, intersection set) pair (8 int32)
struct alignas(16) MplpSet {
  int32_t cluster, off_obj, off_msg, off_stage, size;
  int32_t str[3];  // = sstr[3 i ..] of its cluster
};

struct PGM_MPLP_LOCAL MplpPlan {
  int32_t n_nodes = 0, n_clusters = 0, n_triplets = 0, n_sets = 0, n_levels = 0;
  int64_t n_unary = 0, n_theta = 0, n_msg = 0, n_stage = 0;
  int64_t n_tab = 0;        // n_unary + n_theta + n_msg: the tables of the state
  int64_t state_len = 0;    // n_tab + 2 (best primal, dual_lp) + n_nodes (the best codes)
  int64_t lds_bytes = 0;
  int32_t theta_in_lds = 0;
  std::vector<int32_t> node_off;    // [n_nodes + 1]
  std::vector<int32_t> level;       // [n_clusters], from 0
  std::vector<MplpCluster> clusters;
  std::vector<MplpSet> sets;
  std::vector<int32_t> lev_set, lev_cell;   // [n_levels + 1]: the level's items in set_items / cell_items
  std::vector<uint32_t> set_items;  // (set << 16) | cell of the set
  std::vector<uint32_t> cell_items; // (cluster << 16) | cell of the cluster
};

struct PGM_MPLP_LOCAL MplpHandle {
  MplpPlan p;
  pgmdev::PlanDev dev;
  const int32_t *d_node_off = nullptr, *d_lev_set = nullptr, *d_lev_cell = nullptr;
  const MplpCluster *d_clusters = nullptr;
  const MplpSet *d_sets = nullptr;
  const uint32_t *d_set_items = nullptr, *d_cell_items = nullptr;
};

// The LDS of a workgroup, in this order: the state's tables [n_tab], the staging area [n_stage], theta [n_theta]
// when it is kept there (all fp64), the pad, the decoded codes and the best codes [n_nodes] bytes each (rounded up
// to 8).
static inline int64_t mplp_lds_bytes(int64_t n_tab, int64_t n_stage, int64_t n_theta_lds, int32_t n_nodes) {
  return 8 * (n_tab + n_stage + n_theta_lds) + kMplpPadBytes + 2 * (((int64_t)n_nodes + 7) / 8 * 8);
}

PGM_MPLP_LOCAL int mplp_plan_build(const int32_t *card, int32_t n_nodes, const int32_t *cl_nvars, const int32_t *cl_vars,
                                   int32_t n_clusters, int32_t n_triplets, MplpPlan &out);
// the checks of pgm_mplp_run (no HIP call); *launch: whether there is anything to launch
PGM_MPLP_LOCAL int mplp_run_check(const MplpHandle *h, const double *unaries, const double *theta, int64_t n_rows,
                                  int32_t n_iter, double dual_threshold, double gap_threshold, const double *state_in,
                                  const uint8_t *codes, const double *values, const int32_t *iters, const double *state_out,
                                  bool *launch);

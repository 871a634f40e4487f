// pgm_mnpl.h — private interface between the two units of the pseudo-likelihood fit of a Markov network
// (include/pgmhip.h "Pseudo-likelihood of a Markov network"): pgmmnpl_plan.cpp (host only: scope validation on top of
// the Gibbs plan's incidence lists, the blanket families, the digits of a blanket configuration, the part slots, the
// LDS sizing, the argument checks of pgm_mnpl_eval) and pgmmnpl.hip (k_mn_pl, k_mn_pl_gather, the device side of the
// handle, the launch).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_gibbs.h"
#include "pgmhip.h"

static constexpr int kMnplBlock = 256;  // work-items of a workgroup, always: the reduction is laid out on it
static constexpr int64_t kMnplLdsMax = 163840 - 256;  // the CU's LDS less a static share of 256 bytes, as k_lbp
static constexpr int kMnplPadBytes = 64;  // the reduction pad: 4 wave totals, and room to spare
static constexpr int kMnplGatherBlock = 256;

// A node as k_mn_pl reads it (workgroup-uniform).  Its count table n[s, c] is the fit plan's table of the blanket
// family (node, blanket columns ascending): [card][n_cfg] at count_off, the last blanket column fastest in c.
struct MnplNode {
  int64_t count_off;
  int32_t card, n_cfg;
  int32_t n_theta;    // entries of the incident tables, end to end in incidence order
  int32_t theta_lds;  // 1: those tables are staged in LDS behind the residual table
};
// Beside GibbsInc e (the same index): the (factor, member) slot of the parts buffer this node writes, the factor's
// table size, where the table sits in the node's LDS copy, and the blanket columns outside the factor: free[free_begin
// .. free_end), in blanket order.
struct MnplInc {
  int64_t part_off;
  int32_t size, lds_off;
  int32_t free_begin, free_end;
};
// The digit of a blanket column in a configuration c: (c / div) % card.  odig[o] is that of GibbsOther o (the same
// index); free[] lists those of the columns a factor leaves out.
struct MnplDigit {
  int32_t div, card;
};
static_assert(sizeof(MnplNode) == 24 && sizeof(MnplInc) == 24 && sizeof(MnplDigit) == 8, "descriptor packing");

struct PGM_FIT_LOCAL MnplPlan {
  GibbsPlan g;  // the factors as families (theta's flat layout) and the incidence lists: GibbsInc / GibbsOther
  std::vector<MnplNode> nodes;
  std::vector<MnplInc> minc;
  std::vector<MnplDigit> odig, free;
  std::vector<pgm_fit_family> families;  // the blanket family of every node, for pgm_fit_plan_create
  std::vector<int64_t> count_off;        // [n_cols + 1]: the fit plan's offsets of those families
  std::vector<int64_t> fac_off, part_off;  // [n_factors + 1]: a factor's table in theta; its n_vars slots in parts
  std::vector<int64_t> node_lds;         // [n_cols]: LDS bytes a node's workgroup uses
  int64_t n_theta = 0, n_counts = 0, n_parts = 0, lds_bytes = 0;  // lds_bytes: of the launch = the largest node's
  int32_t max_node = 0, theta_lds_nodes = 0;
};

struct PGM_FIT_LOCAL MnplHandle {
  MnplPlan p;
  pgmdev::PlanDev dev;
  const int32_t *d_inc_off = nullptr;
  const GibbsInc *d_inc = nullptr;
  const GibbsOther *d_others = nullptr;
  const MnplNode *d_nodes = nullptr;
  const MnplInc *d_minc = nullptr;
  const MnplDigit *d_odig = nullptr, *d_free = nullptr;
  const int64_t *d_fac_off = nullptr, *d_part_off = nullptr;
  double *d_parts = nullptr, *d_node_val = nullptr;  // scratch: [n_parts], [n_cols]
};

// the LDS of a node's workgroup, in this order: the residual table [card][n_cfg], the incident tables when staged
// (all fp64), the pad
static inline int64_t mnpl_lds_bytes(int64_t resid, int64_t n_theta_lds) { return 8 * (resid + n_theta_lds) + kMnplPadBytes; }

PGM_FIT_LOCAL int mnpl_plan_build(const pgm_fit_family *factors, int32_t n, const int32_t *card, int32_t n_cols,
                                  MnplPlan &out);
// the checks of pgm_mnpl_eval (no HIP call)
PGM_FIT_LOCAL int mnpl_eval_check(const MnplHandle *h, const int64_t *counts, const double *theta, double l2,
                                  const double *value, const double *grad, const double *node_values);

// pgm_lbp.h — private interface between the two units of sum-product loopy belief propagation on a Markov network
// (include/pgmhip.h "Marginals by loopy belief propagation"): pgmlbp_plan.cpp (host only: validation of the factor
// scopes, the (factor, variable) pairs and their message offsets, the per-node incidence lists, the deduplication of
// the factor tables, the LDS layout, the argument checks of pgm_lbp_run) and pgmlbp.hip (k_lbp, the device side of
// the handle, the launch).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_LBP_LOCAL __attribute__((visibility("hidden")))

static constexpr int kLbpMaxVars = 3;  // variables of a factor
static constexpr int kLbpMaxCard = 254;
static constexpr int kLbpBlock = 256;  // work-items of a workgroup, always: the reductions are laid out on it
static constexpr int64_t kLbpLdsMax = 163840 - 256;  // the CU's LDS less a static share of 256 bytes, as k_mplp
static constexpr int kLbpPadBytes = 64;  // the reduction pad: 4 wave values of two quantities

// A (factor f, variable v) pair as the kernel reads it (20 int32, 16-byte aligned).  The message f -> v, the cavity
// v -> f and the unnormalised new message all live at [moff, moff + card) of their arrays.  The factor's other
// variables, in the factor's order: other i has n_i states, stride s_i in the factor's table and its cavity at c_i
// (n_i = 1, s_i = 0 when there is no such variable).
struct alignas(16) LbpPair {
  int32_t moff, card;    // the pair's cells
  int32_t uoff;          // the node's term in a row of unaries
  int32_t csr0, csr1;    // the node's pairs in nbr_moff
  int32_t nv, pos;       // variables of the factor; position of v among them
  int32_t off_th;        // the factor's table: in the LDS copy of the unique tables, or in theta (theta_in_lds = 0)
  int32_t off_out;       // the factor's own offset in theta: where its belief goes
  int32_t sv;            // stride of v in the table
  int32_t n0, s0, c0, n1, s1, c1;
  int32_t pad[4];
};
// a unique table: `size` entries of theta from `src` to the LDS copy at `dst`
struct LbpTable {
  int32_t src, dst, size, pad;
};

struct PGM_LBP_LOCAL LbpPlan {
  int32_t n_nodes = 0, n_factors = 0, n_pairs = 0, n_tables_unique = 0, theta_in_lds = 0;
  int64_t n_unary = 0, n_msg = 0, n_theta = 0, n_theta_unique = 0;
  int64_t state_len = 0;  // n_msg: the messages
  int64_t lds_bytes = 0;
  std::vector<int32_t> node_off;    // [n_nodes + 1]
  std::vector<int32_t> factor_off;  // [n_factors + 1]: the factors' tables in theta
  std::vector<int32_t> node_csr;    // [n_nodes + 1]: the node's pairs in nbr_moff
  std::vector<int32_t> nbr_moff;    // [n_pairs]: moff of the pairs of a node, in factor order
  std::vector<int32_t> item_pair;   // [n_msg]: the pair of a message cell
  std::vector<int32_t> lead;        // [n_factors]: the pair of the factor's first variable
  std::vector<LbpPair> pairs;
  std::vector<LbpTable> tables;     // [n_tables_unique]
};

struct PGM_LBP_LOCAL LbpHandle {
  LbpPlan p;
  pgmdev::PlanDev dev;
  const int32_t *d_node_off = nullptr, *d_node_csr = nullptr, *d_nbr_moff = nullptr, *d_item_pair = nullptr, *d_lead = nullptr;
  const LbpPair *d_pairs = nullptr;
  const LbpTable *d_tables = nullptr;
};

// The LDS of a workgroup, in this order: the node terms [n_unary], the messages, the cavities and the unnormalised
// new messages [n_msg] each, the unique tables [n_theta_lds] when they are kept there (all fp64), the pad.
static inline int64_t lbp_lds_bytes(int64_t n_unary, int64_t n_msg, int64_t n_theta_lds) {
  return 8 * (n_unary + 3 * n_msg + n_theta_lds) + kLbpPadBytes;
}

PGM_LBP_LOCAL int lbp_plan_build(const int32_t *card, int32_t n_nodes, const int32_t *f_nvars, const int32_t *f_vars,
                                 int32_t n_factors, const double *theta, LbpPlan &out);
// the checks of pgm_lbp_run (no HIP call); *launch: whether there is anything to launch
PGM_LBP_LOCAL int lbp_run_check(const LbpHandle *h, const double *unaries, const double *theta, int64_t n_rows,
                                int32_t n_iter, double tol, double damping, const double *state_in,
                                const double *marginals, const double *values, const int32_t *iters,
                                const double *factor_beliefs, const double *state_out, bool *launch);

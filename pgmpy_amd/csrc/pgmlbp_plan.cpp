// pgmlbp_plan.cpp — the host side of loopy belief propagation (include/pgmhip.h "Marginals by loopy belief
// propagation"): validation of the nodes and factor scopes, the (factor, variable) pairs with their message offsets
// and table strides, the incidence list of every node, the deduplication of the factor tables by value, the LDS
// layout and the argument checks of pgm_lbp_run.  No HIP call and no HIP include: ctypes drives all of it without a
// device.  The kernel and the launch are pgmlbp.hip.
#include <algorithm>
#include <cmath>
#include <map>
#include <new>
#include <string>

#include "pgm_lbp.h"

int lbp_plan_build(const int32_t *card, int32_t n_nodes, const int32_t *f_nvars, const int32_t *f_vars, int32_t n_factors,
                   const double *theta, LbpPlan &out) {
  if (n_nodes < 1) return pgmi_failf(PGM_EINVAL, "lbp_plan_create: %d nodes (1 at least)", n_nodes);
  if (!card) return pgmi_failf(PGM_EINVAL, "lbp_plan_create: null card");
  if (n_factors < 0) return pgmi_failf(PGM_EINVAL, "lbp_plan_create: %d factors", n_factors);
  if (n_factors && (!f_nvars || !f_vars)) return pgmi_failf(PGM_EINVAL, "lbp_plan_create: null factors");
  if ((uintptr_t)theta % 8) return pgmi_failf(PGM_EINVAL, "lbp_plan_create: theta is not 8-byte aligned");
  LbpPlan p;
  p.n_nodes = n_nodes, p.n_factors = n_factors;
  for (int32_t v = 0; v < n_nodes; ++v) {
    if (card[v] < 1 || card[v] > kLbpMaxCard)
      return pgmi_failf(PGM_EINVAL, "lbp_plan_create: node %d has cardinality %d (1 .. %d)", v, card[v], kLbpMaxCard);
    p.node_off.push_back((int32_t)p.n_unary);
    p.n_unary += card[v];
    if (lbp_lds_bytes(p.n_unary, 0, 0) > kLbpLdsMax)
      return pgmi_failf(PGM_EINVAL, "lbp_plan_create: the node terms alone need more than the %lld bytes of LDS",
                        (long long)kLbpLdsMax);
  }
  p.node_off.push_back((int32_t)p.n_unary);

  // the pairs in (factor, position) order; the tables in theta one after the other, C order over the factor's variables
  std::vector<int32_t> pair_node;
  for (int32_t f = 0; f < n_factors; ++f) {
    const int32_t nv = f_nvars[f], *vars = f_vars + (size_t)f * kLbpMaxVars;
    if (nv < 1 || nv > kLbpMaxVars)
      return pgmi_failf(PGM_EINVAL, "lbp_plan_create: factor %d has %d variables (1 .. %d)", f, nv, kLbpMaxVars);
    int32_t stride[kLbpMaxVars] = {0, 0, 0};
    int64_t size = 1;
    for (int32_t j = 0; j < nv; ++j) {
      if (vars[j] < 0 || vars[j] >= n_nodes)
        return pgmi_failf(PGM_EINVAL, "lbp_plan_create: factor %d: node %d is out of range (0 .. %d)", f, vars[j], n_nodes - 1);
      for (int32_t m = 0; m < j; ++m)
        if (vars[m] == vars[j]) return pgmi_failf(PGM_EINVAL, "lbp_plan_create: factor %d lists node %d twice", f, vars[j]);
      size *= card[vars[j]];
    }
    for (int32_t j = nv - 1, s = 1; j >= 0; --j) stride[j] = s, s *= card[vars[j]];
    if (p.n_theta + size > INT32_MAX)
      return pgmi_failf(PGM_EINVAL, "lbp_plan_create: the tables up to factor %d have %lld entries (2^31 - 1 at most)", f,
                        (long long)(p.n_theta + size));
    p.factor_off.push_back((int32_t)p.n_theta);
    p.lead.push_back((int32_t)p.pairs.size());
    const int32_t first = (int32_t)p.pairs.size();
    for (int32_t j = 0; j < nv; ++j) {
      LbpPair P = {};
      P.moff = (int32_t)p.n_msg, P.card = card[vars[j]], P.uoff = p.node_off[(size_t)vars[j]];
      P.nv = nv, P.pos = j, P.off_out = (int32_t)p.n_theta, P.sv = stride[j];
      P.n0 = P.n1 = 1;
      p.n_msg += P.card;
      if (lbp_lds_bytes(p.n_unary, p.n_msg, 0) > kLbpLdsMax)
        return pgmi_failf(PGM_EINVAL, "lbp_plan_create: the state up to factor %d needs %lld bytes of LDS (%lld at most)", f,
                          (long long)lbp_lds_bytes(p.n_unary, p.n_msg, 0), (long long)kLbpLdsMax);
      for (int32_t x = 0; x < P.card; ++x) p.item_pair.push_back((int32_t)p.pairs.size());
      p.pairs.push_back(P);
      pair_node.push_back(vars[j]);
    }
    for (int32_t j = 0; j < nv; ++j) {  // the other variables of pair j, in the factor's order
      LbpPair &P = p.pairs[(size_t)(first + j)];
      int32_t k = 0;
      for (int32_t o = 0; o < nv; ++o) {
        if (o == j) continue;
        const LbpPair &O = p.pairs[(size_t)(first + o)];
        if (k++ == 0) P.n0 = O.card, P.s0 = stride[o], P.c0 = O.moff;
        else P.n1 = O.card, P.s1 = stride[o], P.c1 = O.moff;
      }
    }
    p.n_theta += size;
  }
  p.factor_off.push_back((int32_t)p.n_theta);
  p.n_pairs = (int32_t)p.pairs.size();
  p.state_len = p.n_msg;

  // the pairs of every node, in factor order
  std::vector<int32_t> deg((size_t)n_nodes, 0);
  for (int32_t v : pair_node) ++deg[(size_t)v];
  p.node_csr.assign((size_t)n_nodes + 1, 0);
  for (int32_t v = 0; v < n_nodes; ++v) p.node_csr[(size_t)v + 1] = p.node_csr[(size_t)v] + deg[(size_t)v];
  p.nbr_moff.assign((size_t)p.n_pairs, 0);
  std::vector<int32_t> fill(p.node_csr.begin(), p.node_csr.end() - 1);
  for (int32_t q = 0; q < p.n_pairs; ++q) p.nbr_moff[(size_t)fill[(size_t)pair_node[(size_t)q]]++] = p.pairs[(size_t)q].moff;
  for (int32_t q = 0; q < p.n_pairs; ++q)
    p.pairs[(size_t)q].csr0 = p.node_csr[(size_t)pair_node[(size_t)q]], p.pairs[(size_t)q].csr1 = p.node_csr[(size_t)pair_node[(size_t)q] + 1];

  // the unique tables: two factors whose tables hold the same values (bit for bit, as flat arrays) share one;
  // without theta every factor keeps its own
  std::map<std::string, int32_t> seen;
  std::vector<int32_t> table_of((size_t)n_factors, 0);
  for (int32_t f = 0; f < n_factors; ++f) {
    const int32_t off = p.factor_off[(size_t)f], size = p.factor_off[(size_t)f + 1] - off;
    int32_t t = (int32_t)p.tables.size();
    if (theta) {
      const auto at = seen.emplace(std::string(reinterpret_cast<const char *>(theta + off), (size_t)size * 8), t);
      t = at.first->second;
    }
    if (t == (int32_t)p.tables.size()) {
      p.tables.push_back(LbpTable{off, (int32_t)p.n_theta_unique, size, 0});
      p.n_theta_unique += size;
    }
    table_of[(size_t)f] = t;
  }
  p.n_tables_unique = (int32_t)p.tables.size();

  // the LDS: the unique tables join the state there when both fit
  p.theta_in_lds = lbp_lds_bytes(p.n_unary, p.n_msg, p.n_theta_unique) <= kLbpLdsMax;
  p.lds_bytes = lbp_lds_bytes(p.n_unary, p.n_msg, p.theta_in_lds ? p.n_theta_unique : 0);
  for (int32_t f = 0; f < n_factors; ++f) {
    const LbpTable &T = p.tables[(size_t)table_of[(size_t)f]];
    for (int32_t j = 0; j < f_nvars[f]; ++j) p.pairs[(size_t)(p.lead[(size_t)f] + j)].off_th = p.theta_in_lds ? T.dst : T.src;
  }
  out = std::move(p);
  return PGM_OK;
}

int lbp_run_check(const LbpHandle *h, const double *unaries, const double *theta, int64_t n_rows, int32_t n_iter, double tol,
                  double damping, const double *state_in, const double *marginals, const double *values, const int32_t *iters,
                  const double *factor_beliefs, const double *state_out, bool *launch) {
  *launch = false;
  if (!h) return pgmi_failf(PGM_EINVAL, "lbp_run: null plan");
  if (!unaries || (!theta && h->p.n_theta)) return pgmi_failf(PGM_EINVAL, "lbp_run: null unaries / theta");
  if (!marginals || !values || !iters) return pgmi_failf(PGM_EINVAL, "lbp_run: null marginals / values / iters");
  if (n_rows < 0 || n_rows > INT32_MAX) return pgmi_failf(PGM_EINVAL, "lbp_run: %lld instances (0 .. 2^31 - 1)", (long long)n_rows);
  if (n_iter < 0) return pgmi_failf(PGM_EINVAL, "lbp_run: %d iterations", n_iter);
  if (!(tol >= 0.0) || std::isinf(tol)) return pgmi_failf(PGM_EINVAL, "lbp_run: tolerance %g (finite, 0 or more)", tol);
  if (!(damping >= 0.0 && damping < 1.0)) return pgmi_failf(PGM_EINVAL, "lbp_run: damping %g (0 or more, below 1)", damping);
  const void *f64[] = {unaries, theta, state_in, marginals, values, factor_beliefs, state_out};
  for (const void *q : f64)
    if ((uintptr_t)q % 8) return pgmi_failf(PGM_EINVAL, "lbp_run: an fp64 pointer is not 8-byte aligned");
  if ((uintptr_t)iters % 4) return pgmi_failf(PGM_EINVAL, "lbp_run: iters is not 4-byte aligned");
  *launch = n_rows > 0;
  return PGM_OK;
}

extern "C" {

int pgm_lbp_plan_create(const int32_t *card, int32_t n_nodes, const int32_t *factor_nvars, const int32_t *factor_vars,
                        int32_t n_factors, const double *theta, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "lbp_plan_create: null plan");
  *plan = nullptr;
  LbpHandle *h = new (std::nothrow) LbpHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "lbp_plan_create: out of memory");
  const int st = lbp_plan_build(card, n_nodes, factor_nvars, factor_vars, n_factors, theta, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_lbp_plan_info(void *plan, pgm_lbp_info_t *info, int32_t *node_off, int32_t *factor_off, int32_t *msg_off) {
  const LbpHandle *h = static_cast<const LbpHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "lbp_plan_info: null plan");
  const LbpPlan &p = h->p;
  if (info) {
    info->n_nodes = p.n_nodes, info->n_factors = p.n_factors, info->n_pairs = p.n_pairs;
    info->n_tables_unique = p.n_tables_unique, info->theta_in_lds = p.theta_in_lds, info->block = kLbpBlock;
    info->n_unary = p.n_unary, info->n_msg = p.n_msg, info->n_theta = p.n_theta, info->n_theta_unique = p.n_theta_unique;
    info->state_len = p.state_len, info->lds_bytes = p.lds_bytes, info->lds_max = kLbpLdsMax;
  }
  if (node_off) std::copy(p.node_off.begin(), p.node_off.end(), node_off);
  if (factor_off) std::copy(p.factor_off.begin(), p.factor_off.end(), factor_off);
  if (msg_off) {
    for (int32_t q = 0; q < p.n_pairs; ++q) msg_off[q] = p.pairs[(size_t)q].moff;
    msg_off[p.n_pairs] = (int32_t)p.n_msg;
  }
  return PGM_OK;
}
}

// pgmmplp_plan.cpp — the host side of max-product linear programming (include/pgmhip.h "MAP by max-product linear
// programming"): validation of the nodes and clusters, the intersection sets in their fixed order, the dependency
// level of every cluster and the flat work-item lists of every level, the state and LDS layout and the argument
// checks of pgm_mplp_run.  No HIP call and no HIP include: ctypes drives all of it without a device.  The kernel
// and the launch are pgmmplp.hip.
#include <algorithm>
#include <cmath>
#include <new>

#include "pgm_mplp.h"

int mplp_plan_build(const int32_t *card, int32_t n_nodes, const int32_t *cl_nvars, const int32_t *cl_vars,
                    int32_t n_clusters, int32_t n_triplets, MplpPlan &out) {
  if (n_nodes < 1) return pgmi_failf(PGM_EINVAL, "mplp_plan_create: %d nodes (1 at least)", n_nodes);
  if (!card) return pgmi_failf(PGM_EINVAL, "mplp_plan_create: null card");
  if (n_clusters < 0 || n_triplets < 0 || n_triplets > n_clusters)
    return pgmi_failf(PGM_EINVAL, "mplp_plan_create: %d clusters, %d of them triplets", n_clusters, n_triplets);
  if (n_clusters && (!cl_nvars || !cl_vars)) return pgmi_failf(PGM_EINVAL, "mplp_plan_create: null clusters");
  MplpPlan p;
  p.n_nodes = n_nodes, p.n_clusters = n_clusters, p.n_triplets = n_triplets;
  const int64_t most = kMplpLdsMax / 8;  // no state past this many fp64 entries fits: the running totals stay small
  for (int32_t v = 0; v < n_nodes; ++v) {
    if (card[v] < 1 || card[v] > kMplpMaxCard)
      return pgmi_failf(PGM_EINVAL, "mplp_plan_create: node %d has cardinality %d (1 .. %d)", v, card[v], kMplpMaxCard);
    p.node_off.push_back((int32_t)p.n_unary);
    p.n_unary += card[v];
    if (p.n_unary > most)
      return pgmi_failf(PGM_EINVAL, "mplp_plan_create: the node objectives alone need more than the %lld bytes of LDS",
                        (long long)kMplpLdsMax);
  }
  p.node_off.push_back((int32_t)p.n_unary);

  // the clusters: variables, sizes, C-order strides; a node is an intersection set when two factor clusters hold it
  const int32_t n_factor = n_clusters - n_triplets;
  std::vector<int32_t> held((size_t)n_nodes, 0);
  p.clusters.assign((size_t)n_clusters, MplpCluster{});
  for (int32_t c = 0; c < n_clusters; ++c) {
    MplpCluster &C = p.clusters[(size_t)c];
    const int32_t nv = cl_nvars[c], lo = c < n_factor ? 2 : 3;
    if (nv < lo || nv > kMplpMaxVars)
      return pgmi_failf(PGM_EINVAL, "mplp_plan_create: cluster %d has %d variables (%d .. %d)", c, nv, lo, kMplpMaxVars);
    C.nv = nv;
    int64_t size = 1;
    for (int32_t j = 0; j < nv; ++j) {
      const int32_t v = cl_vars[(size_t)c * kMplpMaxVars + j];
      if (v < 0 || v >= n_nodes)
        return pgmi_failf(PGM_EINVAL, "mplp_plan_create: cluster %d: node %d is out of range (0 .. %d)", c, v, n_nodes - 1);
      for (int32_t m = 0; m < j; ++m)
        if (C.var[m] == v) return pgmi_failf(PGM_EINVAL, "mplp_plan_create: cluster %d lists node %d twice", c, v);
      C.var[j] = v, C.card[j] = card[v];
      size *= card[v];
      if (c < n_factor) ++held[(size_t)v];
    }
    for (int32_t j = nv - 1, stride = 1; j >= 0; --j) C.cstride[j] = stride, stride *= C.card[j];
    C.size = (int32_t)size, C.off_theta = (int32_t)p.n_theta, C.off_obj = (int32_t)(p.n_unary + p.n_theta);
    p.n_theta += size;
    if (p.n_unary + p.n_theta > most)
      return pgmi_failf(PGM_EINVAL, "mplp_plan_create: the objectives up to cluster %d need %lld bytes of LDS (%lld at most)", c,
                        (long long)(8 * (p.n_unary + p.n_theta)), (long long)kMplpLdsMax);
  }
  auto same_scope = [&](const MplpCluster &A, int32_t a, int32_t b) {
    return A.nv == 2 && ((A.var[0] == a && A.var[1] == b) || (A.var[0] == b && A.var[1] == a));
  };

  // the sets of a cluster in the order of its variables (a triplet: of the pairs of its variables), the messages
  p.n_msg = 0;
  for (int32_t c = 0; c < n_clusters; ++c) {
    MplpCluster &C = p.clusters[(size_t)c];
    auto add = [&](int32_t off_obj, int32_t size, const int32_t (&str)[3]) {
      MplpSet S = {};
      S.cluster = c, S.off_obj = off_obj, S.size = size;
      S.off_msg = (int32_t)(p.n_unary + p.n_theta + p.n_msg);
      for (int j = 0; j < 3; ++j) S.str[j] = C.sstr[3 * C.k + j] = str[j];
      C.sobj[C.k] = off_obj, C.smsg[C.k] = S.off_msg;
      ++C.k;
      p.n_msg += size;
      p.sets.push_back(S);
    };
    if (c < n_factor) {
      for (int32_t j = 0; j < C.nv; ++j)
        if (held[(size_t)C.var[j]] > 1) {
          int32_t str[3] = {0, 0, 0};
          str[j] = 1;
          add(p.node_off[(size_t)C.var[j]], C.card[j], str);
        }
    } else {
      const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
      for (const auto &pr : pairs) {
        const int32_t a = C.var[pr[0]], b = C.var[pr[1]];
        int32_t e = -1;
        for (int32_t f = 0; f < n_factor && e < 0; ++f)
          if (same_scope(p.clusters[(size_t)f], a, b)) e = f;
        if (e < 0)
          return pgmi_failf(PGM_EINVAL, "mplp_plan_create: triplet %d: no pairwise cluster over nodes %d and %d", c, a, b);
        const MplpCluster &E = p.clusters[(size_t)e];
        int32_t str[3] = {0, 0, 0};
        str[pr[0]] = E.var[0] == a ? E.cstride[0] : E.cstride[1];
        str[pr[1]] = E.var[0] == a ? E.cstride[1] : E.cstride[0];
        add(E.off_obj, E.size, str);
      }
    }
    if (p.n_unary + p.n_theta + p.n_msg > most)
      return pgmi_failf(PGM_EINVAL, "mplp_plan_create: the state up to cluster %d needs %lld bytes of LDS (%lld at most)", c,
                        (long long)(8 * (p.n_unary + p.n_theta + p.n_msg)), (long long)kMplpLdsMax);
  }
  for (int32_t f = 0; f < n_factor; ++f)
    for (int32_t g = 0; g < f; ++g) {
      const MplpCluster &A = p.clusters[(size_t)f], &B = p.clusters[(size_t)g];
      if (A.nv != B.nv) continue;
      int32_t common = 0;
      for (int32_t i = 0; i < A.nv; ++i)
        for (int32_t j = 0; j < B.nv; ++j) common += A.var[i] == B.var[j];
      if (common == A.nv) return pgmi_failf(PGM_EINVAL, "mplp_plan_create: clusters %d and %d have the same scope", g, f);
    }
  p.n_sets = (int32_t)p.sets.size();
  p.n_tab = p.n_unary + p.n_theta + p.n_msg;
  p.state_len = p.n_tab + 2 + n_nodes;

  // the level of a cluster: one past the highest level of an earlier cluster that touches one of its tables (its
  // own objective, the objectives of its sets); a table is named by its state offset
  std::vector<int32_t> last((size_t)(p.n_unary + p.n_theta), -1);
  p.level.assign((size_t)n_clusters, 0);
  for (int32_t c = 0; c < n_clusters; ++c) {
    const MplpCluster &C = p.clusters[(size_t)c];
    int32_t lev = last[(size_t)C.off_obj];
    for (int32_t i = 0; i < C.k; ++i) lev = std::max(lev, last[(size_t)C.sobj[i]]);
    p.level[(size_t)c] = ++lev;
    last[(size_t)C.off_obj] = lev;
    for (int32_t i = 0; i < C.k; ++i) last[(size_t)C.sobj[i]] = lev;
    if (C.k) p.n_levels = std::max(p.n_levels, lev + 1);
  }

  // the items of a level, clusters in model order; the staging offsets restart at every level
  p.lev_set.push_back(0), p.lev_cell.push_back(0);
  for (int32_t lev = 0; lev < p.n_levels; ++lev) {
    int64_t stage = 0;
    size_t s = 0;
    for (int32_t c = 0; c < n_clusters; ++c) {
      const MplpCluster &C = p.clusters[(size_t)c];
      if (C.k && p.level[(size_t)c] == lev) {
        for (int32_t i = 0; i < C.k; ++i) {
          MplpSet &S = p.sets[s + (size_t)i];
          S.off_stage = (int32_t)stage;
          stage += S.size;
          for (int32_t cell = 0; cell < S.size; ++cell) p.set_items.push_back((uint32_t)(s + (size_t)i) << 16 | (uint32_t)cell);
        }
        for (int32_t cell = 0; cell < C.size; ++cell) p.cell_items.push_back((uint32_t)c << 16 | (uint32_t)cell);
      }
      s += (size_t)C.k;
    }
    p.n_stage = std::max(p.n_stage, stage);
    p.lev_set.push_back((int32_t)p.set_items.size()), p.lev_cell.push_back((int32_t)p.cell_items.size());
  }

  // the LDS: theta joins the state there when both fit
  const int64_t base = mplp_lds_bytes(p.n_tab, p.n_stage, 0, n_nodes);
  if (base > kMplpLdsMax)
    return pgmi_failf(PGM_EINVAL, "mplp_plan_create: the state and its staging area need %lld bytes of LDS, %lld at most",
                      (long long)base, (long long)kMplpLdsMax);
  p.theta_in_lds = mplp_lds_bytes(p.n_tab, p.n_stage, p.n_theta, n_nodes) <= kMplpLdsMax;
  p.lds_bytes = p.theta_in_lds ? mplp_lds_bytes(p.n_tab, p.n_stage, p.n_theta, n_nodes) : base;
  out = std::move(p);
  return PGM_OK;
}

int mplp_run_check(const MplpHandle *h, const double *unaries, const double *theta, int64_t n_rows, int32_t n_iter,
                   double dual_threshold, double gap_threshold, const double *state_in, const uint8_t *codes,
                   const double *values, const int32_t *iters, const double *state_out, bool *launch) {
  *launch = false;
  if (!h) return pgmi_failf(PGM_EINVAL, "mplp_run: null plan");
  if (!unaries || !theta) return pgmi_failf(PGM_EINVAL, "mplp_run: null unaries / theta");
  if (!codes || !values || !iters) return pgmi_failf(PGM_EINVAL, "mplp_run: null codes / values / iters");
  if (n_rows < 0 || n_rows > INT32_MAX) return pgmi_failf(PGM_EINVAL, "mplp_run: %lld instances (0 .. 2^31 - 1)", (long long)n_rows);
  if (n_iter < 0) return pgmi_failf(PGM_EINVAL, "mplp_run: %d iterations", n_iter);
  if (!(dual_threshold >= 0.0) || !(gap_threshold >= 0.0) || std::isinf(dual_threshold) || std::isinf(gap_threshold))
    return pgmi_failf(PGM_EINVAL, "mplp_run: thresholds %g / %g (finite, 0 or more)", dual_threshold, gap_threshold);
  const void *f64[] = {unaries, theta, state_in, values, state_out};
  for (const void *q : f64)
    if ((uintptr_t)q % 8) return pgmi_failf(PGM_EINVAL, "mplp_run: an fp64 pointer is not 8-byte aligned");
  if ((uintptr_t)iters % 4) return pgmi_failf(PGM_EINVAL, "mplp_run: iters is not 4-byte aligned");
  *launch = n_rows > 0;
  return PGM_OK;
}

extern "C" {

int pgm_mplp_plan_create(const int32_t *card, int32_t n_nodes, const int32_t *cluster_nvars, const int32_t *cluster_vars,
                         int32_t n_clusters, int32_t n_triplets, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "mplp_plan_create: null plan");
  *plan = nullptr;
  MplpHandle *h = new (std::nothrow) MplpHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "mplp_plan_create: out of memory");
  const int st = mplp_plan_build(card, n_nodes, cluster_nvars, cluster_vars, n_clusters, n_triplets, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_mplp_plan_info(void *plan, pgm_mplp_info_t *info, int32_t *node_off, int32_t *cluster_off, int32_t *set_count,
                       int32_t *level) {
  const MplpHandle *h = static_cast<const MplpHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "mplp_plan_info: null plan");
  const MplpPlan &p = h->p;
  if (info) {
    info->n_nodes = p.n_nodes, info->n_clusters = p.n_clusters, info->n_sets = p.n_sets, info->n_levels = p.n_levels;
    info->theta_in_lds = p.theta_in_lds, info->block = kMplpBlock;
    info->n_unary = p.n_unary, info->n_theta = p.n_theta, info->n_msg = p.n_msg, info->n_stage = p.n_stage;
    info->state_len = p.state_len, info->lds_bytes = p.lds_bytes, info->lds_max = kMplpLdsMax;
  }
  if (node_off) std::copy(p.node_off.begin(), p.node_off.end(), node_off);
  for (int32_t c = 0; c < p.n_clusters; ++c) {
    if (cluster_off) cluster_off[c] = p.clusters[(size_t)c].off_theta;
    if (set_count) set_count[c] = p.clusters[(size_t)c].k;
    if (level) level[c] = p.level[(size_t)c];
  }
  if (cluster_off) cluster_off[p.n_clusters] = (int32_t)p.n_theta;
  return PGM_OK;
}
}

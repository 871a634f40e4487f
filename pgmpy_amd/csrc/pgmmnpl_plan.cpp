// pgmmnpl_plan.cpp — the host side of the pseudo-likelihood fit of a Markov network (include/pgmhip.h
// "Pseudo-likelihood of a Markov network"): scope validation through gibbs_plan_build, whose incidence lists the
// kernel walks, the blanket family of every node and its count offset, the digit of every blanket column in a
// configuration, the (factor, member) slots of the parts buffer, the LDS sizing and the argument checks of
// pgm_mnpl_eval.  No HIP call and no HIP include: ctypes drives all of it without a device.  The kernels and the
// launch are pgmmnpl.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pgm_mnpl.h"

int mnpl_plan_build(const pgm_fit_family *factors, int32_t n, const int32_t *card, int32_t n_cols, MnplPlan &out) {
  if (!factors) return pgmi_fail(PGM_EINVAL, "mnpl_plan_create: null factors");
  if (!card) return pgmi_fail(PGM_EINVAL, "mnpl_plan_create: null cardinalities");
  MnplPlan p;
  const int st = gibbs_plan_build(factors, n, card, n_cols, p.g);
  if (st != PGM_OK) return st;
  const GibbsPlan &g = p.g;
  p.n_theta = g.fit.total_bins;
  if (p.n_theta > INT32_MAX)
    return pgmi_failf(PGM_EINVAL, "mnpl_plan_create: the tables have %lld entries (2^31 - 1 at most)", (long long)p.n_theta);

  // the slots of the parts buffer: factor f has n_vars of its size, member m at part_off[f] + m * size
  for (int32_t f = 0; f < n; ++f) {
    const FitFam &k = g.fit.fams[(size_t)f];
    p.fac_off.push_back(k.off);
    p.part_off.push_back(p.n_parts);
    p.n_parts += (int64_t)k.n_vars * k.size;
  }
  p.fac_off.push_back(p.n_theta);
  p.part_off.push_back(p.n_parts);

  p.minc.assign(g.inc.size(), MnplInc());
  p.odig.assign(g.others.size(), MnplDigit());
  p.nodes.assign((size_t)n_cols, MnplNode());
  p.families.assign((size_t)n_cols, pgm_fit_family());
  p.node_lds.assign((size_t)n_cols, 0);
  std::vector<int32_t> blanket, div, pos((size_t)n_cols, -1);
  for (int32_t i = 0; i < n_cols; ++i) {
    const int32_t e0 = g.inc_off[(size_t)i], e1 = g.inc_off[(size_t)i + 1];
    // the blanket: every other column of an incident factor, ascending
    blanket.clear();
    for (int32_t e = e0; e < e1; ++e)
      for (int32_t o = g.inc[(size_t)e].other_begin; o < g.inc[(size_t)e].other_end; ++o) blanket.push_back(g.others[(size_t)o].col);
    std::sort(blanket.begin(), blanket.end());
    blanket.erase(std::unique(blanket.begin(), blanket.end()), blanket.end());
    const int32_t nb = (int32_t)blanket.size();
    if (1 + nb > PGM_MAX_DIMS)
      return pgmi_failf(PGM_EINVAL, "mnpl_plan_create: node %d has %d blanket columns (%d at most)", i, nb, PGM_MAX_DIMS - 1);
    // the residual table against the LDS of a workgroup, before its size can overflow
    int64_t resid = card[i];
    for (int32_t b = 0; b < nb; ++b) {
      resid *= card[blanket[(size_t)b]];
      if (mnpl_lds_bytes(resid, 0) > kMnplLdsMax) {
        double bytes = 8.0 * card[i];
        for (int32_t c : blanket) bytes *= card[c];
        return pgmi_failf(PGM_EINVAL,
                          "mnpl_plan_create: node %d with %d blanket columns needs a residual table of %.0f bytes, more "
                          "than the %lld bytes of LDS a workgroup may take (there is no global-memory tier)",
                          i, nb, bytes, (long long)(kMnplLdsMax - kMnplPadBytes));
      }
    }
    // the blanket family and the digits of a configuration: the last blanket column fastest
    pgm_fit_family &fam = p.families[(size_t)i];
    memset(&fam, 0, sizeof fam);
    fam.n_vars = 1 + nb, fam.col[0] = i, fam.card[0] = card[i];
    div.assign((size_t)nb, 1);
    for (int32_t b = nb - 1, s = 1; b >= 0; --b) {
      const int32_t c = blanket[(size_t)b];
      fam.col[1 + b] = c, fam.card[1 + b] = card[c];
      div[(size_t)b] = s, s *= card[c];
      pos[(size_t)c] = b;
    }
    MnplNode &nd = p.nodes[(size_t)i];
    nd.card = card[i], nd.n_cfg = (int32_t)(resid / card[i]), nd.count_off = p.n_counts;
    p.count_off.push_back(p.n_counts);
    p.n_counts += resid;

    std::vector<char> in_factor((size_t)nb);
    for (int32_t e = e0; e < e1; ++e) {
      const GibbsInc &I = g.inc[(size_t)e];
      const FitFam &k = g.fit.fams[(size_t)I.factor];
      MnplInc &M = p.minc[(size_t)e];
      M.part_off = p.part_off[(size_t)I.factor] + (int64_t)g.inc_pos[(size_t)e] * k.size;
      M.size = k.size, M.lds_off = nd.n_theta;
      nd.n_theta += k.size;
      std::fill(in_factor.begin(), in_factor.end(), 0);
      for (int32_t o = I.other_begin; o < I.other_end; ++o) {
        const int32_t b = pos[(size_t)g.others[(size_t)o].col];
        p.odig[(size_t)o] = MnplDigit{div[(size_t)b], card[blanket[(size_t)b]]};
        in_factor[(size_t)b] = 1;
      }
      M.free_begin = (int32_t)p.free.size();
      for (int32_t b = 0; b < nb; ++b)
        if (!in_factor[(size_t)b]) p.free.push_back(MnplDigit{div[(size_t)b], card[blanket[(size_t)b]]});
      M.free_end = (int32_t)p.free.size();
    }
    // the incident tables join the residual table in LDS when both fit
    nd.theta_lds = mnpl_lds_bytes(resid, nd.n_theta) <= kMnplLdsMax;
    p.theta_lds_nodes += nd.theta_lds;
    p.node_lds[(size_t)i] = mnpl_lds_bytes(resid, nd.theta_lds ? nd.n_theta : 0);
    if (p.node_lds[(size_t)i] > p.lds_bytes) p.lds_bytes = p.node_lds[(size_t)i], p.max_node = i;
  }
  p.count_off.push_back(p.n_counts);
  out = std::move(p);
  return PGM_OK;
}

int mnpl_eval_check(const MnplHandle *h, const int64_t *counts, const double *theta, double l2, const double *value,
                    const double *grad, const double *node_values) {
  if (!h) return pgmi_fail(PGM_EINVAL, "mnpl_eval: null plan");
  if (!counts || !theta) return pgmi_fail(PGM_EINVAL, "mnpl_eval: null counts / theta");
  if (!value) return pgmi_fail(PGM_EINVAL, "mnpl_eval: null value");
  if (!(l2 >= 0.0) || std::isinf(l2)) return pgmi_failf(PGM_EINVAL, "mnpl_eval: l2 %g (finite, 0 or more)", l2);
  const void *q64[] = {counts, theta, value, grad, node_values};
  for (const void *q : q64)
    if ((uintptr_t)q % 8) return pgmi_fail(PGM_EINVAL, "mnpl_eval: a pointer is not 8-byte aligned");
  return PGM_OK;
}

extern "C" {

int pgm_mnpl_plan_create(const pgm_fit_family *factors, int32_t n_factors, const int32_t *card, int32_t n_cols,
                         void **plan) {
  return plan_create<MnplHandle>("mnpl_plan_create", plan,
                                 [&](MnplPlan &p) { return mnpl_plan_build(factors, n_factors, card, n_cols, p); });
}

int pgm_mnpl_plan_info(void *plan, pgm_mnpl_info_t *info, pgm_fit_family *families, int64_t *count_off,
                       int64_t *fac_off, int64_t *part_off, int64_t *node_lds, int64_t *slots) {
  if (!plan) return pgmi_fail(PGM_EINVAL, "mnpl_plan_info: null plan");
  const MnplPlan &p = static_cast<const MnplHandle *>(plan)->p;
  if (info) {
    memset(info, 0, sizeof *info);
    info->n_nodes = p.g.n_cols, info->n_factors = (int32_t)p.g.fit.fams.size();
    info->n_incidences = (int32_t)p.g.inc.size(), info->block = kMnplBlock;
    info->max_node = p.max_node, info->max_degree = p.families[(size_t)p.max_node].n_vars - 1;
    info->theta_lds_nodes = p.theta_lds_nodes;
    info->n_theta = p.n_theta, info->n_counts = p.n_counts, info->n_parts = p.n_parts;
    info->lds_bytes = p.lds_bytes, info->lds_max = kMnplLdsMax;
  }
  if (families) std::copy(p.families.begin(), p.families.end(), families);
  if (count_off) std::copy(p.count_off.begin(), p.count_off.end(), count_off);
  if (fac_off) std::copy(p.fac_off.begin(), p.fac_off.end(), fac_off);
  if (part_off) std::copy(p.part_off.begin(), p.part_off.end(), part_off);
  if (node_lds) std::copy(p.node_lds.begin(), p.node_lds.end(), node_lds);
  if (slots)
    for (size_t e = 0; e < p.g.inc.size(); ++e)
      slots[3 * e] = p.g.inc[e].factor, slots[3 * e + 1] = p.g.inc_pos[e], slots[3 * e + 2] = p.minc[e].part_off;
  return PGM_OK;
}
}

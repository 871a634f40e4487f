// pgmgibbs_plan.cpp — the host side of Gibbs sampling (pgmpy_amd.sampling.GibbsSampling): factor
// validation (the fit plan's flat table layout plus the rules of a Gibbs sweep), the per-column lists of
// incident factors, the argument checks of the pgm_gibbs_* entry points and the host-only queries.  No HIP
// include: this unit is tested on the CPU on its own (tools/gibbs_plan_selftest.cpp, linked with
// pgmfit_plan.cpp).  The kernels and launches are pgmgibbs.hip.
#include <cstring>

#include "pgm_gibbs.h"
#include "pgm_internal.h"

static constexpr int kGibbsMaxCard = PGM_EV_MISSING - 1;  // 254: a uint8 code, 255 is PGM_EV_MISSING

int gibbs_plan_build(const pgm_fit_family *factors, int32_t n, const int32_t *card, int32_t n_cols, GibbsPlan &out) {
  if (!factors) return pgmi_fail(PGM_EINVAL, "gibbs_plan_create: null factors");
  if (!card) return pgmi_fail(PGM_EINVAL, "gibbs_plan_create: null cardinalities");
  if (n <= 0) return pgmi_failf(PGM_EINVAL, "gibbs_plan_create: %d factors", n);
  if (n_cols <= 0) return pgmi_failf(PGM_EINVAL, "gibbs_plan_create: %d columns", n_cols);
  for (int32_t c = 0; c < n_cols; ++c)
    if (card[c] <= 0 || card[c] > kGibbsMaxCard)
      return pgmi_failf(PGM_EINVAL, "gibbs_plan_create: column %d cardinality %d (1 .. %d)", c, card[c], kGibbsMaxCard);
  std::vector<int32_t> degree((size_t)n_cols, 0);
  std::vector<int32_t> seen((size_t)n_cols, -1);  // the last factor that listed the column
  int64_t n_others = 0;
  for (int32_t f = 0; f < n; ++f) {
    const pgm_fit_family &in = factors[f];
    if (in.n_vars < 1 || in.n_vars > PGM_MAX_DIMS)
      return pgmi_failf(PGM_EINVAL, "gibbs_plan_create: factor %d has %d columns (1 .. %d)", f, in.n_vars, PGM_MAX_DIMS);
    for (int v = 0; v < in.n_vars; ++v) {
      const int32_t c = in.col[v];
      if (c < 0 || c >= n_cols)
        return pgmi_failf(PGM_EINVAL, "gibbs_plan_create: factor %d position %d column %d (0 .. %d)", f, v, c, n_cols - 1);
      if (in.card[v] != card[c])
        return pgmi_failf(PGM_EINVAL, "gibbs_plan_create: factor %d column %d cardinality %d, the column has %d", f, c,
                          in.card[v], card[c]);
      if (seen[(size_t)c] == f)
        return pgmi_failf(PGM_EINVAL, "gibbs_plan_create: factor %d lists column %d twice", f, c);
      seen[(size_t)c] = f;
      ++degree[(size_t)c];
    }
    n_others += (int64_t)in.n_vars * (in.n_vars - 1);
  }
  for (int32_t c = 0; c < n_cols; ++c)
    if (degree[(size_t)c] == 0) return pgmi_failf(PGM_EINVAL, "gibbs_plan_create: column %d is in no factor", c);
  // the flat table layout (off, stride) and the table size limit
  const int st = fit_plan_build(factors, n, out.fit);
  if (st != PGM_OK) return st;
  out.n_cols = n_cols;
  out.card.assign(card, card + n_cols);
  out.inc_off.assign((size_t)n_cols + 1, 0);
  out.max_degree = out.max_card = 0;
  for (int32_t c = 0; c < n_cols; ++c) {
    out.inc_off[(size_t)c + 1] = out.inc_off[(size_t)c] + degree[(size_t)c];
    if (degree[(size_t)c] > out.max_degree) out.max_degree = degree[(size_t)c];
    if (card[c] > out.max_card) out.max_card = card[c];
  }
  out.inc.assign((size_t)out.inc_off.back(), GibbsInc());
  out.inc_pos.assign((size_t)out.inc_off.back(), 0);
  out.others.clear();
  out.others.reserve((size_t)n_others);
  std::vector<int32_t> fill(out.inc_off.begin(), out.inc_off.end() - 1);
  for (int32_t f = 0; f < n; ++f) {  // factors ascending within every column's list
    const FitFam &k = out.fit.fams[(size_t)f];
    for (int v = 0; v < k.n_vars; ++v) {
      const int32_t e = fill[(size_t)k.col[v]]++;
      GibbsInc &I = out.inc[(size_t)e];
      I.off = k.off, I.stride = k.stride[v], I.factor = f;
      I.other_begin = (int32_t)out.others.size();
      for (int o = 0; o < k.n_vars; ++o)
        if (o != v) out.others.push_back(GibbsOther{k.col[o], k.stride[o]});
      I.other_end = (int32_t)out.others.size();
      out.inc_pos[(size_t)e] = v;
    }
  }
  return PGM_OK;
}

bool gibbs_lds_path(const GibbsPlan &p) { return (int64_t)p.n_cols * kGibbsBlock <= kGibbsLdsBudget; }

static int gibbs_window_check(const char *what, const GibbsHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld,
                              int64_t row0, int64_t n_chains, int64_t first_chain, int64_t *blocks) {
  if (!h) return pgmi_failf(PGM_EINVAL, "%s: null plan", what);
  if (!codes) return pgmi_failf(PGM_EINVAL, "%s: null codes", what);
  const int st = window_check(what, "chains", ld, row0, n_chains, first_chain);
  if (st != PGM_OK) return st;
  if (n_cols < h->p.n_cols)
    return pgmi_failf(PGM_EINVAL, "%s: the plan has %d columns, codes has %d", what, h->p.n_cols, n_cols);
  const int64_t nb = (n_chains + kGibbsBlock - 1) / kGibbsBlock;
  if (nb > INT32_MAX)
    return pgmi_failf(PGM_EINVAL, "%s: %lld workgroups (advance the chains in several calls)", what, (long long)nb);
  if (blocks) *blocks = nb;
  return PGM_OK;
}

int gibbs_sweep_check(const GibbsHandle *h, const double *values, const uint8_t *codes, int32_t n_cols, int64_t ld,
                      int64_t row0, int64_t n_chains, int64_t first_chain, int64_t first_sweep, int64_t n_sweeps,
                      const uint8_t *trace, int64_t ld_trace, int64_t thin, int64_t *blocks) {
  if (h && !values) return pgmi_fail(PGM_EINVAL, "gibbs_sweep: null values");
  const int st = gibbs_window_check("gibbs_sweep", h, codes, n_cols, ld, row0, n_chains, first_chain, blocks);
  if (st != PGM_OK) return st;
  // the sweep is the fourth counter word of the stream: 1 .. 2^32 - 1 (0 is the forward sampler's)
  if (n_sweeps < 0 || first_sweep < 1 || first_sweep > (int64_t)UINT32_MAX || n_sweeps > (int64_t)UINT32_MAX - first_sweep + 1)
    return pgmi_failf(PGM_EINVAL, "gibbs_sweep: sweeps [%lld, + %lld) outside 1 .. 2^32 - 1", (long long)first_sweep,
                      (long long)n_sweeps);
  if (thin < 1) return pgmi_failf(PGM_EINVAL, "gibbs_sweep: thin %lld", (long long)thin);
  if (trace) {
    const int64_t records = n_sweeps / thin;
    if (ld_trace < 0 || (n_chains > 0 && records > ld_trace / n_chains))
      return pgmi_failf(PGM_EINVAL, "gibbs_sweep: %lld records of %lld chains exceed ld_trace %lld", (long long)records,
                        (long long)n_chains, (long long)ld_trace);
  }
  if (n_sweeps == 0 && blocks) *blocks = 0;
  return PGM_OK;
}

int gibbs_start_check(const GibbsHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                      int64_t n_chains, int64_t first_chain, int64_t *blocks) {
  return gibbs_window_check("gibbs_start", h, codes, n_cols, ld, row0, n_chains, first_chain, blocks);
}

extern "C" {

int pgm_gibbs_plan_create(const pgm_fit_family *factors, int32_t n_factors, const int32_t *card, int32_t n_cols,
                          void **plan) {
  return plan_create<GibbsHandle>("gibbs_plan_create", plan,
                                  [&](GibbsPlan &p) { return gibbs_plan_build(factors, n_factors, card, n_cols, p); });
}

int pgm_gibbs_plan_info(void *plan, int64_t n_chains, pgm_gibbs_info_t *info, int64_t *offsets, int64_t *sizes,
                        int32_t *inc_off, int32_t *inc) {
  if (!plan) return pgmi_fail(PGM_EINVAL, "gibbs_plan_info: null plan");
  if (n_chains < 0) return pgmi_failf(PGM_EINVAL, "gibbs_plan_info: n_chains %lld", (long long)n_chains);
  const GibbsPlan &p = static_cast<const GibbsHandle *>(plan)->p;
  if (info) {
    memset(info, 0, sizeof *info);
    const bool lds = gibbs_lds_path(p);
    info->n_factors = (int32_t)p.fit.fams.size();
    info->n_cols = p.n_cols;
    info->total_entries = p.fit.total_bins;
    info->total_incidences = (int64_t)p.inc.size();
    info->blocks = (n_chains + kGibbsBlock - 1) / kGibbsBlock;
    info->max_degree = p.max_degree;
    info->max_card = p.max_card;
    info->path = lds ? PGM_GIBBS_LDS : PGM_GIBBS_GLOBAL;
    info->block = kGibbsBlock;
    info->lds_bytes = lds ? p.n_cols * kGibbsBlock : 0;
    info->lds_budget = kGibbsLdsBudget;
    info->reg_card = kGibbsRegCard;
  }
  plan_info_layout(p.fit, offsets, sizes);
  if (inc_off) memcpy(inc_off, p.inc_off.data(), p.inc_off.size() * sizeof(int32_t));
  if (inc)
    for (size_t e = 0; e < p.inc.size(); ++e) inc[2 * e] = p.inc[e].factor, inc[2 * e + 1] = p.inc_pos[e];
  return PGM_OK;
}
}

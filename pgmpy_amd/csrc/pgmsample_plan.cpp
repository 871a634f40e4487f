// pgmsample_plan.cpp — the host side of forward sampling (pgmpy_amd.sampling, DiscreteBayesianNetwork.simulate):
// family validation (the fit plan's layout plus the sampler's ordering rules), the argument checks of the
// pgm_sample_* entry points and the host-only queries.  No HIP include: this unit is tested on the CPU on
// its own (tools/sample_plan_selftest.cpp, linked with pgmfit_plan.cpp).  The kernels and launches are
// pgmsample.hip.
#include <cstring>
#include <map>

#include "pgm_internal.h"
#include "pgm_sample.h"

int sample_plan_build(const pgm_fit_family *fams, int32_t n, SamplePlan &out) {
  if (!fams) return pgmi_fail(PGM_EINVAL, "sample_plan_create: null families");
  if (n <= 0) return pgmi_failf(PGM_EINVAL, "sample_plan_create: %d families", n);
  std::map<int32_t, int32_t> node_of;  // code column -> the family whose node it is
  for (int32_t f = 0; f < n; ++f) {
    const pgm_fit_family &in = fams[f];
    if (in.n_vars < 1 || in.n_vars > PGM_MAX_DIMS)
      return pgmi_failf(PGM_EINVAL, "sample_plan_create: family %d has %d variables (1 .. %d)", f, in.n_vars,
                        PGM_MAX_DIMS);
    for (int v = 0; v < in.n_vars; ++v) {
      // uint8 codes: states 0 .. 254, 255 is PGM_EV_MISSING
      if (in.card[v] <= 0 || in.card[v] > PGM_EV_MISSING)
        return pgmi_failf(PGM_EINVAL, "sample_plan_create: family %d variable %d cardinality %d (1 .. %d)", f, v,
                          in.card[v], PGM_EV_MISSING);
      if (in.col[v] < 0)
        return pgmi_failf(PGM_EINVAL, "sample_plan_create: family %d variable %d column %d", f, v, in.col[v]);
    }
    // a topological order: every parent was drawn by an earlier family, with the cardinality it has there
    for (int v = 1; v < in.n_vars; ++v) {
      const auto it = node_of.find(in.col[v]);
      if (it == node_of.end())
        return pgmi_failf(PGM_EINVAL, "sample_plan_create: family %d parent column %d is not the node of an earlier family",
                          f, in.col[v]);
      if (fams[it->second].card[0] != in.card[v])
        return pgmi_failf(PGM_EINVAL, "sample_plan_create: family %d parent column %d cardinality %d, its own family %d has %d",
                          f, in.col[v], in.card[v], it->second, fams[it->second].card[0]);
    }
    if (!node_of.emplace(in.col[0], f).second)
      return pgmi_failf(PGM_EINVAL, "sample_plan_create: column %d is the node of families %d and %d", in.col[0],
                        node_of[in.col[0]], f);
  }
  return fit_plan_build(fams, n, out.fit);  // the flat table layout (and the table size limit)
}

int sample_cdf_check(const SampleHandle *h, const double *values, const double *cdf) {
  if (!h) return pgmi_fail(PGM_EINVAL, "sample_cdf: null plan");
  if (!values) return pgmi_fail(PGM_EINVAL, "sample_cdf: null values");
  if (!cdf) return pgmi_fail(PGM_EINVAL, "sample_cdf: null cdf");
  if ((h->p.fit.col_off.back() + 255) / 256 > INT32_MAX)
    return pgmi_fail(PGM_EINVAL, "sample_cdf: too many CPD columns for one launch");
  return PGM_OK;
}

int sample_forward_check(const SampleHandle *h, const double *values, const double *cdf, const uint8_t *modes,
                         const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                         int64_t first_row, const double *weights, int64_t *blocks) {
  if (!h) return pgmi_fail(PGM_EINVAL, "sample_forward: null plan");
  if (!cdf) return pgmi_fail(PGM_EINVAL, "sample_forward: null cdf");
  if (!codes) return pgmi_fail(PGM_EINVAL, "sample_forward: null codes");
  if (weights && !values) return pgmi_fail(PGM_EINVAL, "sample_forward: weights need the values");
  const int st = window_check("sample_forward", "rows", ld, row0, n_rows, first_row);
  if (st != PGM_OK) return st;
  if (n_cols < h->p.fit.n_cols)
    return pgmi_failf(PGM_EINVAL, "sample_forward: the plan writes column %d, codes has %d columns", h->p.fit.n_cols - 1,
                      n_cols);
  if (modes)
    for (size_t f = 0; f < h->p.fit.fams.size(); ++f)
      if (modes[f] > PGM_SAMPLE_OBSERVED)
        return pgmi_failf(PGM_EINVAL, "sample_forward: family %d mode %d", (int)f, (int)modes[f]);
  const int64_t nb = (n_rows + kSampleRowsPerBlock - 1) / kSampleRowsPerBlock;
  if (nb > INT32_MAX)
    return pgmi_failf(PGM_EINVAL, "sample_forward: %lld workgroups (draw the rows in several calls)", (long long)nb);
  if (blocks) *blocks = nb;
  return PGM_OK;
}

extern "C" {

int pgm_sample_plan_create(const pgm_fit_family *fams, int32_t n, void **plan) {
  return plan_create<SampleHandle>("sample_plan_create", plan, [&](SamplePlan &p) { return sample_plan_build(fams, n, p); });
}

int pgm_sample_plan_info(void *plan, const void *codes, int64_t ld, int64_t row0, const void *weights,
                         const void *uniforms, pgm_sample_info_t *info, int64_t *offsets, int64_t *sizes) {
  if (!plan) return pgmi_fail(PGM_EINVAL, "sample_plan_info: null plan");
  const FitPlan &p = static_cast<const SampleHandle *>(plan)->p.fit;
  if (info) {
    memset(info, 0, sizeof *info);
    info->n_families = (int32_t)p.fams.size();
    info->n_cols = p.n_cols;
    info->block = kSampleBlock;
    info->rows_per_block = kSampleRowsPerBlock;
    info->total_bins = p.total_bins;
    info->total_columns = p.col_off.back();
    info->vec4 = codes && codes_vec4(codes, ld, row0) ? 1 : 0;
    info->weighted = weights ? 1 : 0;
    info->explicit_uniforms = uniforms ? 1 : 0;
  }
  plan_info_layout(p, offsets, sizes);
  return PGM_OK;
}
}

// pgmfit_plan.cpp — the host side of parameter learning (DiscreteBayesianNetwork.fit): family validation,
// the layout of the flat count buffer, the grouping of families per workgroup and the argument checks
// of the pgm_fit_* entry points.  No HIP include: this unit is tested on the CPU on its own
// (tools/fit_plan_selftest.cpp).  The kernels and launches are pgmfit.hip.
#include <cmath>
#include <cstring>

#include "pgm_fit.h"
#include "pgm_internal.h"

int fit_plan_build(const pgm_fit_family *fams, int32_t n, FitPlan &out) {
  if (!fams) return pgmi_fail(PGM_EINVAL, "fit_plan_create: null families");
  if (n <= 0) return pgmi_failf(PGM_EINVAL, "fit_plan_create: %d families", n);
  out = FitPlan();
  out.fams.resize((size_t)n);
  out.group_of.resize((size_t)n);
  out.col_off.resize((size_t)n + 1);
  out.chunk_off.resize((size_t)n + 1);
  out.ci_off.resize((size_t)n + 1);
  out.ci_multi_off.resize((size_t)n + 1);
  int64_t off = 0, cols = 0, chunks = 0, ci_chunks = 0, ci_blocks = 0;
  for (int32_t f = 0; f < n; ++f) {
    const pgm_fit_family &in = fams[f];
    // the node and up to PGM_MAX_DIMS - 1 parents
    if (in.n_vars < 1 || in.n_vars > PGM_MAX_DIMS)
      return pgmi_failf(PGM_EINVAL, "fit_plan_create: family %d has %d variables (1 .. %d)", f, in.n_vars,
                        PGM_MAX_DIMS);
    FitFam &k = out.fams[(size_t)f];
    memset(&k, 0, sizeof k);
    k.n_vars = in.n_vars;
    int64_t size = 1;
    for (int v = in.n_vars - 1; v >= 0; --v) {
      // uint8 codes: states 0 .. 254, 255 is PGM_EV_MISSING
      if (in.card[v] <= 0 || in.card[v] > PGM_EV_MISSING)
        return pgmi_failf(PGM_EINVAL, "fit_plan_create: family %d variable %d cardinality %d (1 .. %d)", f, v,
                          in.card[v], PGM_EV_MISSING);
      if (in.col[v] < 0) return pgmi_failf(PGM_EINVAL, "fit_plan_create: family %d variable %d column %d", f, v, in.col[v]);
      k.col[v] = in.col[v];
      k.card[v] = in.card[v];
      // the CPD's layout: the node outermost, then the parents in C order
      k.stride[v] = (int32_t)size;
      size *= in.card[v];
      if (size > INT32_MAX)
        return pgmi_failf(PGM_EINVAL, "fit_plan_create: family %d table exceeds 2^31 - 1 bins", f);
      if (in.col[v] + 1 > out.n_cols) out.n_cols = in.col[v] + 1;
    }
    k.size = (int32_t)size;
    k.off = off;
    out.col_off[(size_t)f] = cols;
    off += size;
    cols += size / in.card[0];
    // the score kernel's work list: (family, chunk) for every kScoreChunk columns of the family
    out.chunk_off[(size_t)f] = chunks;
    chunks += (size / in.card[0] + kScoreChunk - 1) / kScoreChunk;
    // the CI work lists: a packed family has a partial of its own but no workgroup in the chunk launch
    out.ci_off[(size_t)f] = ci_chunks;
    out.ci_multi_off[(size_t)f] = ci_blocks;
    if (in.n_vars < 2) {
      if (out.ci_bad < 0) out.ci_bad = f;
    } else {
      const int64_t qz = size / ((int64_t)in.card[0] * in.card[1]);
      const int64_t nc = (qz + kCiChunk - 1) / kCiChunk;
      ci_chunks += nc;
      if (qz == 1 && in.card[0] + in.card[1] <= kCiSmall) out.ci_single.push_back(f);
      else ci_blocks += nc;
    }
    // consecutive families share a workgroup while their tables fit the LDS tile together; a family
    // larger than the tile is a group of its own and counts into global memory
    const bool big = size > kFitTileBins;
    if (big || out.groups.empty() || out.groups.back().global ||
        out.groups.back().bins + size > kFitTileBins) {
      FitGroup g;
      g.off = k.off, g.fam_begin = f, g.fam_end = f + 1, g.bins = (int32_t)size, g.global = big ? 1 : 0;
      out.groups.push_back(g);
    } else {
      out.groups.back().fam_end = f + 1;
      out.groups.back().bins += (int32_t)size;
    }
    out.group_of[(size_t)f] = (int32_t)out.groups.size() - 1;
  }
  out.col_off[(size_t)n] = cols;
  out.chunk_off[(size_t)n] = chunks;
  out.ci_off[(size_t)n] = ci_chunks;
  out.ci_multi_off[(size_t)n] = ci_blocks;
  out.total_bins = off;
  return PGM_OK;
}

int fit_count_check(const FitHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                    const void *tables, int64_t *blocks) {
  if (!h) return pgmi_fail(PGM_EINVAL, "fit_count: null plan");
  if (!codes) return pgmi_fail(PGM_EINVAL, "fit_count: null codes");
  if (!tables) return pgmi_fail(PGM_EINVAL, "fit_count: null tables");
  const int st = window_check("fit_count", "rows", ld, row0, n_rows, 0);
  if (st != PGM_OK) return st;
  if (n_cols < h->p.n_cols)
    return pgmi_failf(PGM_EINVAL, "fit_count: the plan reads column %d, codes has %d columns", h->p.n_cols - 1, n_cols);
  const int64_t chunks = (n_rows + kFitRowsPerBlock - 1) / kFitRowsPerBlock;
  const int64_t nb = chunks * (int64_t)h->p.groups.size();
  if (nb > INT32_MAX)
    return pgmi_failf(PGM_EINVAL, "fit_count: %lld workgroups (count the rows in several calls)", (long long)nb);
  if (blocks) *blocks = nb;
  return PGM_OK;
}

bool codes_vec4(const void *codes, int64_t ld, int64_t row0) {
  return ((uintptr_t)codes & 3) == 0 && (ld & 3) == 0 && (row0 & 3) == 0;
}

int window_check(const char *what, const char *noun, int64_t ld, int64_t row0, int64_t n, int64_t first) {
  if (n < 0 || row0 < 0) return pgmi_failf(PGM_EINVAL, "%s: n_%s %lld row0 %lld", what, noun, (long long)n, (long long)row0);
  if (ld < n || row0 > ld - n)
    return pgmi_failf(PGM_EINVAL, "%s: rows [%lld, %lld) outside ld %lld", what, (long long)row0, (long long)(row0 + n),
                      (long long)ld);
  if (first < 0 || first > INT64_MAX - n)
    return pgmi_failf(PGM_EINVAL, "%s: stream %s [%lld, + %lld)", what, noun, (long long)first, (long long)n);
  return PGM_OK;
}

void plan_info_layout(const FitPlan &p, int64_t *offsets, int64_t *sizes) {
  for (size_t f = 0; f < p.fams.size(); ++f) {
    if (offsets) offsets[f] = p.fams[f].off;
    if (sizes) sizes[f] = p.fams[f].size;
  }
}

int fit_finish_check(const FitHandle *h, const void *counts, int32_t mode, const double *values) {
  if (!h) return pgmi_fail(PGM_EINVAL, "fit_finish: null plan");
  if (!counts) return pgmi_fail(PGM_EINVAL, "fit_finish: null counts");
  if (!values) return pgmi_fail(PGM_EINVAL, "fit_finish: null values");
  if (mode & ~(PGM_FIT_BAYES | PGM_FIT_WEIGHTED)) return pgmi_failf(PGM_EINVAL, "fit_finish: mode %d", mode);
  return PGM_OK;
}

int fit_score_check(const FitHandle *h, const int64_t *counts, int32_t mode, const double *alpha, const double *beta,
                    const double *scores, int64_t *blocks) {
  if (!h) return pgmi_fail(PGM_EINVAL, "fit_score: null plan");
  if (!counts) return pgmi_fail(PGM_EINVAL, "fit_score: null counts");
  if (!scores) return pgmi_fail(PGM_EINVAL, "fit_score: null scores");
  if (mode & ~(PGM_SCORE_LL | PGM_SCORE_SKIP_EMPTY)) return pgmi_failf(PGM_EINVAL, "fit_score: mode %d", mode);
  if (!(mode & PGM_SCORE_LL)) {
    if (!alpha) return pgmi_fail(PGM_EINVAL, "fit_score: null alpha in BD mode");
    if (!beta) return pgmi_fail(PGM_EINVAL, "fit_score: null beta in BD mode");
  }
  const int64_t nb = h->p.chunk_off.back();
  if (nb > INT32_MAX) return pgmi_failf(PGM_EINVAL, "fit_score: %lld workgroups (score the families in several plans)", (long long)nb);
  if (blocks) *blocks = nb;
  return PGM_OK;
}

int fit_citest_check(const FitHandle *h, const int64_t *counts, double lambda, int32_t flags, const double *stat,
                     const int64_t *dof, const double *pvalue, int64_t *blocks) {
  if (!h) return pgmi_fail(PGM_EINVAL, "fit_citest: null plan");
  if (!counts) return pgmi_fail(PGM_EINVAL, "fit_citest: null counts");
  if (!stat) return pgmi_fail(PGM_EINVAL, "fit_citest: null stat");
  if (!dof) return pgmi_fail(PGM_EINVAL, "fit_citest: null dof");
  if (!pvalue) return pgmi_fail(PGM_EINVAL, "fit_citest: null pvalue");
  if (!std::isfinite(lambda)) return pgmi_failf(PGM_EINVAL, "fit_citest: lambda %g is not finite", lambda);
  if (flags & ~PGM_CI_YATES) return pgmi_failf(PGM_EINVAL, "fit_citest: flags %d", flags);
  if (h->p.ci_bad >= 0)
    return pgmi_failf(PGM_EINVAL, "fit_citest: family %d has fewer than two variables (a test needs X and Y)",
                      h->p.ci_bad);
  const int64_t nb = h->p.ci_multi_off.back();
  if (nb > INT32_MAX) return pgmi_failf(PGM_EINVAL, "fit_citest: %lld workgroups (test the families in several plans)", (long long)nb);
  if (blocks) *blocks = nb;
  return PGM_OK;
}

int fit_estep_spec(const FitHandle *h, const int32_t *latent_cols, int32_t n_latent, const char *what, EmSpec *spec,
                   int32_t *n_obs_cols) {
  if (!h) return pgmi_failf(PGM_EINVAL, "%s: null plan", what);
  if (!latent_cols) return pgmi_failf(PGM_EINVAL, "%s: null latent_cols", what);
  if (n_latent < 1 || n_latent > PGM_EM_MAX_LATENT)
    return pgmi_failf(PGM_EINVAL, "%s: %d latent columns (1 .. %d)", what, n_latent, PGM_EM_MAX_LATENT);
  EmSpec s;
  memset(&s, 0, sizeof s);
  s.n_latent = n_latent;
  s.n_fam = (int32_t)h->p.fams.size();
  for (int32_t j = 0; j < n_latent; ++j) {
    if (latent_cols[j] < 0) return pgmi_failf(PGM_EINVAL, "%s: latent column %d", what, latent_cols[j]);
    for (int32_t i = 0; i < j; ++i)
      if (latent_cols[i] == latent_cols[j])
        return pgmi_failf(PGM_EINVAL, "%s: latent column %d is listed twice", what, latent_cols[j]);
    s.col[j] = latent_cols[j];
  }
  int32_t obs_cols = 0;
  for (int32_t f = 0; f < s.n_fam; ++f) {
    const FitFam &F = h->p.fams[(size_t)f];
    int32_t k = -1;  // the family's slot in s.fam once a latent is found in its scope
    for (int32_t v = 0; v < F.n_vars; ++v) {
      int32_t j = 0;
      while (j < n_latent && s.col[j] != F.col[v]) ++j;
      if (j == n_latent) {
        if (F.col[v] + 1 > obs_cols) obs_cols = F.col[v] + 1;
        continue;
      }
      if (s.card[j] != 0 && s.card[j] != F.card[v])
        return pgmi_failf(PGM_EINVAL, "%s: latent column %d has cardinality %d in family %d and %d in an earlier one",
                          what, s.col[j], F.card[v], f, s.card[j]);
      s.card[j] = F.card[v];
      if (k < 0) {
        if (s.n_lat_fam == PGM_EM_MAX_FAMILIES)
          return pgmi_failf(PGM_EINVAL, "%s: more than %d families have a latent in scope", what, PGM_EM_MAX_FAMILIES);
        k = s.n_lat_fam++;
        s.fam[k] = f;
      }
      // a column listed twice in one family adds both strides, as the count kernel adds both codes
      s.stride[k][j] += F.stride[v];
    }
  }
  int64_t configs = 1;
  for (int32_t j = 0; j < n_latent; ++j) {
    if (s.card[j] == 0) return pgmi_failf(PGM_EINVAL, "%s: latent column %d is in no family of the plan", what, s.col[j]);
    configs *= s.card[j];
    if (configs > PGM_EM_MAX_CONFIGS)
      return pgmi_failf(PGM_EINVAL, "%s: more than %d latent configurations", what, PGM_EM_MAX_CONFIGS);
  }
  s.n_configs = (int32_t)configs;
  if (spec) *spec = s;
  if (n_obs_cols) *n_obs_cols = obs_cols;
  return PGM_OK;
}

int fit_estep_check(const FitHandle *h, const int32_t *latent_cols, int32_t n_latent, const double *values,
                    const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, const double *tables,
                    EmSpec *spec, int64_t *blocks) {
  if (!h) return pgmi_fail(PGM_EINVAL, "fit_estep: null plan");
  if (!values) return pgmi_fail(PGM_EINVAL, "fit_estep: null values");
  if (!codes) return pgmi_fail(PGM_EINVAL, "fit_estep: null codes");
  if (!tables) return pgmi_fail(PGM_EINVAL, "fit_estep: null tables");
  int32_t obs_cols = 0;
  const int st = fit_estep_spec(h, latent_cols, n_latent, "fit_estep", spec, &obs_cols);
  if (st != PGM_OK) return st;
  const int win = window_check("fit_estep", "rows", ld, row0, n_rows, 0);
  if (win != PGM_OK) return win;
  if (n_cols < obs_cols)
    return pgmi_failf(PGM_EINVAL, "fit_estep: the plan reads the observed column %d, codes has %d columns", obs_cols - 1,
                      n_cols);
  const int64_t chunks = (n_rows + kFitRowsPerBlock - 1) / kFitRowsPerBlock;
  const int64_t nb = chunks * (int64_t)h->p.groups.size();
  if (nb > INT32_MAX)
    return pgmi_failf(PGM_EINVAL, "fit_estep: %lld workgroups (count the rows in several calls)", (long long)nb);
  if (blocks) *blocks = nb;
  return PGM_OK;
}

int fit_states_check(const FitHandle *h, const int64_t *counts, const int64_t *n_states) {
  if (!h) return pgmi_fail(PGM_EINVAL, "fit_states_observed: null plan");
  if (!counts) return pgmi_fail(PGM_EINVAL, "fit_states_observed: null counts");
  if (!n_states) return pgmi_fail(PGM_EINVAL, "fit_states_observed: null n_states");
  return PGM_OK;
}

static bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }

int fit_log_values_check(const FitHandle *h, const double *values, const double *logv, int64_t *blocks) {
  if (!h) return pgmi_fail(PGM_EINVAL, "fit_log_values: null plan");
  if (!values) return pgmi_fail(PGM_EINVAL, "fit_log_values: null values");
  if (!logv) return pgmi_fail(PGM_EINVAL, "fit_log_values: null logv");
  if (!aligned8(values) || !aligned8(logv))
    return pgmi_fail(PGM_EINVAL, "fit_log_values: values and logv must be 8-byte aligned");
  const int64_t nb = (h->p.total_bins + kLogpBlock - 1) / kLogpBlock;
  if (nb > INT32_MAX) return pgmi_fail(PGM_EINVAL, "fit_log_values: too many table entries for one launch");
  if (blocks) *blocks = nb;
  return PGM_OK;
}

int fit_logprob_check(const FitHandle *h, const double *logv, const uint8_t *codes, int32_t n_cols, int64_t ld,
                      int64_t row0, int64_t n_rows, const double *logp, const double *total, const int64_t *n_skipped,
                      int64_t *blocks) {
  if (!h) return pgmi_fail(PGM_EINVAL, "fit_logprob: null plan");
  if (!logv) return pgmi_fail(PGM_EINVAL, "fit_logprob: null logv");
  if (!codes) return pgmi_fail(PGM_EINVAL, "fit_logprob: null codes");
  if (!aligned8(logv) || !aligned8(logp) || !aligned8(total) || !aligned8(n_skipped))
    return pgmi_fail(PGM_EINVAL, "fit_logprob: logv, logp, total and n_skipped must be 8-byte aligned");
  const int st = window_check("fit_logprob", "rows", ld, row0, n_rows, 0);
  if (st != PGM_OK) return st;
  if (n_cols < h->p.n_cols)
    return pgmi_failf(PGM_EINVAL, "fit_logprob: the plan reads column %d, codes has %d columns", h->p.n_cols - 1, n_cols);
  const int64_t nb = (n_rows + kLogpRowsPerBlock - 1) / kLogpRowsPerBlock;
  if (nb > kLogpMaxBlocks)
    return pgmi_failf(PGM_EINVAL, "fit_logprob: %lld workgroups, a call covers %d (score the rows in several calls)",
                      (long long)nb, kLogpMaxBlocks);
  if (blocks) *blocks = nb;
  return PGM_OK;
}

extern "C" {

int pgm_fit_logprob_info(void *plan, const void *codes, int64_t ld, int64_t row0, int64_t n_rows,
                         pgm_logp_info_t *info) {
  if (!plan) return pgmi_fail(PGM_EINVAL, "fit_logprob_info: null plan");
  if (!info) return pgmi_fail(PGM_EINVAL, "fit_logprob_info: null info");
  const int st = window_check("fit_logprob_info", "rows", ld, row0, n_rows, 0);
  if (st != PGM_OK) return st;
  memset(info, 0, sizeof *info);
  info->block = kLogpBlock;
  info->rows_per_block = kLogpRowsPerBlock;
  info->vec4 = codes && codes_vec4(codes, ld, row0) ? 1 : 0;
  info->n_families = (int32_t)static_cast<const FitHandle *>(plan)->p.fams.size();
  info->n_partials = (n_rows + kLogpRowsPerBlock - 1) / kLogpRowsPerBlock;
  return PGM_OK;
}

int pgm_fit_plan_create(const pgm_fit_family *fams, int32_t n, void **plan) {
  return plan_create<FitHandle>("fit_plan_create", plan, [&](FitPlan &p) { return fit_plan_build(fams, n, p); });
}

int pgm_fit_plan_info(void *plan, pgm_fit_info_t *info, int64_t *offsets, int64_t *sizes, int32_t *strides,
                      int32_t *groups) {
  if (!plan) return pgmi_fail(PGM_EINVAL, "fit_plan_info: null plan");
  const FitPlan &p = static_cast<const FitHandle *>(plan)->p;
  if (info) {
    memset(info, 0, sizeof *info);
    info->n_families = (int32_t)p.fams.size();
    info->n_groups = (int32_t)p.groups.size();
    info->tile_bins = kFitTileBins;
    info->rows_per_block = kFitRowsPerBlock;
    info->n_cols = p.n_cols;
    info->block = kFitBlock;
    info->total_bins = p.total_bins;
    info->total_columns = p.col_off.back();
  }
  plan_info_layout(p, offsets, sizes);
  for (size_t f = 0; f < p.fams.size(); ++f) {
    if (strides) memcpy(strides + f * PGM_MAX_DIMS, p.fams[f].stride, sizeof p.fams[f].stride);
    if (groups) groups[f] = p.group_of[f];
  }
  return PGM_OK;
}

int pgm_fit_estep_info(void *plan, const int32_t *latent_cols, int32_t n_latent, pgm_em_info_t *info) {
  if (!info) return pgmi_fail(PGM_EINVAL, "fit_estep_info: null info");
  EmSpec s;
  const int st = fit_estep_spec(static_cast<const FitHandle *>(plan), latent_cols, n_latent, "fit_estep_info", &s, nullptr);
  if (st != PGM_OK) return st;
  memset(info, 0, sizeof *info);
  info->n_latent = s.n_latent;
  info->n_configs = s.n_configs;
  info->n_latent_families = s.n_lat_fam;
  info->n_plain_families = s.n_fam - s.n_lat_fam;
  info->block = kFitBlock;
  info->rows_per_block = kFitRowsPerBlock;
  info->lds_bytes = fit_estep_lds(s.n_lat_fam);
  return PGM_OK;
}
}

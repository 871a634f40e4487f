// pgmlw_plan.cpp — the host side of the likelihood-weighted posterior (pgm_sample_posterior;
// pgmpy_amd.inference.ApproxInference): the launch geometry (workgroup size against the LDS budget, the
// fixed-point exponent K, rows per launch), the argument checks and the host-only query.  No HIP include.
// The kernels and launches are pgmlw.hip.
#include <cstring>
#include <map>

#include "pgm_internal.h"
#include "pgm_lw.h"

static bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }

int lw_geometry(const char *what, const SampleHandle *h, const FitHandle *t, int64_t n_samples, int32_t block,
                LwGeometry *g) {
  if (n_samples < 1 || n_samples > kLwMaxSamples)
    return pgmi_failf(PGM_EINVAL, "%s: n_samples %lld (1 .. %lld)", what, (long long)n_samples, (long long)kLwMaxSamples);
  if (block != 0 && block != 64 && block != 128 && block != 256)
    return pgmi_failf(PGM_EINVAL, "%s: block %d (0: automatic, 64, 128 or 256)", what, block);
  const int64_t n_cols = h->p.fit.n_cols, bins = t->p.total_bins;
  int32_t chosen = 0;
  for (int32_t b = block ? block : 256; b >= 64; b >>= 1) {
    if (lw_lds_bytes(n_cols, bins, b, true) <= kLwLdsBudget) {
      chosen = b;
      break;
    }
    if (block) break;  // a forced size is not stepped down
  }
  if (!chosen)
    return pgmi_failf(PGM_EINVAL,
                      "%s: %lld target bins (8 bytes each) and %lld code columns (%d bytes each) take %lld bytes of LDS "
                      "with a workgroup of %d, the budget is %d",
                      what, (long long)bins, (long long)n_cols, block ? block : 64,
                      (long long)lw_lds_bytes(n_cols, bins, block ? block : 64, true), block ? block : 64, kLwLdsBudget);
  int32_t log2s = 0;  // ceil(log2 n_samples)
  while (((int64_t)1 << log2s) < n_samples) ++log2s;
  g->block = chosen;
  g->k = 62 - log2s < 52 ? 62 - log2s : 52;
  g->lds_bytes = (int32_t)lw_lds_bytes(n_cols, bins, chosen, true);
  g->n_cols = (int32_t)n_cols;
  g->total_bins = bins;
  g->chunks = (n_samples + kLwChunk - 1) / kLwChunk;
  g->rows_per_launch = kLwMaxGroups / g->chunks;
  if (g->rows_per_launch > 65535) g->rows_per_launch = 65535;  // the finishing launch's grid.y
  return PGM_OK;
}

int sample_posterior_check(const SampleHandle *h, const FitHandle *t, const double *values, const double *cdf,
                           const uint8_t *modes, const uint8_t *evidence, int32_t n_cols, int64_t ld, int64_t row0,
                           int64_t n_rows, int64_t n_samples, int64_t first_row, int32_t block, const void *acc,
                           const void *scale, const void *post, const void *log_evidence, const void *ess,
                           LwGeometry *g) {
  if (!h) return pgmi_fail(PGM_EINVAL, "sample_posterior: null plan");
  if (!t) return pgmi_fail(PGM_EINVAL, "sample_posterior: null targets");
  if (!values) return pgmi_fail(PGM_EINVAL, "sample_posterior: null values");
  if (!cdf) return pgmi_fail(PGM_EINVAL, "sample_posterior: null cdf");
  if (!evidence) return pgmi_fail(PGM_EINVAL, "sample_posterior: null evidence");
  if (!acc) return pgmi_fail(PGM_EINVAL, "sample_posterior: null acc");
  if (!scale) return pgmi_fail(PGM_EINVAL, "sample_posterior: null scale");
  if (!aligned8(values) || !aligned8(cdf) || !aligned8(acc) || !aligned8(scale) || !aligned8(post) ||
      !aligned8(log_evidence) || !aligned8(ess))
    return pgmi_fail(PGM_EINVAL,
                     "sample_posterior: values, cdf, acc, scale, post, log_evidence and ess must be 8-byte aligned");
  const int st = window_check("sample_posterior", "rows", ld, row0, n_rows, 0);
  if (st != PGM_OK) return st;
  const int gs = lw_geometry("sample_posterior", h, t, n_samples, block, g);
  if (gs != PGM_OK) return gs;
  if (first_row < 0 || n_rows > (INT64_MAX - first_row) / n_samples)
    return pgmi_failf(PGM_EINVAL, "sample_posterior: stream rows [%lld, + %lld x %lld)", (long long)first_row,
                      (long long)n_rows, (long long)n_samples);
  if (n_cols < h->p.fit.n_cols)
    return pgmi_failf(PGM_EINVAL, "sample_posterior: the plan reads column %d, evidence has %d columns",
                      h->p.fit.n_cols - 1, n_cols);
  if (n_cols < t->p.n_cols)
    return pgmi_failf(PGM_EINVAL, "sample_posterior: the targets read column %d, evidence has %d columns", t->p.n_cols - 1,
                      n_cols);
  if (modes)
    for (size_t f = 0; f < h->p.fit.fams.size(); ++f)
      if (modes[f] > PGM_SAMPLE_OBSERVED)
        return pgmi_failf(PGM_EINVAL, "sample_posterior: family %d mode %d", (int)f, (int)modes[f]);
  std::map<int32_t, int32_t> card_of;  // code column -> cardinality of the family whose node it is
  for (const FitFam &F : h->p.fit.fams) card_of[F.col[0]] = F.card[0];
  for (size_t f = 0; f < t->p.fams.size(); ++f) {
    const FitFam &F = t->p.fams[f];
    for (int32_t v = 0; v < F.n_vars; ++v) {
      const auto it = card_of.find(F.col[v]);
      if (it == card_of.end())
        return pgmi_failf(PGM_EINVAL, "sample_posterior: target %d column %d is the node of no family of the sample plan",
                          (int)f, F.col[v]);
      if (it->second != F.card[v])
        return pgmi_failf(PGM_EINVAL, "sample_posterior: target %d column %d cardinality %d, the sample plan has %d", (int)f,
                          F.col[v], F.card[v], it->second);
    }
  }
  return PGM_OK;
}

extern "C" {

int pgm_sample_posterior_info(void *plan, void *targets, int64_t n_rows, int64_t n_samples, int32_t block,
                              pgm_lw_info_t *info) {
  if (!plan) return pgmi_fail(PGM_EINVAL, "sample_posterior_info: null plan");
  if (!targets) return pgmi_fail(PGM_EINVAL, "sample_posterior_info: null targets");
  if (!info) return pgmi_fail(PGM_EINVAL, "sample_posterior_info: null info");
  if (n_rows < 0) return pgmi_failf(PGM_EINVAL, "sample_posterior_info: n_rows %lld", (long long)n_rows);
  LwGeometry g;
  const int st = lw_geometry("sample_posterior_info", static_cast<const SampleHandle *>(plan),
                             static_cast<const FitHandle *>(targets), n_samples, block, &g);
  if (st != PGM_OK) return st;
  memset(info, 0, sizeof *info);
  info->block = g.block;
  info->chunk = kLwChunk;
  info->k = g.k;
  info->lds_bytes = g.lds_bytes;
  info->lds_budget = kLwLdsBudget;
  info->n_cols = g.n_cols;
  info->total_bins = g.total_bins;
  info->chunks_per_row = g.chunks;
  info->workgroups = n_rows * g.chunks;
  info->rows_per_launch = g.rows_per_launch;
  return PGM_OK;
}
}

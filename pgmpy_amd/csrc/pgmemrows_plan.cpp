// pgmemrows_plan.cpp — the host side of the rows E-step (pgm_fit_estep_rows): the plan's column lists (every
// code column with its cardinality and the families that hold it), the latent columns of a call, the argument
// checks and pgm_fit_estep_rows_info.  No HIP include: every path here runs without a device.  The kernel and
// the launch are pgmemrows.hip.
#include <algorithm>
#include <cstring>

#include "pgm_emrows.h"

int emr_lists(FitHandle *h, const char *what) {
  EmrLists &e = h->emr;
  std::lock_guard<std::mutex> lk(e.mu);
  if (!e.built) {
    const FitPlan &p = h->p;
    // (column, family) pairs in ascending order; a family that lists a column twice is kept once
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (size_t f = 0; f < p.fams.size(); ++f)
      for (int32_t v = 0; v < p.fams[f].n_vars; ++v) pairs.emplace_back(p.fams[f].col[v], (int32_t)f);
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    for (const auto &pr : pairs) {
      if (e.cols.empty() || e.cols.back() != pr.first) {
        e.cols.push_back(pr.first);
        e.card.push_back(0);
        e.inc_off.push_back((int32_t)e.inc_fam.size());
      }
      e.inc_fam.push_back(pr.second);
      const FitFam &F = p.fams[(size_t)pr.second];
      for (int32_t v = 0; v < F.n_vars; ++v) {
        if (F.col[v] != pr.first) continue;
        if (e.card.back() == 0) e.card.back() = F.card[v];
        else if (e.card.back() != F.card[v] && e.two_card < 0) e.two_card = pr.first;
      }
    }
    e.inc_off.push_back((int32_t)e.inc_fam.size());
    e.built = true;
  }
  if (e.two_card >= 0)
    return pgmi_failf(PGM_EINVAL, "%s: column %d has two cardinalities in the plan's families", what, e.two_card);
  return PGM_OK;
}

int emr_spec(FitHandle *h, const int32_t *latent_cols, int32_t n_latent, int32_t flags, bool want_tables,
             const char *what, EmrSpec *spec, int32_t *n_obs_cols) {
  if (!h) return pgmi_failf(PGM_EINVAL, "%s: null plan", what);
  if (n_latent < 0 || n_latent > kEmrMaxU)
    return pgmi_failf(PGM_EINVAL, "%s: %d latent columns (0 .. %d)", what, n_latent, kEmrMaxU);
  if (n_latent > 0 && !latent_cols) return pgmi_failf(PGM_EINVAL, "%s: null latent_cols", what);
  if (flags & ~PGM_EMR_NO_FLOOR) return pgmi_failf(PGM_EINVAL, "%s: flags %d", what, flags);
  // a latent with two cardinalities is named as such before the plan-wide check names the column
  for (int32_t j = 0; j < n_latent; ++j) {
    if (latent_cols[j] < 0) return pgmi_failf(PGM_EINVAL, "%s: latent column %d", what, latent_cols[j]);
    for (int32_t i = 0; i < j; ++i)
      if (latent_cols[i] == latent_cols[j])
        return pgmi_failf(PGM_EINVAL, "%s: latent column %d is listed twice", what, latent_cols[j]);
    int32_t card = 0;
    for (const FitFam &F : h->p.fams)
      for (int32_t v = 0; v < F.n_vars; ++v) {
        if (F.col[v] != latent_cols[j]) continue;
        if (card != 0 && card != F.card[v])
          return pgmi_failf(PGM_EINVAL, "%s: latent column %d has cardinality %d in one family and %d in an earlier one",
                            what, latent_cols[j], F.card[v], card);
        card = F.card[v];
      }
    if (card == 0) return pgmi_failf(PGM_EINVAL, "%s: latent column %d is in no family of the plan", what, latent_cols[j]);
  }
  const int st = emr_lists(h, what);
  if (st != PGM_OK) return st;
  const EmrLists &e = h->emr;
  EmrSpec s;
  memset(&s, 0, sizeof s);
  s.n_latent = n_latent;
  s.n_pos = (int32_t)e.cols.size();
  s.n_fam = (int32_t)h->p.fams.size();
  s.flags = flags;
  s.tile = want_tables && h->p.total_bins <= kFitTileBins ? 1 : 0;
  s.total_bins = (int32_t)std::min<int64_t>(h->p.total_bins, INT32_MAX);
  int32_t obs_cols = 0, k = 0;
  for (int32_t i = 0; i < s.n_pos; ++i) {
    bool latent = false;
    for (int32_t j = 0; j < n_latent; ++j) latent |= latent_cols[j] == e.cols[(size_t)i];
    if (latent) s.pos[k++] = i;
    else obs_cols = e.cols[(size_t)i] + 1;
  }
  if (spec) *spec = s;
  if (n_obs_cols) *n_obs_cols = obs_cols;
  return PGM_OK;
}

int emr_check(FitHandle *h, const int32_t *latent_cols, int32_t n_latent, int32_t flags, const double *values,
              const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, const double *tables,
              const double *loglik, EmrSpec *spec, int64_t *blocks) {
  const char *what = "fit_estep_rows";
  if (!h) return pgmi_failf(PGM_EINVAL, "%s: null plan", what);
  if (!values) return pgmi_failf(PGM_EINVAL, "%s: null values", what);
  if (!codes) return pgmi_failf(PGM_EINVAL, "%s: null codes", what);
  if (!tables && !loglik) return pgmi_failf(PGM_EINVAL, "%s: null tables and null loglik: nothing to compute", what);
  int32_t obs_cols = 0;
  const int st = emr_spec(h, latent_cols, n_latent, flags, tables != nullptr, what, spec, &obs_cols);
  if (st != PGM_OK) return st;
  const int win = window_check(what, "rows", ld, row0, n_rows, 0);
  if (win != PGM_OK) return win;
  if (n_cols < obs_cols)
    return pgmi_failf(PGM_EINVAL, "%s: the plan reads the observed column %d, codes has %d columns", what, obs_cols - 1,
                      n_cols);
  const int64_t nb = (n_rows + kEmrRows - 1) / kEmrRows;
  if (nb > INT32_MAX) return pgmi_failf(PGM_EINVAL, "%s: %lld workgroups (take the rows in several calls)", what, (long long)nb);
  if (blocks) *blocks = nb;
  return PGM_OK;
}

extern "C" {

int pgm_fit_estep_rows_info(void *plan, const int32_t *latent_cols, int32_t n_latent, pgm_emr_info_t *info) {
  if (!info) return pgmi_fail(PGM_EINVAL, "fit_estep_rows_info: null info");
  FitHandle *h = static_cast<FitHandle *>(plan);
  EmrSpec s;
  const int st = emr_spec(h, latent_cols, n_latent, 0, true, "fit_estep_rows_info", &s, nullptr);
  if (st != PGM_OK) return st;
  memset(info, 0, sizeof *info);
  info->block = kEmrBlock;
  info->rows_per_block = kEmrRows;
  info->tile = s.tile;
  info->tile_bins = kFitTileBins;
  info->lds_bytes = kEmrStaticLds + (s.tile ? s.total_bins * (int32_t)sizeof(double) : 0);
  info->blocks_per_cu = std::min(kEmrBlocksPerCuByRegs, 160 * 1024 / info->lds_bytes);  // registers, then 160 KiB of LDS
  info->n_columns = s.n_pos;
  info->n_latent = s.n_latent;
  info->n_families = s.n_fam;
  info->max_unobserved = kEmrMaxU;
  info->max_configs = PGM_EM_MAX_CONFIGS;
  info->max_component_families = kEmrMaxFam;
  info->max_row_families = kEmrMaxRowFam;
  info->total_bins = h->p.total_bins;
  return PGM_OK;
}
}

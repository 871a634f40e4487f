// pgmcg_plan.cpp — the host side of the conditional-Gaussian scores (include/pgmhip.h "conditional-Gaussian
// scores"): validation of the families, the operand layout (mp, tiles, blocks of tiles, jobs and their
// chunks), the choice of the row slice and of the passes over the stage, and the argument checks of the
// pgm_cg_* entry points.  No HIP call and no HIP include: ctypes drives all of it without a device.  The
// kernels and launches are pgmcg.hip.
#include <algorithm>
#include <new>

#include "pgm_cg.h"

static int64_t cg_round_up(int64_t x, int64_t q) { return (x + q - 1) / q * q; }

static int cg_distinct(const char *what, int32_t f, const int32_t *cols, int32_t n, int32_t *top) {
  std::vector<int32_t> sorted(cols, cols + n);
  std::sort(sorted.begin(), sorted.end());
  for (int32_t i = 0; i < n; ++i) {
    if (sorted[(size_t)i] < 0) return pgmi_failf(PGM_EINVAL, "cg_plan_create: family %d names %s column %d", f, what, sorted[(size_t)i]);
    if (i > 0 && sorted[(size_t)i] == sorted[(size_t)i - 1])
      return pgmi_failf(PGM_EINVAL, "cg_plan_create: family %d lists %s column %d twice", f, what, sorted[(size_t)i]);
    *top = std::max(*top, sorted[(size_t)i] + 1);
  }
  return PGM_OK;
}

int cg_plan_build(const pgm_cg_family *fams, int32_t n, CgPlan &out) {
  if (n < 1) return pgmi_failf(PGM_EINVAL, "cg_plan_create: %d families", n);
  if (!fams) return pgmi_failf(PGM_EINVAL, "cg_plan_create: null families");
  CgPlan p;
  p.chunk_off.push_back(0);
  for (int32_t f = 0; f < n; ++f) {
    const pgm_cg_family &in = fams[f];
    if (in.n_cont < 0 || in.n_cont > kCgMaxCont)
      return pgmi_failf(PGM_EINVAL, "cg_plan_create: family %d has %d continuous columns (PGM_CG_MAX_CONT = %d)", f, in.n_cont,
                        kCgMaxCont);
    if (in.n_disc < 0 || in.n_disc > PGM_MAX_DIMS)
      return pgmi_failf(PGM_EINVAL, "cg_plan_create: family %d has %d discrete columns (PGM_MAX_DIMS = %d)", f, in.n_disc,
                        PGM_MAX_DIMS);
    if (in.var_discrete != 0 && in.var_discrete != 1)
      return pgmi_failf(PGM_EINVAL, "cg_plan_create: family %d: var_discrete %d", f, in.var_discrete);
    if ((in.var_discrete ? in.n_disc : in.n_cont) < 1)
      return pgmi_failf(PGM_EINVAL, "cg_plan_create: family %d has no %s column for its variable", f,
                        in.var_discrete ? "discrete" : "continuous");
    if (const int st = cg_distinct("discrete", f, in.dcol, in.n_disc, &p.n_code_cols)) return st;
    if (const int st = cg_distinct("continuous", f, in.ccol, in.n_cont, &p.n_value_cols)) return st;
    CgFam F = {};
    F.n_disc = in.n_disc, F.m = in.n_cont, F.var_disc = in.var_discrete;
    F.mp = 1;
    while (F.mp < F.m + 1) F.mp *= 2;
    int64_t Q = 1;
    for (int32_t d = 0; d < in.n_disc; ++d) {
      if (in.card[d] < 1 || in.card[d] > 255)
        return pgmi_failf(PGM_EINVAL, "cg_plan_create: family %d: cardinality %d of column %d (1 .. 255)", f, in.card[d], in.dcol[d]);
      Q *= in.card[d];
      if (Q * F.mp > kCgMaxRows)
        return pgmi_failf(PGM_EINVAL,
                          "cg_plan_create: family %d has more than PGM_CG_MAX_ROWS = %d operand rows (configurations x %d "
                          "padded columns)",
                          f, kCgMaxRows, F.mp);
      F.dcol[d] = in.dcol[d], F.card[d] = in.card[d];
    }
    for (int32_t d = in.n_disc - 1, s = 1; d >= 0; --d) {  // C order: the first column slowest
      F.stride[d] = s;
      s *= in.card[d];
    }
    for (int32_t c = 0; c < in.n_cont; ++c) F.ccol[c] = in.ccol[c];
    F.Q = (int32_t)Q;
    F.QD = in.var_discrete ? F.Q / in.card[0] : F.Q;
    F.cpt = kCgTile / F.mp;
    F.n_tiles = (F.Q * F.mp + kCgTile - 1) / kCgTile;
    F.mom_off = p.moments_size;
    p.moments_size += (int64_t)F.Q * F.mp * F.mp;
    for (int32_t t0 = 0; t0 < F.n_tiles; t0 += kCgTilesPerWave)
      p.blocks.push_back(CgBlock{f, t0, std::min(kCgTilesPerWave, F.n_tiles - t0), 0, p.total_tiles + t0});
    p.total_tiles += F.n_tiles;
    p.total_jobs += F.QD;
    p.chunk_off.push_back(p.chunk_off.back() + (F.QD + kCgScoreChunk - 1) / kCgScoreChunk);
    p.fams.push_back(F);
  }
  p.stage_tiles = std::min(p.total_tiles * kCgMaxSlices, kCgStageTiles);
  out = std::move(p);
  return PGM_OK;
}

int64_t cg_slice_rows(const CgPlan &p, int64_t n_rows) {
  const int64_t fit = cg_round_up(std::max<int64_t>(1, (n_rows + kCgMaxSlices - 1) / kCgMaxSlices), kCgStep);
  const int64_t own = p.slice_rows > 0 ? cg_round_up(p.slice_rows, kCgStep) : kCgSliceMin;
  return std::max(own, fit);
}

bool cg_vec16(const void *X, int64_t ld_x, int64_t row0) { return ((uintptr_t)X % 16 == 0) && ld_x % 2 == 0 && row0 % 2 == 0; }

void cg_passes(const CgPlan &p, int64_t n_slices, std::vector<CgPass> &out) {
  out.clear();
  const int64_t room = p.stage_tiles / std::max<int64_t>(1, n_slices);  // tiles of one pass; >= one block's
  for (size_t b = 0; b < p.blocks.size(); ++b) {
    const CgBlock &B = p.blocks[b];
    if (out.empty() || out.back().n_tiles + B.n_tiles > room) out.push_back(CgPass{(int64_t)b, 0, B.tile_off, 0});
    out.back().n_blocks += 1;
    out.back().n_tiles += B.n_tiles;
  }
}

static int cg_window(const char *what, const char *name, const void *base, int32_t n_cols, int32_t plan_cols, int64_t ld,
                     int64_t elem, int64_t row0, int64_t n_rows) {
  if (plan_cols > 0 && !base) return pgmi_failf(PGM_EINVAL, "%s: null %s", what, name);
  if (ld < 0 || row0 > ld || n_rows > ld - row0)
    return pgmi_failf(PGM_EINVAL, "%s: rows [%lld, %lld) outside %s's ld %lld", what, (long long)row0, (long long)(row0 + n_rows),
                      name, (long long)ld);
  if (n_cols < 0 || plan_cols > n_cols)
    return pgmi_failf(PGM_EINVAL, "%s: column %d of %s is named, it has %d columns", what, plan_cols - 1, name, n_cols);
  if (ld > 0 && (int64_t)n_cols > (INT64_MAX / elem) / ld)
    return pgmi_failf(PGM_EINVAL, "%s: %d columns of %lld rows in %s", what, n_cols, (long long)ld, name);
  return PGM_OK;
}

int cg_moments_check(const CgHandle *h, const uint8_t *codes, int32_t n_code_cols, int64_t ld_codes, const double *X,
                     int32_t n_value_cols, int64_t ld_x, int64_t row0, int64_t n_rows, const double *shift, const double *moments,
                     int64_t *slice, int64_t *n_slices) {
  *slice = *n_slices = 0;
  if (!h) return pgmi_failf(PGM_EINVAL, "cg_moments: null plan");
  if (!moments) return pgmi_failf(PGM_EINVAL, "cg_moments: null moments");
  if (h->p.n_value_cols > 0 && !shift) return pgmi_failf(PGM_EINVAL, "cg_moments: null shift");
  if (n_rows < 0 || row0 < 0)
    return pgmi_failf(PGM_EINVAL, "cg_moments: n_rows %lld row0 %lld", (long long)n_rows, (long long)row0);
  if (const int st = cg_window("cg_moments", "codes", codes, n_code_cols, h->p.n_code_cols, ld_codes, 1, row0, n_rows)) return st;
  if (const int st = cg_window("cg_moments", "X", X, n_value_cols, h->p.n_value_cols, ld_x, 8, row0, n_rows)) return st;
  *slice = cg_slice_rows(h->p, n_rows);
  *n_slices = (n_rows + *slice - 1) / *slice;
  return PGM_OK;
}

int cg_score_check(const CgHandle *h, const double *moments, const double *ll, const int64_t *n_complete,
                   const int64_t *n_observed, const int64_t *n_dropped) {
  if (!h) return pgmi_failf(PGM_EINVAL, "cg_score: null plan");
  if (!moments) return pgmi_failf(PGM_EINVAL, "cg_score: null moments");
  if (!ll || !n_complete || !n_observed || !n_dropped) return pgmi_failf(PGM_EINVAL, "cg_score: null output");
  return PGM_OK;
}

extern "C" {

int pgm_cg_plan_create(const pgm_cg_family *families, int32_t n_families, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "cg_plan_create: null plan");
  *plan = nullptr;
  CgHandle *h = new (std::nothrow) CgHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "cg_plan_create: out of memory");
  const int st = cg_plan_build(families, n_families, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_cg_plan_info(void *plan, pgm_cg_info_t *info, int64_t *layout) {
  const CgHandle *h = static_cast<const CgHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "cg_plan_info: null plan");
  const CgPlan &p = h->p;
  if (info) {
    info->n_families = (int32_t)p.fams.size();
    info->n_code_cols = p.n_code_cols;
    info->n_value_cols = p.n_value_cols;
    info->reserved = 0;
    info->total_tiles = p.total_tiles;
    info->total_blocks = (int64_t)p.blocks.size();
    info->total_jobs = p.total_jobs;
    info->total_chunks = p.chunk_off.back();
    info->moments_size = p.moments_size;
    info->stage_tiles = p.stage_tiles;
    info->slice_rows = p.slice_rows;
  }
  if (layout)
    for (size_t f = 0; f < p.fams.size(); ++f) {
      const CgFam &F = p.fams[f];
      int64_t *o = layout + PGM_CG_LAYOUT * f;
      o[0] = F.mp, o[1] = F.Q, o[2] = (int64_t)F.Q * F.mp, o[3] = F.n_tiles, o[4] = F.mom_off, o[5] = F.QD;
    }
  return PGM_OK;
}

int pgm_cg_plan_set_slice(void *plan, int64_t slice_rows) {
  CgHandle *h = static_cast<CgHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "cg_plan_set_slice: null plan");
  if (slice_rows < 0 || slice_rows > kCgSliceMax)
    return pgmi_failf(PGM_EINVAL, "cg_plan_set_slice: %lld rows (0 .. %lld)", (long long)slice_rows, (long long)kCgSliceMax);
  h->p.slice_rows = slice_rows;
  return PGM_OK;
}

int pgm_cg_moments_info(void *plan, const void *X, int64_t ld_x, int64_t row0, int64_t n_rows, int64_t *slice_rows,
                        int64_t *n_slices, int64_t *n_passes, int32_t *vec16) {
  const CgHandle *h = static_cast<const CgHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "cg_moments_info: null plan");
  if (n_rows < 0) return pgmi_failf(PGM_EINVAL, "cg_moments_info: n_rows %lld", (long long)n_rows);
  const int64_t slice = cg_slice_rows(h->p, n_rows), slices = (n_rows + slice - 1) / slice;
  if (slice_rows) *slice_rows = slice;
  if (n_slices) *n_slices = slices;
  if (n_passes) {
    std::vector<CgPass> passes;
    cg_passes(h->p, slices, passes);
    *n_passes = (int64_t)passes.size();
  }
  if (vec16) *vec16 = cg_vec16(X, ld_x, row0) ? 1 : 0;
  return PGM_OK;
}
}

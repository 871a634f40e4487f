// pgmlg_plan.cpp — the host side of the linear-Gaussian networks (include/pgmhip.h "linear-Gaussian
// networks"): validation of a Gram handle's columns and a network handle's families, the tile groups, the
// choice of the row slice and of the column-sum pieces, and the argument checks of the pgm_lg_* entry
// points.  No HIP call and no HIP include: ctypes drives all of it without a device.  The kernels and
// launches are pgmlg.hip.
#include <algorithm>
#include <new>

#include "pgm_lg.h"

static int64_t lg_round_up(int64_t x, int64_t q) { return (x + q - 1) / q * q; }

// ---------------------------------------------------------------------------- the Gram handle
int lg_gram_plan_build(const int32_t *cols, int32_t d, LgGramPlan &out) {
  if (d < 0 || d > kLgMaxColumns) return pgmi_failf(PGM_EINVAL, "lg_gram_plan_create: %d columns (0 .. %d)", d, kLgMaxColumns);
  if (d > 0 && !cols) return pgmi_failf(PGM_EINVAL, "lg_gram_plan_create: null cols");
  LgGramPlan p;
  for (int32_t j = 0; j < d; ++j) {
    if (cols[j] < 0) return pgmi_failf(PGM_EINVAL, "lg_gram_plan_create: entry %d is column %d", j, cols[j]);
    p.n_cols = std::max(p.n_cols, cols[j] + 1);
  }
  {  // a column listed twice would be a pair of exactly collinear regressors that the caller did not ask for
    std::vector<int32_t> sorted(cols, cols + d);
    std::sort(sorted.begin(), sorted.end());
    for (int32_t j = 1; j < d; ++j)
      if (sorted[j] == sorted[j - 1])
        return pgmi_failf(PGM_EINVAL, "lg_gram_plan_create: column %d is listed twice", sorted[j]);
  }
  p.cols.assign(cols, cols + d);
  p.d = d;
  p.n_tiles = (d + 1 + kLgTile - 1) / kLgTile;
  p.n_super = (p.n_tiles + kLgSuper - 1) / kLgSuper;
  p.n_tile_pairs = (int64_t)p.n_tiles * (p.n_tiles + 1) / 2;
  p.lane_col.assign((size_t)p.n_super * kLgSuperCols, kLgPad);
  std::copy(p.cols.begin(), p.cols.end(), p.lane_col.begin());
  p.lane_col[(size_t)d] = kLgOnes;
  for (int32_t I = 0; I < p.n_super; ++I)
    for (int32_t J = I; J < p.n_super; ++J) p.groups.push_back(LgGroup{I, J});
  p.max_slices = std::max<int64_t>(4, kLgTargetBlocks / (int64_t)p.groups.size());
  out = std::move(p);
  return PGM_OK;
}

int64_t lg_slice_rows(const LgGramPlan &p, int64_t n_rows) {
  int64_t slice;
  if (p.slice_rows > 0) {
    slice = lg_round_up(p.slice_rows, kLgStep);
  } else {
    const int64_t want = std::max<int64_t>(1, kLgTargetBlocks / (int64_t)p.groups.size());  // slices that give every CU work
    slice = lg_round_up(std::max<int64_t>(kLgSliceMin, (n_rows + want - 1) / want), kLgStep);
  }
  // the handle's partials
  slice = std::max(slice, lg_round_up(std::max<int64_t>(1, (n_rows + p.max_slices - 1) / p.max_slices), kLgStep));
  return slice;
}

bool lg_vec16(const void *X, int64_t ld, int64_t row0) {
  return ((uintptr_t)X % 16 == 0) && ld % 2 == 0 && row0 % 2 == 0;
}

int64_t lg_colsum_chunk(int64_t n_rows) {
  const int64_t need = (n_rows + kLgColsumMaxChunks - 1) / kLgColsumMaxChunks;
  return std::max(kLgColsumChunk, lg_round_up(std::max<int64_t>(1, need), kLgColsumBlock));
}

int lg_window_check(const char *what, const void *X, int32_t n_cols, int32_t plan_cols, int64_t ld, int64_t row0,
                    int64_t n_rows) {
  if (!X) return pgmi_failf(PGM_EINVAL, "%s: null X", what);
  if (n_rows < 0 || row0 < 0)
    return pgmi_failf(PGM_EINVAL, "%s: n_rows %lld row0 %lld", what, (long long)n_rows, (long long)row0);
  if (ld < 0 || row0 > ld || n_rows > ld - row0)
    return pgmi_failf(PGM_EINVAL, "%s: rows [%lld, %lld) outside ld %lld", what, (long long)row0,
                      (long long)(row0 + n_rows), (long long)ld);
  if (n_cols < 0 || plan_cols > n_cols)
    return pgmi_failf(PGM_EINVAL, "%s: column %d is named, X has %d columns", what, plan_cols - 1, n_cols);
  if (ld > 0 && (int64_t)n_cols > (INT64_MAX / 8) / ld)
    return pgmi_failf(PGM_EINVAL, "%s: %d columns of %lld rows", what, n_cols, (long long)ld);
  return PGM_OK;
}

int lg_colsum_check(const LgGramHandle *h, const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                    const double *sums, const int64_t *counts, int64_t *chunk, int64_t *n_chunks) {
  *chunk = *n_chunks = 0;
  if (!h) return pgmi_failf(PGM_EINVAL, "lg_colsum: null plan");
  if (!sums || !counts) return pgmi_failf(PGM_EINVAL, "lg_colsum: null sums / counts");
  const int st = lg_window_check("lg_colsum", X, n_cols, h->p.n_cols, ld, row0, n_rows);
  if (st != PGM_OK) return st;
  if (n_rows == 0 || h->p.d == 0) return PGM_OK;
  *chunk = lg_colsum_chunk(n_rows);
  *n_chunks = (n_rows + *chunk - 1) / *chunk;
  return PGM_OK;
}

int lg_gram_check(const LgGramHandle *h, const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                  const double *shift, const double *out, int64_t *slice, int64_t *n_slices) {
  *slice = *n_slices = 0;
  if (!h) return pgmi_failf(PGM_EINVAL, "lg_gram: null plan");
  if (!shift || !out) return pgmi_failf(PGM_EINVAL, "lg_gram: null shift / out");
  const int st = lg_window_check("lg_gram", X, n_cols, h->p.n_cols, ld, row0, n_rows);
  if (st != PGM_OK) return st;
  if (n_rows == 0) return PGM_OK;
  *slice = lg_slice_rows(h->p, n_rows);
  *n_slices = (n_rows + *slice - 1) / *slice;
  if (*n_slices > h->p.max_slices)  // lg_slice_rows rules it out
    return pgmi_failf(PGM_EINVAL, "lg_gram: %lld row slices, the handle keeps %lld", (long long)*n_slices, (long long)h->p.max_slices);
  return PGM_OK;
}

// ---------------------------------------------------------------------------- the network handle
int lg_net_build(const int32_t *fam_off, const int32_t *fam_cols, int32_t n, LgNetPlan &out) {
  if (!fam_off || !fam_cols) return pgmi_failf(PGM_EINVAL, "lg_net_create: null fam_off / fam_cols");
  if (n <= 0) return pgmi_failf(PGM_EINVAL, "lg_net_create: %d families", n);
  if (fam_off[0] != 0) return pgmi_failf(PGM_EINVAL, "lg_net_create: fam_off[0] is %d", fam_off[0]);
  LgNetPlan p;
  for (int32_t f = 0; f < n; ++f) {
    const int64_t len = (int64_t)fam_off[f + 1] - fam_off[f];
    if (len < 1) return pgmi_failf(PGM_EINVAL, "lg_net_create: family %d has %lld columns", f, (long long)len);
    if (len - 1 > kLgMaxParents)
      return pgmi_failf(PGM_EINVAL, "lg_net_create: family %d has %lld parents (at most %d)", f, (long long)(len - 1), kLgMaxParents);
    p.max_parents = std::max(p.max_parents, (int32_t)(len - 1));
  }
  if ((int64_t)fam_off[n] + n > INT32_MAX) return pgmi_failf(PGM_EINVAL, "lg_net_create: %d family columns", fam_off[n]);
  for (int32_t k = 0; k < fam_off[n]; ++k) {
    if (fam_cols[k] < 0) return pgmi_failf(PGM_EINVAL, "lg_net_create: column %d", fam_cols[k]);
    p.n_cols = std::max(p.n_cols, fam_cols[k] + 1);
  }
  // node_at[c]: the family whose node column c is, -1: none yet
  std::vector<int32_t> node_at((size_t)p.n_cols, -1), seen((size_t)p.n_cols, -1);
  for (int32_t f = 0; f < n; ++f) {
    const int32_t v = fam_cols[fam_off[f]];
    if (node_at[(size_t)v] >= 0)
      return pgmi_failf(PGM_EINVAL, "lg_net_create: column %d is the node of families %d and %d", v, node_at[(size_t)v], f);
    seen[(size_t)v] = f;
    for (int32_t k = fam_off[f] + 1; k < fam_off[f + 1]; ++k) {
      const int32_t c = fam_cols[k];
      if (seen[(size_t)c] == f) return pgmi_failf(PGM_EINVAL, "lg_net_create: family %d lists column %d twice", f, c);
      seen[(size_t)c] = f;
      if (node_at[(size_t)c] < 0)
        return pgmi_failf(PGM_EINVAL, "lg_net_create: family %d: parent column %d is not the node of an earlier family", f, c);
    }
    node_at[(size_t)v] = f;
  }
  p.fam_off.assign(fam_off, fam_off + n + 1);
  p.fam_cols.assign(fam_cols, fam_cols + fam_off[n]);
  out = std::move(p);
  return PGM_OK;
}

static int lg_blocks(const char *what, int64_t n_rows, int64_t *blocks) {
  *blocks = (n_rows + kLgBlock - 1) / kLgBlock;
  if (*blocks > INT32_MAX) return pgmi_failf(PGM_EINVAL, "%s: %lld rows in one call", what, (long long)n_rows);
  return PGM_OK;
}

int lg_sample_check(const LgNetHandle *h, const double *coef, const double *X, int32_t n_cols, int64_t ld, int64_t row0,
                    int64_t n_rows, int64_t first_row, int64_t *blocks) {
  *blocks = 0;
  if (!h) return pgmi_failf(PGM_EINVAL, "lg_sample: null plan");
  if (!coef) return pgmi_failf(PGM_EINVAL, "lg_sample: null coef");
  const int st = lg_window_check("lg_sample", X, n_cols, h->p.n_cols, ld, row0, n_rows);
  if (st != PGM_OK) return st;
  if (first_row < 0 || first_row > INT64_MAX - n_rows)
    return pgmi_failf(PGM_EINVAL, "lg_sample: first_row %lld", (long long)first_row);
  return lg_blocks("lg_sample", n_rows, blocks);
}

int lg_logpdf_check(const LgNetHandle *h, const double *coef, const double *konst, const double *X, int32_t n_cols, int64_t ld,
                    int64_t row0, int64_t n_rows, const double *logp, const double *total, int64_t *blocks) {
  *blocks = 0;
  if (!h) return pgmi_failf(PGM_EINVAL, "lg_logpdf: null plan");
  if (!coef || !konst) return pgmi_failf(PGM_EINVAL, "lg_logpdf: null coef / konst");
  if (!logp && !total) return pgmi_failf(PGM_EINVAL, "lg_logpdf: null logp and total");
  const int st = lg_window_check("lg_logpdf", X, n_cols, h->p.n_cols, ld, row0, n_rows);
  if (st != PGM_OK) return st;
  const int bl = lg_blocks("lg_logpdf", n_rows, blocks);
  if (bl != PGM_OK) return bl;
  if (*blocks > kLgMaxBlocks)
    return pgmi_failf(PGM_EINVAL, "lg_logpdf: %lld rows in one call (at most %lld)", (long long)n_rows,
                      (long long)(kLgMaxBlocks * kLgBlock));
  return PGM_OK;
}

int lg_affine_check(const double *W, const double *c, const int32_t *in_cols, int32_t n_in, int32_t n_out, const double *X,
                    int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, const double *out, int64_t ld_out,
                    int64_t *blocks) {
  *blocks = 0;
  if (!W || !c || !out) return pgmi_failf(PGM_EINVAL, "lg_affine: null W / c / out");
  if (n_in < 0 || (n_in > 0 && !in_cols)) return pgmi_failf(PGM_EINVAL, "lg_affine: %d input columns, null in_cols", n_in);
  if (n_out < 1 || n_out > 65535) return pgmi_failf(PGM_EINVAL, "lg_affine: %d outputs (1 .. 65535)", n_out);
  int32_t top = 0;
  for (int32_t i = 0; i < n_in; ++i) {
    if (in_cols[i] < 0) return pgmi_failf(PGM_EINVAL, "lg_affine: input %d is column %d", i, in_cols[i]);
    top = std::max(top, in_cols[i] + 1);
  }
  const int st = lg_window_check("lg_affine", X, n_cols, top, ld, row0, n_rows);
  if (st != PGM_OK) return st;
  if (ld_out < n_rows) return pgmi_failf(PGM_EINVAL, "lg_affine: ld_out %lld < n_rows %lld", (long long)ld_out, (long long)n_rows);
  return lg_blocks("lg_affine", n_rows, blocks);
}

extern "C" {

int pgm_lg_gram_plan_create(const int32_t *cols, int32_t d, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "lg_gram_plan_create: null plan");
  *plan = nullptr;
  LgGramHandle *h = new (std::nothrow) LgGramHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "lg_gram_plan_create: out of memory");
  const int st = lg_gram_plan_build(cols, d, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_lg_gram_plan_info(void *plan, pgm_lg_gram_info_t *info, int32_t *groups) {
  const LgGramHandle *h = static_cast<const LgGramHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "lg_gram_plan_info: null plan");
  const LgGramPlan &p = h->p;
  if (info) {
    info->d = p.d;
    info->n_cols = p.n_cols;
    info->n_tiles = p.n_tiles;
    info->n_super = p.n_super;
    info->single_wave = p.n_super == 1 ? 1 : 0;
    info->reserved = 0;
    info->n_groups = (int64_t)p.groups.size();
    info->n_tile_pairs = p.n_tile_pairs;
    info->out_size = (int64_t)(p.d + 1) * (p.d + 1);
    info->max_slices = p.max_slices;
    info->slice_rows = p.slice_rows;
  }
  if (groups)
    for (size_t g = 0; g < p.groups.size(); ++g) {
      groups[2 * g] = p.groups[g].I;
      groups[2 * g + 1] = p.groups[g].J;
    }
  return PGM_OK;
}

int pgm_lg_gram_plan_set_slice(void *plan, int64_t slice_rows) {
  LgGramHandle *h = static_cast<LgGramHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "lg_gram_plan_set_slice: null plan");
  if (slice_rows < 0 || slice_rows > kLgSliceMax)
    return pgmi_failf(PGM_EINVAL, "lg_gram_plan_set_slice: %lld rows (0 .. %lld)", (long long)slice_rows, (long long)kLgSliceMax);
  h->p.slice_rows = slice_rows;
  return PGM_OK;
}

int pgm_lg_gram_info(void *plan, const void *X, int64_t ld, int64_t row0, int64_t n_rows, int64_t *slice_rows,
                     int64_t *n_slices, int32_t *vec16) {
  const LgGramHandle *h = static_cast<const LgGramHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "lg_gram_info: null plan");
  if (n_rows < 0) return pgmi_failf(PGM_EINVAL, "lg_gram_info: n_rows %lld", (long long)n_rows);
  const int64_t slice = lg_slice_rows(h->p, n_rows);
  if (slice_rows) *slice_rows = slice;
  if (n_slices) *n_slices = (n_rows + slice - 1) / slice;
  if (vec16) *vec16 = lg_vec16(X, ld, row0) ? 1 : 0;
  return PGM_OK;
}

int pgm_lg_net_create(const int32_t *fam_off, const int32_t *fam_cols, int32_t n_families, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "lg_net_create: null plan");
  *plan = nullptr;
  LgNetHandle *h = new (std::nothrow) LgNetHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "lg_net_create: out of memory");
  const int st = lg_net_build(fam_off, fam_cols, n_families, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_lg_net_info(void *plan, pgm_lg_net_info_t *info, int64_t *coef_off) {
  const LgNetHandle *h = static_cast<const LgNetHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "lg_net_info: null plan");
  const LgNetPlan &p = h->p;
  const int32_t n = (int32_t)p.fam_off.size() - 1;
  if (info) {
    info->n_families = n;
    info->n_cols = p.n_cols;
    info->max_parents = p.max_parents;
    info->reserved = 0;
    info->n_coef = (int64_t)p.fam_off[(size_t)n] + n;
  }
  if (coef_off)
    for (int32_t f = 0; f < n; ++f) coef_off[f] = (int64_t)p.fam_off[(size_t)f] + f;
  return PGM_OK;
}
}

// pgmpair_plan.cpp — the host side of the pairwise counts (include/pgmhip.h "pairwise counts"): validation
// of the variables, the state table, the tile-pair and group lists, the choice of the row slice and the
// argument checks of the pgm_pair_* entry points.  No HIP call and no HIP include: a stand-alone CPU program
// drives all of it (tools/pair_plan_selftest.cpp).  The kernels and launches are pgmpair.hip.
#include <algorithm>
#include <new>

#include "pgm_pair.h"

int pair_plan_build(const int32_t *cols, const int32_t *cards, int32_t n_vars, PairPlan &out) {
  if (!cols || !cards) return pgmi_failf(PGM_EINVAL, "pair_plan_create: null cols / cards");
  if (n_vars <= 0) return pgmi_failf(PGM_EINVAL, "pair_plan_create: %d variables", n_vars);
  PairPlan p;
  p.off.assign(1, 0);
  for (int32_t v = 0; v < n_vars; ++v) {
    if (cards[v] < 1 || cards[v] > kPairMaxCard)
      return pgmi_failf(PGM_EINVAL, "pair_plan_create: variable %d cardinality %d (1 .. %d)", v, cards[v], kPairMaxCard);
    if (cols[v] < 0) return pgmi_failf(PGM_EINVAL, "pair_plan_create: variable %d column %d", v, cols[v]);
    p.n_cols = std::max(p.n_cols, cols[v] + 1);
    p.off.push_back(p.off.back() + cards[v]);
  }
  {  // a column listed twice would make two variables of one: every pair table is between different columns
    std::vector<int32_t> sorted(cols, cols + n_vars);
    std::sort(sorted.begin(), sorted.end());
    for (int32_t v = 1; v < n_vars; ++v)
      if (sorted[v] == sorted[v - 1])
        return pgmi_failf(PGM_EINVAL, "pair_plan_create: column %d is listed twice", sorted[v]);
  }
  p.cols.assign(cols, cols + n_vars);
  p.cards.assign(cards, cards + n_vars);
  p.S = p.off.back();
  p.Sp = (p.S + kPairTile - 1) / kPairTile * kPairTile;
  const int64_t n_super = (p.S + kPairSuperStates - 1) / kPairSuperStates;
  const int64_t n_tiles = p.Sp / kPairTile;
  // the state table, padded to whole super-tiles
  p.states.assign((size_t)(n_super * kPairSuperStates), PairState{0, 0, 1, 1});
  std::vector<int32_t> var_of((size_t)p.S);
  for (int32_t v = 0; v < n_vars; ++v)
    for (int32_t k = 0; k < cards[v]; ++k) {
      p.states[(size_t)(p.off[v] + k)] = PairState{cols[v], k, cards[v], 0};
      var_of[(size_t)(p.off[v] + k)] = v;
    }
  // a tile pair is needed when its states belong to more than one variable
  auto first_var = [&](int64_t t) { return var_of[(size_t)(t * kPairTile)]; };
  auto last_var = [&](int64_t t) { return var_of[(size_t)std::min<int64_t>(p.S, (t + 1) * kPairTile) - 1]; };
  std::vector<uint8_t> group_needed((size_t)(n_super * n_super), 0);
  for (int64_t ti = 0; ti < n_tiles; ++ti)
    for (int64_t tj = ti; tj < n_tiles; ++tj) {
      if (first_var(ti) == last_var(tj)) continue;  // states are in variable order: one variable throughout
      p.tile_pairs.push_back((int32_t)ti);
      p.tile_pairs.push_back((int32_t)tj);
      group_needed[(size_t)((ti / kPairSuper) * n_super + tj / kPairSuper)] = 1;
    }
  std::vector<uint8_t> checked((size_t)n_super, 0);
  for (int64_t I = 0; I < n_super; ++I)
    for (int64_t J = I; J < n_super; ++J)
      if (group_needed[(size_t)(I * n_super + J)]) p.groups.push_back(PairGroup{(int32_t)I, (int32_t)J, 0, 0});
  // every super-tile in a group checks its codes exactly once: on the B side where it has one, else on the A side
  for (PairGroup &g : p.groups)
    if (!checked[(size_t)g.J]) {
      g.check |= 2;
      checked[(size_t)g.J] = 1;
    }
  for (PairGroup &g : p.groups)
    if (!checked[(size_t)g.I]) {
      g.check |= 1;
      checked[(size_t)g.I] = 1;
    }
  for (int32_t u = 0; u < n_vars; ++u)
    for (int32_t v = u + 1; v < n_vars; ++v)
      p.pairs.push_back(PairVars{(int32_t)p.off[u], (int32_t)p.off[v], cards[u], cards[v]});
  out = std::move(p);
  return PGM_OK;
}

int64_t pair_slice_rows(const PairPlan &p, int64_t n_rows, int32_t n_strata) {
  auto round_up = [](int64_t x) { return (x + kPairSliceQuantum - 1) / kPairSliceQuantum * kPairSliceQuantum; };
  int64_t slice;
  if (p.slice_rows > 0) {
    slice = round_up(p.slice_rows);
  } else {
    const int64_t per = std::max<int64_t>(1, (int64_t)p.groups.size() * n_strata);
    const int64_t want = std::max<int64_t>(1, kPairTargetBlocks / per);  // slices that give every CU work
    slice = round_up(std::max<int64_t>(1, (n_rows + want - 1) / want));
  }
  // grid.y
  slice = std::max(slice, round_up((n_rows + kPairMaxSlices - 1) / kPairMaxSlices));
  return std::min(slice, kPairSliceMax);
}

bool pair_codes_vec16(const void *codes, int64_t ld, int64_t row0) {
  return ((uintptr_t)codes % 16 == 0) && ld % 16 == 0 && row0 % 16 == 0;
}

int pair_count_check(const PairHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                     int32_t strat_col, int32_t n_strata, const int64_t *counts, int64_t *slice, int64_t *n_slices) {
  *slice = *n_slices = 0;
  if (!h) return pgmi_failf(PGM_EINVAL, "pair_count: null plan");
  if (!codes || !counts) return pgmi_failf(PGM_EINVAL, "pair_count: null codes / counts");
  if (n_rows < 0 || row0 < 0)
    return pgmi_failf(PGM_EINVAL, "pair_count: n_rows %lld row0 %lld", (long long)n_rows, (long long)row0);
  if (ld < 0 || row0 > ld || n_rows > ld - row0)
    return pgmi_failf(PGM_EINVAL, "pair_count: rows [%lld, %lld) outside ld %lld", (long long)row0,
                      (long long)(row0 + n_rows), (long long)ld);
  if (h->p.n_cols > n_cols)
    return pgmi_failf(PGM_EINVAL, "pair_count: the plan reads column %d, codes has %d columns", h->p.n_cols - 1, n_cols);
  if (strat_col < -1 || strat_col >= n_cols)
    return pgmi_failf(PGM_EINVAL, "pair_count: stratum column %d, codes has %d columns", strat_col, n_cols);
  if (n_strata < 1 || n_strata > kPairMaxCard || (strat_col < 0 && n_strata != 1))
    return pgmi_failf(PGM_EINVAL, "pair_count: %d strata (1 .. %d; 1 without a stratum column)", n_strata, kPairMaxCard);
  if (n_rows == 0 || h->p.groups.empty()) return PGM_OK;
  *slice = pair_slice_rows(h->p, n_rows, n_strata);
  *n_slices = (n_rows + *slice - 1) / *slice;
  if (*n_slices > kPairMaxSlices)
    return pgmi_failf(PGM_EINVAL, "pair_count: %lld row slices (count the rows in several calls)", (long long)*n_slices);
  if ((int64_t)h->p.groups.size() > INT32_MAX)
    return pgmi_failf(PGM_EINVAL, "pair_count: %lld tile groups", (long long)h->p.groups.size());
  return PGM_OK;
}

int pair_stat_check(const char *what, const PairHandle *h, const int64_t *counts, int32_t n_strata,
                    const void *const *outs, int n_outs) {
  if (!h) return pgmi_failf(PGM_EINVAL, "%s: null plan", what);
  if (!counts) return pgmi_failf(PGM_EINVAL, "%s: null counts", what);
  for (int i = 0; i < n_outs; ++i)
    if (!outs[i]) return pgmi_failf(PGM_EINVAL, "%s: null output %d", what, i);
  if (n_strata < 1 || n_strata > kPairMaxCard)
    return pgmi_failf(PGM_EINVAL, "%s: %d strata (1 .. %d)", what, n_strata, kPairMaxCard);
  if ((int64_t)h->p.pairs.size() > INT32_MAX) return pgmi_failf(PGM_EINVAL, "%s: %lld pairs", what, (long long)h->p.pairs.size());
  return PGM_OK;
}

extern "C" {

int pgm_pair_plan_create(const int32_t *cols, const int32_t *cards, int32_t n_vars, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "pair_plan_create: null plan");
  *plan = nullptr;
  PairHandle *h = new (std::nothrow) PairHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "pair_plan_create: out of memory");
  const int st = pair_plan_build(cols, cards, n_vars, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_pair_plan_info(void *plan, pgm_pair_info_t *info, int64_t *offsets, int32_t *tile_pairs, int32_t *groups) {
  const PairHandle *h = static_cast<const PairHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "pair_plan_info: null plan");
  const PairPlan &p = h->p;
  if (info) {
    info->n_vars = (int32_t)p.cols.size();
    info->n_cols = p.n_cols;
    info->S = p.S;
    info->Sp = p.Sp;
    info->table_size = p.Sp * p.Sp;
    info->n_pairs = (int64_t)p.pairs.size();
    info->n_tile_pairs = (int64_t)p.tile_pairs.size() / 2;
    info->n_groups = (int64_t)p.groups.size();
    info->n_state_entries = (int64_t)p.states.size();
    info->slice_rows = p.slice_rows;
  }
  if (offsets) std::copy(p.off.begin(), p.off.end(), offsets);
  if (tile_pairs) std::copy(p.tile_pairs.begin(), p.tile_pairs.end(), tile_pairs);
  if (groups)
    for (size_t g = 0; g < p.groups.size(); ++g) {
      groups[3 * g] = p.groups[g].I;
      groups[3 * g + 1] = p.groups[g].J;
      groups[3 * g + 2] = p.groups[g].check;
    }
  return PGM_OK;
}

int pgm_pair_plan_set_slice(void *plan, int64_t slice_rows) {
  PairHandle *h = static_cast<PairHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "pair_plan_set_slice: null plan");
  if (slice_rows < 0 || slice_rows > kPairSliceMax)
    return pgmi_failf(PGM_EINVAL, "pair_plan_set_slice: %lld rows (0 .. %lld)", (long long)slice_rows, (long long)kPairSliceMax);
  h->p.slice_rows = slice_rows;
  return PGM_OK;
}

int pgm_pair_count_info(void *plan, const void *codes, int64_t ld, int64_t row0, int64_t n_rows, int32_t n_strata,
                        int64_t *slice_rows, int64_t *n_slices, int32_t *vec16) {
  const PairHandle *h = static_cast<const PairHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "pair_count_info: null plan");
  if (n_rows < 0 || n_strata < 1) return pgmi_failf(PGM_EINVAL, "pair_count_info: n_rows %lld, %d strata", (long long)n_rows, n_strata);
  const int64_t slice = pair_slice_rows(h->p, n_rows, n_strata);
  if (slice_rows) *slice_rows = slice;
  if (n_slices) *n_slices = (n_rows + slice - 1) / slice;
  if (vec16) *vec16 = pair_codes_vec16(codes, ld, row0) ? 1 : 0;
  return PGM_OK;
}
}

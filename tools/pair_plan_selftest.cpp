// pair_plan_selftest.cpp — the host side of the pairwise counts (pgmpy_amd/csrc/pgmpair_plan.cpp: the
// validation of the variables, the state table, the tile-pair and group lists, the choice of the row slice
// and the argument checks of pgm_pair_count / pgm_pair_mi) on the CPU, at the edge shapes of the tests.
// Links that unit alone; meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I include -I pgmpy_amd/csrc
//       tools/pair_plan_selftest.cpp pgmpy_amd/csrc/pgmpair_plan.cpp -o pair_plan_selftest
// Exit status 0 and "pair_plan_selftest ok" when every check holds.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "pgmhip.h"
#include "pgm_internal.h"
#include "pgm_pair.h"

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

// ---------------------------------------------------------------------------- the library's error hooks
static std::string g_last_err;

extern "C" int pgmi_fail(int code, const char *msg) {
  g_last_err = msg;
  return code;
}

extern "C" int pgmi_failf(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_err = buf;
  return code;
}

static bool err_has(const char *text) { return g_last_err.find(text) != std::string::npos; }

static int build(const std::vector<int32_t> &cols, const std::vector<int32_t> &cards, PairPlan &p) {
  return pair_plan_build(cols.data(), cards.data(), (int32_t)cols.size(), p);
}

// the lists against their definitions, by brute force over the states
static int check_lists(const PairPlan &p) {
  const int64_t n_tiles = p.Sp / kPairTile;
  CHECK(p.Sp % kPairTile == 0 && p.Sp >= p.S && p.Sp - p.S < kPairTile);
  CHECK((int64_t)p.states.size() % kPairSuperStates == 0 && (int64_t)p.states.size() >= p.S &&
        (int64_t)p.states.size() - p.S < kPairSuperStates);
  std::vector<int> var_of((size_t)p.S);
  for (size_t v = 0; v < p.cols.size(); ++v)
    for (int32_t k = 0; k < p.cards[v]; ++k) {
      const PairState &s = p.states[(size_t)(p.off[v] + k)];
      CHECK(s.col == p.cols[v] && s.k == k && s.card == p.cards[v] && s.pad == 0);
      var_of[(size_t)(p.off[v] + k)] = (int)v;
    }
  for (size_t s = (size_t)p.S; s < p.states.size(); ++s) CHECK(p.states[s].pad == 1);
  std::set<std::pair<int, int>> want_tiles, got_tiles, want_groups, got_groups;
  for (int64_t s = 0; s < p.S; ++s)
    for (int64_t t = s; t < p.S; ++t)
      if (var_of[(size_t)s] != var_of[(size_t)t]) {
        want_tiles.insert({(int)(s / kPairTile), (int)(t / kPairTile)});
        want_groups.insert({(int)(s / kPairSuperStates), (int)(t / kPairSuperStates)});
      }
  for (size_t i = 0; i + 1 < p.tile_pairs.size(); i += 2) {
    CHECK(p.tile_pairs[i] <= p.tile_pairs[i + 1] && p.tile_pairs[i + 1] < n_tiles);
    CHECK(got_tiles.insert({p.tile_pairs[i], p.tile_pairs[i + 1]}).second);
  }
  CHECK(got_tiles == want_tiles);
  std::multiset<int> checks;
  std::set<int> in_group;
  for (const PairGroup &g : p.groups) {
    CHECK(g.I <= g.J && (int64_t)(g.J + 1) * kPairSuperStates <= (int64_t)p.states.size());
    CHECK(got_groups.insert({g.I, g.J}).second);
    in_group.insert(g.I);
    in_group.insert(g.J);
    if (g.check & 1) checks.insert(g.I);
    if (g.check & 2) checks.insert(g.J);
  }
  CHECK(got_groups == want_groups);
  CHECK(checks.size() == in_group.size() && std::set<int>(checks.begin(), checks.end()) == in_group);  // each once
  const size_t n = p.cols.size();
  CHECK(p.pairs.size() == n * (n - 1) / 2);
  size_t i = 0;
  for (size_t u = 0; u < n; ++u)
    for (size_t v = u + 1; v < n; ++v, ++i)
      CHECK(p.pairs[i].off_u == p.off[u] && p.pairs[i].off_v == p.off[v] && p.pairs[i].card_u == p.cards[u] &&
            p.pairs[i].card_v == p.cards[v]);
  return 0;
}

static int test_layouts() {
  const std::vector<std::vector<int32_t>> shapes = {
      {2, 3, 4}, {8, 8}, {8, 8, 1}, {15, 3, 15}, {1, 5, 1, 9}, {254, 2}, {2, 254, 3}, {60, 7, 60, 5, 70}, {1, 1}, {5},
      {254, 254, 254}, {16, 16, 16, 16, 16}};
  for (const auto &cards : shapes) {
    std::vector<int32_t> cols(cards.size());
    for (size_t v = 0; v < cols.size(); ++v) cols[v] = (int32_t)(cols.size() - 1 - v) * 3;
    PairPlan p;
    CHECK(build(cols, cards, p) == PGM_OK);
    CHECK(p.n_cols == (int32_t)(cols.size() - 1) * 3 + 1);
    if (check_lists(p)) return 1;
  }
  PairPlan p;
  CHECK(build({0, 1, 2}, {8, 8, 1}, p) == PGM_OK && p.S == 17 && p.Sp == 32 && p.states.size() == 64);
  CHECK(build({0, 1, 2}, {15, 3, 15}, p) == PGM_OK && p.S == 33 && p.Sp == 48 && p.tile_pairs.size() == 10);
  CHECK(build({0, 1}, {254, 2}, p) == PGM_OK && p.Sp == 256 && p.tile_pairs.size() == 32 && p.groups.size() == 4);
  CHECK(build({7}, {5}, p) == PGM_OK && p.groups.empty() && p.pairs.empty() && p.tile_pairs.empty());
  return 0;
}

static int test_validation() {
  PairPlan p;
  CHECK(build({0, 1}, {2, 0}, p) == PGM_EINVAL && err_has("variable 1 cardinality 0 (1 .. 254)"));
  CHECK(build({0, 1}, {255, 2}, p) == PGM_EINVAL && err_has("variable 0 cardinality 255"));
  CHECK(build({3, 1, 3}, {2, 2, 2}, p) == PGM_EINVAL && err_has("column 3 is listed twice"));
  CHECK(build({0, -1}, {2, 2}, p) == PGM_EINVAL && err_has("variable 1 column -1"));
  CHECK(pair_plan_build(nullptr, nullptr, 2, p) == PGM_EINVAL && err_has("null cols / cards"));
  const int32_t c = 0, k = 2;
  CHECK(pair_plan_build(&c, &k, 0, p) == PGM_EINVAL && err_has("0 variables"));
  void *h = nullptr;
  CHECK(pgm_pair_plan_create(&c, &k, 1, nullptr) == PGM_EINVAL);
  CHECK(pgm_pair_plan_create(&c, &k, 0, &h) == PGM_EINVAL && h == nullptr);
  return 0;
}

static int test_slices() {
  PairPlan p;
  std::vector<int32_t> cols(37), cards(37, 3);
  for (int v = 0; v < 37; ++v) cols[v] = v;
  CHECK(build(cols, cards, p) == PGM_OK && p.groups.size() == 3);
  const int64_t rows[] = {1, 255, 256, 257, 70000, 1000000, 3000000000ll, (int64_t)1 << 40};
  for (int64_t n : rows)
    for (int32_t strata : {1, 3, 254}) {
      const int64_t s = pair_slice_rows(p, n, strata);
      CHECK(s % kPairSliceQuantum == 0 && s >= kPairSliceQuantum && s <= kPairSliceMax);
      if (n <= kPairSliceMax * kPairMaxSlices / 2) CHECK((n + s - 1) / s <= kPairMaxSlices);
    }
  CHECK(pair_slice_rows(p, 70000, 1) == 256 && pair_slice_rows(p, 1000000, 1) == 3072);
  p.slice_rows = 1000;
  CHECK(pair_slice_rows(p, 70000, 1) == 1024);
  p.slice_rows = 1;
  CHECK(pair_slice_rows(p, 100000000, 1) == 1536);  // grid.y caps the number of slices
  CHECK(pair_codes_vec16((const void *)4096, 1024, 16) && !pair_codes_vec16((const void *)4096, 1003, 0) &&
        !pair_codes_vec16((const void *)4096, 1024, 3) && !pair_codes_vec16((const void *)4100, 1024, 0));
  return 0;
}

static int test_checks() {
  const int32_t cols[] = {0, 1, 2}, cards[] = {2, 3, 4};
  void *plan = nullptr;
  CHECK(pgm_pair_plan_create(cols, cards, 3, &plan) == PGM_OK && plan);
  PairHandle *h = static_cast<PairHandle *>(plan);
  pgm_pair_info_t info;
  int64_t off[4];
  int32_t tiles[2], groups[3];
  CHECK(pgm_pair_plan_info(plan, &info, off, tiles, groups) == PGM_OK);
  CHECK(info.S == 9 && info.Sp == 16 && info.table_size == 256 && info.n_pairs == 3 && info.n_tile_pairs == 1 &&
        info.n_groups == 1 && info.n_state_entries == 64 && info.n_cols == 3 && info.n_vars == 3);
  CHECK(off[0] == 0 && off[1] == 2 && off[2] == 5 && off[3] == 9 && tiles[0] == 0 && tiles[1] == 0 && groups[2] == 2);
  const uint8_t *codes = reinterpret_cast<const uint8_t *>(64);
  const int64_t *counts = reinterpret_cast<const int64_t *>(64);
  int64_t slice = 0, n = 0;
  CHECK(pair_count_check(h, codes, 3, 100, 0, 100, -1, 1, counts, &slice, &n) == PGM_OK && slice == 256 && n == 1);
  CHECK(pair_count_check(h, codes, 3, 100, 0, 0, -1, 1, counts, &slice, &n) == PGM_OK && n == 0);
  CHECK(pair_count_check(h, codes, 3, 100, 0, 100, 3, 1, counts, &slice, &n) == PGM_EINVAL && err_has("stratum column 3"));
  CHECK(pair_count_check(h, codes, 3, 100, 0, 100, -1, 2, counts, &slice, &n) == PGM_EINVAL && err_has("2 strata"));
  CHECK(pair_count_check(h, codes, 3, 100, 0, 100, 1, 255, counts, &slice, &n) == PGM_EINVAL);
  CHECK(pair_count_check(h, codes, 2, 100, 0, 100, -1, 1, counts, &slice, &n) == PGM_EINVAL && err_has("reads column 2"));
  CHECK(pair_count_check(h, codes, 3, 100, 1, 100, -1, 1, counts, &slice, &n) == PGM_EINVAL && err_has("outside ld"));
  CHECK(pair_count_check(h, nullptr, 3, 100, 0, 100, -1, 1, counts, &slice, &n) == PGM_EINVAL);
  CHECK(pair_count_check(nullptr, codes, 3, 100, 0, 100, -1, 1, counts, &slice, &n) == PGM_EINVAL);
  const void *outs[] = {counts, nullptr};
  CHECK(pair_stat_check("pair_mi", h, counts, 1, outs, 1) == PGM_OK);
  CHECK(pair_stat_check("pair_mi", h, counts, 1, outs, 2) == PGM_EINVAL && err_has("null output 1"));
  CHECK(pair_stat_check("pair_mi", h, counts, 0, outs, 1) == PGM_EINVAL);
  CHECK(pgm_pair_plan_set_slice(plan, 512) == PGM_OK && pgm_pair_plan_set_slice(plan, -1) == PGM_EINVAL);
  int32_t vec = -1;
  CHECK(pgm_pair_count_info(plan, codes, 1024, 0, 5000, 1, &slice, &n, &vec) == PGM_OK && slice == 512 && n == 10 && vec == 1);
  delete h;  // the device side was never used
  return 0;
}

int main() {
  if (test_layouts() || test_validation() || test_slices() || test_checks()) return 1;
  printf("pair_plan_selftest ok\n");
  return 0;
}

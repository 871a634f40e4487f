// gibbs_plan_selftest.cpp — the host side of Gibbs sampling (pgmpy_amd/csrc/pgmgibbs_plan.cpp: factor
// validation, the incidence lists, the argument checks of pgm_gibbs_sweep / pgm_gibbs_start, the choice of
// the kernel path) and the sweep coordinate of the random stream (pgm_sample.h) on the CPU.  Links the two
// host units alone; meant for a plain and for a sanitizer build:
//   c++ -std=c++17 -g [-fsanitize=address,undefined] -I include -I pgmpy_amd/csrc
//       tools/gibbs_plan_selftest.cpp pgmpy_amd/csrc/pgmgibbs_plan.cpp pgmpy_amd/csrc/pgmfit_plan.cpp
//       -o gibbs_plan_selftest
// Exit status 0 and "gibbs_plan_selftest ok" when every check holds.  `--uniform3 SEED CHAIN COL SWEEP`
// prints the 53-bit integer behind that uniform: the test suite compares it with its numpy restatement.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pgm_gibbs.h"
#include "pgm_internal.h"
#include "pgmhip.h"

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

static pgm_fit_family factor(std::vector<int> cols, std::vector<int> cards) {
  pgm_fit_family f;
  memset(&f, 0, sizeof f);
  f.n_vars = (int32_t)cols.size();
  for (size_t v = 0; v < cols.size() && v < PGM_MAX_DIMS; ++v) f.col[v] = cols[v], f.card[v] = cards[v];
  return f;
}

// ---------------------------------------------------------------------------- the stream
static int test_stream() {
  // sweep 0 is the forward sampler's stream
  for (uint64_t r : {0ull, 5ull, 0xffffffffull, 1ull << 32, (1ull << 62) + 17})
    for (uint32_t c : {0u, 1u, 36u, 1041u})
      CHECK(sample_uniform3(12345, r, c, 0) == sample_uniform(12345, r, c));
  // the sweep is the fourth counter word; the words of a column pair are shared as before
  uint32_t x[4];
  philox4x32_10(7, 1, 3, 0xffffffffu, 9, 2, x);
  const uint64_t seed = ((uint64_t)2 << 32) | 9, chain = ((uint64_t)1 << 32) | 7;
  CHECK(sample_uniform3(seed, chain, 6, 0xffffffffu) == (double)(((uint64_t)x[0] << 21) | (x[1] >> 11)) * 0x1.0p-53);
  CHECK(sample_uniform3(seed, chain, 7, 0xffffffffu) == (double)(((uint64_t)x[2] << 21) | (x[3] >> 11)) * 0x1.0p-53);
  CHECK(sample_uniform3(seed, chain, 6, 1) != sample_uniform3(seed, chain, 6, 2));
  for (uint32_t j = 1; j < 2000; ++j) {
    const double u = sample_uniform3(77, j * 0x100000001ull, j % 77, j * 2654435761u | 1u);
    CHECK(u >= 0.0 && u < 1.0);
  }
  return 0;
}

// ---------------------------------------------------------------------------- accepted and rejected factors
static int test_plan() {
  // a CPD-style set: P(c3), P(c0 | c3), P(c2 | c3), P(c1 | c0, c2)
  const pgm_fit_family fs[] = {factor({3}, {2}), factor({0, 3}, {3, 2}), factor({2, 3}, {4, 2}), factor({1, 0, 2}, {2, 3, 4})};
  const int32_t card[] = {3, 2, 4, 2};
  GibbsPlan p;
  CHECK(gibbs_plan_build(fs, 4, card, 4, p) == PGM_OK);
  CHECK(p.n_cols == 4 && p.fit.total_bins == 2 + 6 + 8 + 24 && p.max_degree == 3 && p.max_card == 4);
  const int32_t inc_off[5] = {0, 2, 3, 5, 8};
  CHECK(memcmp(p.inc_off.data(), inc_off, sizeof inc_off) == 0);
  // column 0: factor 1 at position 0 (stride 2), factor 3 at position 1 (stride 4)
  CHECK(p.inc[0].factor == 1 && p.inc_pos[0] == 0 && p.inc[0].stride == 2 && p.inc[0].off == 2);
  CHECK(p.inc[1].factor == 3 && p.inc_pos[1] == 1 && p.inc[1].stride == 4 && p.inc[1].off == 16);
  CHECK(p.inc[1].other_end - p.inc[1].other_begin == 2);
  const GibbsOther *o = &p.others[(size_t)p.inc[1].other_begin];
  CHECK(o[0].col == 1 && o[0].stride == 12 && o[1].col == 2 && o[1].stride == 1);
  // column 3: factors 0, 1, 2 ascending
  CHECK(p.inc[5].factor == 0 && p.inc[6].factor == 1 && p.inc[7].factor == 2 && p.inc_pos[6] == 1);
  CHECK(p.inc[5].other_begin == p.inc[5].other_end);
  for (size_t e = 0; e < p.inc.size(); ++e) CHECK(p.inc[e].other_end <= (int32_t)p.others.size());
  CHECK(gibbs_lds_path(p));
  // a Markov-style set: a column in many factors (no bound on the degree), columns in any order
  std::vector<pgm_fit_family> star;
  std::vector<int32_t> scard(41, 2);
  scard[0] = 254;
  for (int v = 1; v <= 40; ++v) star.push_back(factor({v, 0}, {2, 254}));
  CHECK(gibbs_plan_build(star.data(), 40, scard.data(), 41, p) == PGM_OK);
  CHECK(p.max_degree == 40 && p.max_card == 254 && p.inc_off[1] == 40 && p.inc[39].factor == 39 && p.inc[39].stride == 1);
  // the path: n_cols * kGibbsBlock bytes against the budget
  const int32_t edge = kGibbsLdsBudget / kGibbsBlock;
  for (int32_t n : {edge, edge + 1}) {
    std::vector<pgm_fit_family> single;
    std::vector<int32_t> c2((size_t)n, 2);
    for (int v = 0; v < n; ++v) single.push_back(factor({v}, {2}));
    CHECK(gibbs_plan_build(single.data(), n, c2.data(), n, p) == PGM_OK);
    CHECK(gibbs_lds_path(p) == (n == edge));
  }
  return 0;
}

static int rejected(const pgm_fit_family *fs, int n, const int32_t *card, int n_cols, const char *msg) {
  GibbsPlan p;
  g_last_err.clear();
  const int st = gibbs_plan_build(fs, n, card, n_cols, p);
  if (st != PGM_EINVAL || g_last_err != msg) {
    fprintf(stderr, "expected PGM_EINVAL \"%s\"\n     got %d \"%s\"\n", msg, st, g_last_err.c_str());
    return 1;
  }
  return 0;
}

static int test_rejected() {
  const int32_t c22[] = {2, 2}, c23[] = {2, 3}, c255[] = {255}, c0[] = {0};
  pgm_fit_family f = factor({0}, {2});
  CHECK(!rejected(nullptr, 1, c22, 1, "gibbs_plan_create: null factors"));
  CHECK(!rejected(&f, 1, nullptr, 1, "gibbs_plan_create: null cardinalities"));
  CHECK(!rejected(&f, 0, c22, 1, "gibbs_plan_create: 0 factors"));
  CHECK(!rejected(&f, 1, c22, 0, "gibbs_plan_create: 0 columns"));
  CHECK(!rejected(&f, 1, c22, 2, "gibbs_plan_create: column 1 is in no factor"));
  CHECK(!rejected(&f, 1, c23 + 1, 1, "gibbs_plan_create: factor 0 column 0 cardinality 2, the column has 3"));
  const pgm_fit_family differ[] = {factor({0, 1}, {2, 2}), factor({1}, {3})};
  CHECK(!rejected(differ, 2, c22, 2, "gibbs_plan_create: factor 1 column 1 cardinality 3, the column has 2"));
  f = factor({0}, {255});
  CHECK(!rejected(&f, 1, c255, 1, "gibbs_plan_create: column 0 cardinality 255 (1 .. 254)"));
  f = factor({0}, {0});
  CHECK(!rejected(&f, 1, c0, 1, "gibbs_plan_create: column 0 cardinality 0 (1 .. 254)"));
  f = factor({0}, {2});
  f.n_vars = PGM_MAX_DIMS + 1;
  CHECK(!rejected(&f, 1, c22, 1, "gibbs_plan_create: factor 0 has 33 columns (1 .. 32)"));
  f.n_vars = 0;
  CHECK(!rejected(&f, 1, c22, 1, "gibbs_plan_create: factor 0 has 0 columns (1 .. 32)"));
  f = factor({2}, {2});
  CHECK(!rejected(&f, 1, c22, 2, "gibbs_plan_create: factor 0 position 0 column 2 (0 .. 1)"));
  f = factor({-1}, {2});
  CHECK(!rejected(&f, 1, c22, 2, "gibbs_plan_create: factor 0 position 0 column -1 (0 .. 1)"));
  f = factor({0, 1, 0}, {2, 2, 2});
  CHECK(!rejected(&f, 1, c22, 2, "gibbs_plan_create: factor 0 lists column 0 twice"));
  // 2^31 entries: past the fit plan's table limit
  std::vector<int> cols, cards;
  std::vector<int32_t> c31(31, 2);
  for (int v = 0; v < 31; ++v) cols.push_back(v), cards.push_back(2);
  f = factor(cols, cards);
  CHECK(!rejected(&f, 1, c31.data(), 31, "fit_plan_create: family 0 table exceeds 2^31 - 1 bins"));
  return 0;
}

// ---------------------------------------------------------------------------- argument checks
static int test_argument_checks() {
  const pgm_fit_family fs[] = {factor({0}, {3}), factor({2, 0}, {2, 3}), factor({1, 2}, {2, 2})};
  const int32_t card[] = {3, 2, 2};
  GibbsHandle h;
  CHECK(gibbs_plan_build(fs, 3, card, 3, h.p) == PGM_OK);
  const double *values = (const double *)0x30000;  // only inspected
  const uint8_t *codes = (const uint8_t *)0x10000, *trace = (const uint8_t *)0x20000;
  int64_t blocks = -1;
  const int64_t last = (int64_t)UINT32_MAX;
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_OK && blocks == 1);
  CHECK(gibbs_sweep_check(&h, values, codes, 4, 3 * kGibbsBlock + 1, 0, 3 * kGibbsBlock + 1, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_OK && blocks == 4);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 0, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_OK && blocks == 0);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, 0, 1, 0, nullptr, 0, 1, &blocks) == PGM_OK && blocks == 0);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 40, 60, INT64_MAX - 60, last, 1, nullptr, 0, 1, &blocks) == PGM_OK);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, 0, 1, last, nullptr, 0, 1, &blocks) == PGM_OK);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 50, 0, 1, 7, trace, 150, 2, &blocks) == PGM_OK);
  CHECK(gibbs_sweep_check(nullptr, values, codes, 3, 100, 0, 100, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "gibbs_sweep: null plan");
  CHECK(gibbs_sweep_check(&h, nullptr, codes, 3, 100, 0, 100, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "gibbs_sweep: null values");
  CHECK(gibbs_sweep_check(&h, values, nullptr, 3, 100, 0, 100, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "gibbs_sweep: null codes");
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 99, 0, 100, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);   // ld < n_chains
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, -1, 50, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);  // row0 < 0
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 41, 60, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);  // leaves ld
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, -1, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, -1, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, INT64_MAX - 99, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(gibbs_sweep_check(&h, values, codes, 2, 100, 0, 100, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "gibbs_sweep: the plan has 3 columns, codes has 2");
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, 0, 0, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);  // sweep 0
  CHECK(g_last_err == "gibbs_sweep: sweeps [0, + 5) outside 1 .. 2^32 - 1");
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, 0, 1, -1, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, 0, last, 2, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, 0, last + 1, 0, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 100, 0, 1, 5, nullptr, 0, 0, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "gibbs_sweep: thin 0");
  CHECK(gibbs_sweep_check(&h, values, codes, 3, 100, 0, 50, 0, 1, 7, trace, 149, 2, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "gibbs_sweep: 3 records of 50 chains exceed ld_trace 149");
  const int64_t huge = (int64_t)kGibbsBlock * ((int64_t)INT32_MAX + 1);
  CHECK(gibbs_sweep_check(&h, values, codes, 3, huge, 0, huge, 0, 1, 5, nullptr, 0, 1, &blocks) == PGM_EINVAL);
  CHECK(gibbs_start_check(&h, codes, 3, 100, 10, 90, 7, &blocks) == PGM_OK && blocks == 1);
  CHECK(gibbs_start_check(nullptr, codes, 3, 100, 0, 100, 0, &blocks) == PGM_EINVAL && g_last_err == "gibbs_start: null plan");
  CHECK(gibbs_start_check(&h, nullptr, 3, 100, 0, 100, 0, &blocks) == PGM_EINVAL && g_last_err == "gibbs_start: null codes");
  CHECK(gibbs_start_check(&h, codes, 3, 100, 11, 90, 0, &blocks) == PGM_EINVAL);
  CHECK(gibbs_start_check(&h, codes, 2, 100, 0, 100, 0, &blocks) == PGM_EINVAL);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 6 && !strcmp(argv[1], "--uniform3")) {
    const double u = sample_uniform3(strtoull(argv[2], nullptr, 0), strtoull(argv[3], nullptr, 0),
                                     (uint32_t)strtoul(argv[4], nullptr, 0), (uint32_t)strtoul(argv[5], nullptr, 0));
    printf("%llu\n", (unsigned long long)(u * 0x1.0p53));
    return 0;
  }
  if (test_stream() || test_plan() || test_rejected() || test_argument_checks()) return 1;
  printf("gibbs_plan_selftest ok\n");
  return 0;
}

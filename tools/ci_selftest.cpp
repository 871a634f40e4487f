// ci_selftest.cpp — the host-testable parts of pgm_fit_citest on the CPU: Q(a, x) of pgmpy_amd/csrc/pgm_igamc.h
// (the very function the finishing kernel calls) against a recorded grid of scipy.stats.chi2.sf, and the CI
// work lists and argument checks of pgmpy_amd/csrc/pgmfit_plan.cpp.  Links that unit alone; meant for a
// sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I include -I pgmpy_amd/csrc
//       tools/ci_selftest.cpp pgmpy_amd/csrc/pgmfit_plan.cpp -o ci_selftest
//   ./ci_selftest grid.txt
// The grid file holds lines "k x sf" (hexadecimal floats); tests/test_ci_cpu.py writes it from the recorded grid.  Prints "max_rel_err <e>" over the points with
// sf >= 1e-300, and "ci_selftest ok" with exit status 0 when every check holds; the error's bound is the
// caller's (tests/test_ci_cpu.py).
//   ./ci_selftest --sf args.txt
// prints "sf <hexadecimal float>" = pgm_chi2_sf(x, k) for every line "k x" of args.txt and nothing else: the host
// build's values at arguments of the caller's choice (tests/test_crafted_cpu.py compares them with mpmath).
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pgmhip.h"
#include "pgm_fit.h"
#include "pgm_igamc.h"
#include "pgm_internal.h"

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

static pgm_fit_family family(std::vector<int> cols, std::vector<int> cards) {
  pgm_fit_family f;
  memset(&f, 0, sizeof f);
  f.n_vars = (int32_t)cols.size();
  for (size_t v = 0; v < cols.size() && v < PGM_MAX_DIMS; ++v) f.col[v] = cols[v], f.card[v] = cards[v];
  return f;
}

// ---------------------------------------------------------------------------- Q(a, x)
static int test_igamc(const char *path) {
  // the special values
  CHECK(pgm_igamc(1.5, 0.0) == 1.0);
  CHECK(pgm_igamc(1.5, -1e-17) == 1.0 && pgm_chi2_sf(-4.4e-16, 4.0) == 1.0);  // a statistic rounded below 0
  CHECK(pgm_igamc(1.5, std::numeric_limits<double>::infinity()) == 0.0);
  CHECK(std::isnan(pgm_igamc(1.5, std::nan(""))));
  CHECK(std::isnan(pgm_igamc(0.0, 1.0)));
  CHECK(std::fabs(pgm_igamc(1.0, 2.0) - std::exp(-2.0)) < 1e-15);  // Q(1, x) = e^-x
  CHECK(std::fabs(pgm_chi2_sf(2.0, 2.0) - std::exp(-1.0)) < 1e-15);
  FILE *f = fopen(path, "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 1;
  }
  double k, x, sf, worst = 0.0, worst_k = 0.0, worst_x = 0.0;
  int points = 0, tail = 0;
  while (fscanf(f, "%la %la %la", &k, &x, &sf) == 3) {
    const double got = pgm_chi2_sf(x, k);
    CHECK(got >= 0.0 && got <= 1.0);
    if (sf >= 1e-300) {
      const double rel = std::fabs(got - sf) / sf;
      if (rel > worst) worst = rel, worst_k = k, worst_x = x;
      ++points;
      tail += sf < 1e-200;
    } else {
      CHECK(got < 1e-299);  // below the range the bound is stated for: only the order of magnitude
    }
  }
  fclose(f);
  CHECK(points >= 500 && tail >= 1);
  printf("points %d\nmax_rel_err %.3e at k = %g x = %g\n", points, worst, worst_k, worst_x);
  return 0;
}

// ---------------------------------------------------------------------------- the work lists
static int test_work_lists() {
  static_assert(kCiChunk == 128 && kCiSmall == 16, "the families below are chosen for these constants");
  // qz: 1 packed, 1 packed, 127, 128, 129, 1 general (9 + 8 > 16), 1 packed (9 + 7), 255 * 3 = 765
  const pgm_fit_family fams[] = {family({0, 1}, {3, 2}),        family({0, 1, 2}, {3, 2, 1}),
                                 family({0, 1, 3}, {3, 2, 127}), family({0, 1, 4}, {3, 2, 128}),
                                 family({0, 1, 5}, {3, 2, 129}), family({6, 7}, {9, 8}),
                                 family({6, 8}, {9, 7}),         family({0, 1, 9, 10}, {40, 40, 255, 3})};
  FitPlan p;
  CHECK(fit_plan_build(fams, 8, p) == PGM_OK && p.ci_bad == -1);
  const int64_t off[9] = {0, 1, 2, 3, 4, 6, 7, 8, 14}, multi[9] = {0, 0, 0, 1, 2, 4, 5, 5, 11};
  CHECK(p.ci_off.size() == 9 && memcmp(p.ci_off.data(), off, sizeof off) == 0);
  CHECK(p.ci_multi_off.size() == 9 && memcmp(p.ci_multi_off.data(), multi, sizeof multi) == 0);
  CHECK(p.ci_single == (std::vector<int32_t>{0, 1, 6}));
  // a family's chunks do not depend on the families before it
  FitPlan alone;
  CHECK(fit_plan_build(fams + 4, 1, alone) == PGM_OK);
  CHECK(alone.ci_off[1] == 2 && alone.ci_multi_off[1] == 2 && alone.ci_single.empty());
  // a family without a Y is recorded, not refused: the plan still counts and scores
  const pgm_fit_family mixed[] = {family({0, 1}, {3, 2}), family({2}, {4}), family({3}, {2})};
  CHECK(fit_plan_build(mixed, 3, p) == PGM_OK && p.ci_bad == 1);
  return 0;
}

// ---------------------------------------------------------------------------- argument checks
static int test_argument_checks() {
  const pgm_fit_family fams[] = {family({0, 1}, {3, 2}), family({2, 0, 1}, {2, 3, 255})};
  FitHandle h;
  CHECK(fit_plan_build(fams, 2, h.p) == PGM_OK);
  const int64_t *counts = (const int64_t *)0x10000;  // addresses are only inspected, never dereferenced
  const double *stat = (const double *)0x20000, *pvalue = (const double *)0x30000;
  const int64_t *dof = (const int64_t *)0x40000;
  int64_t blocks = -1;
  CHECK(fit_citest_check(&h, counts, 1.0, PGM_CI_YATES, stat, dof, pvalue, &blocks) == PGM_OK && blocks == 2);
  CHECK(fit_citest_check(&h, counts, -0.5, 0, stat, dof, pvalue, nullptr) == PGM_OK);
  CHECK(fit_citest_check(nullptr, counts, 1.0, 0, stat, dof, pvalue, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_citest: null plan");
  CHECK(fit_citest_check(&h, nullptr, 1.0, 0, stat, dof, pvalue, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_citest: null counts");
  CHECK(fit_citest_check(&h, counts, 1.0, 0, nullptr, dof, pvalue, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_citest: null stat");
  CHECK(fit_citest_check(&h, counts, 1.0, 0, stat, nullptr, pvalue, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_citest: null dof");
  CHECK(fit_citest_check(&h, counts, 1.0, 0, stat, dof, nullptr, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_citest: null pvalue");
  CHECK(fit_citest_check(&h, counts, std::nan(""), 0, stat, dof, pvalue, &blocks) == PGM_EINVAL);
  CHECK(g_last_err.find("is not finite") != std::string::npos);
  CHECK(fit_citest_check(&h, counts, std::numeric_limits<double>::infinity(), 0, stat, dof, pvalue, &blocks) == PGM_EINVAL);
  CHECK(fit_citest_check(&h, counts, 1.0, 2, stat, dof, pvalue, &blocks) == PGM_EINVAL && g_last_err == "fit_citest: flags 2");
  CHECK(fit_citest_check(&h, counts, 1.0, -1, stat, dof, pvalue, &blocks) == PGM_EINVAL);
  const pgm_fit_family lone[] = {family({0, 1}, {3, 2}), family({2}, {4})};
  FitHandle g;
  CHECK(fit_plan_build(lone, 2, g.p) == PGM_OK);
  CHECK(fit_citest_check(&g, counts, 1.0, 0, stat, dof, pvalue, &blocks) == PGM_EINVAL);
  CHECK(g_last_err.find("family 1 has fewer than two variables") != std::string::npos);
  return 0;
}

// ---------------------------------------------------------------------------- pgm_chi2_sf at given arguments
static int print_sf(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 1;
  }
  double k, x;
  while (fscanf(f, "%la %la", &k, &x) == 2) printf("sf %a\n", pgm_chi2_sf(x, k));
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2 || (strcmp(argv[1], "--sf") == 0 && argc < 3)) {
    fprintf(stderr, "usage: ci_selftest <grid file of 'k x sf' lines> | --sf <file of 'k x' lines>\n");
    return 2;
  }
  if (strcmp(argv[1], "--sf") == 0) return print_sf(argv[2]);
  if (test_igamc(argv[1]) || test_work_lists() || test_argument_checks()) return 1;
  printf("ci_selftest ok\n");
  return 0;
}

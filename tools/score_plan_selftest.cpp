// score_plan_selftest.cpp — the host side of the structure-score launches (pgmpy_amd/csrc/pgmfit_plan.cpp:
// the (family, chunk) work list of the score kernel and the argument checks of pgm_fit_score) on the CPU,
// against hand-built families.  Links that unit alone; meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I include -I pgmpy_amd/csrc
//       tools/score_plan_selftest.cpp pgmpy_amd/csrc/pgmfit_plan.cpp -o score_plan_selftest
// Exit status 0 and "score_plan_selftest ok" when every check holds.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pgmhip.h"
#include "pgm_fit.h"
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

// ---------------------------------------------------------------------------- the work list
static int test_chunks() {
  static_assert(kScoreChunk == 128, "the families below are factorised for a 128-column chunk");
  // columns: 1 (no parents), 127, 128, 129, 420 = 3 chunks + 36, 1 (254 states, a parent of cardinality 1), 241
  const pgm_fit_family fams[] = {family({0}, {3}),
                                 family({0, 1}, {3, 127}),
                                 family({0, 2, 3}, {3, 8, 16}),
                                 family({0, 4, 5}, {3, 3, 43}),
                                 family({0, 6, 7}, {3, 20, 21}),
                                 family({8, 9}, {254, 1}),
                                 family({10, 11}, {17, 241})};
  FitPlan p;
  CHECK(fit_plan_build(fams, 7, p) == PGM_OK);
  const int64_t want[8] = {0, 1, 2, 3, 5, 9, 10, 12};
  CHECK(p.chunk_off.size() == 8 && memcmp(p.chunk_off.data(), want, sizeof want) == 0);
  // every chunk lies inside its family's columns and the chunks of a family cover them
  for (size_t f = 0; f < p.fams.size(); ++f) {
    const int64_t ncol = p.fams[f].size / p.fams[f].card[0], chunks = p.chunk_off[f + 1] - p.chunk_off[f];
    CHECK(chunks >= 1 && (chunks - 1) * kScoreChunk < ncol && chunks * kScoreChunk >= ncol);
    CHECK(ncol == p.col_off[f + 1] - p.col_off[f]);
  }
  // the work list of a family does not depend on the families before it
  FitPlan alone;
  CHECK(fit_plan_build(fams + 4, 1, alone) == PGM_OK);
  CHECK(alone.chunk_off.size() == 2 && alone.chunk_off[0] == 0 && alone.chunk_off[1] == 4);
  // the largest table a plan takes: 2^31 - 1 > bins, r = 1: 254^3 * 131 columns
  const pgm_fit_family big = family({0, 1, 2, 3, 4}, {1, 254, 254, 254, 131});
  CHECK(fit_plan_build(&big, 1, alone) == PGM_OK);
  CHECK(alone.chunk_off[1] == (254LL * 254 * 254 * 131 + kScoreChunk - 1) / kScoreChunk);
  return 0;
}

// ---------------------------------------------------------------------------- argument checks
static int test_argument_checks() {
  const pgm_fit_family fams[] = {family({0}, {3}), family({2, 0, 1}, {2, 3, 127})};
  FitHandle h;
  CHECK(fit_plan_build(fams, 2, h.p) == PGM_OK);
  const int64_t *counts = (const int64_t *)0x10000;  // addresses are only inspected, never dereferenced
  const double *alpha = (const double *)0x20000, *beta = (const double *)0x30000, *scores = (const double *)0x40000;
  int64_t blocks = -1;
  CHECK(fit_score_check(&h, counts, PGM_SCORE_BD, alpha, beta, scores, &blocks) == PGM_OK && blocks == 1 + 3);
  CHECK(fit_score_check(&h, counts, PGM_SCORE_BD | PGM_SCORE_SKIP_EMPTY, alpha, beta, scores, &blocks) == PGM_OK);
  CHECK(fit_score_check(&h, counts, PGM_SCORE_LL, nullptr, nullptr, scores, &blocks) == PGM_OK);
  CHECK(fit_score_check(&h, counts, PGM_SCORE_LL | PGM_SCORE_SKIP_EMPTY, nullptr, nullptr, scores, nullptr) == PGM_OK);
  CHECK(fit_score_check(nullptr, counts, PGM_SCORE_LL, alpha, beta, scores, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_score: null plan");
  CHECK(fit_score_check(&h, nullptr, PGM_SCORE_LL, alpha, beta, scores, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_score: null counts");
  CHECK(fit_score_check(&h, counts, PGM_SCORE_LL, alpha, beta, nullptr, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_score: null scores");
  CHECK(fit_score_check(&h, counts, 4, alpha, beta, scores, &blocks) == PGM_EINVAL && g_last_err == "fit_score: mode 4");
  CHECK(fit_score_check(&h, counts, -1, alpha, beta, scores, &blocks) == PGM_EINVAL);
  CHECK(fit_score_check(&h, counts, PGM_SCORE_BD, nullptr, beta, scores, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_score: null alpha in BD mode");
  CHECK(fit_score_check(&h, counts, PGM_SCORE_SKIP_EMPTY, alpha, nullptr, scores, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_score: null beta in BD mode");
  return 0;
}

int main() {
  if (test_chunks() || test_argument_checks()) return 1;
  printf("score_plan_selftest ok\n");
  return 0;
}

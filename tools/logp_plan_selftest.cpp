// logp_plan_selftest.cpp — the host side of the per-row log-probability (pgmpy_amd/csrc/pgmfit_plan.cpp: the
// argument checks of pgm_fit_log_values / pgm_fit_logprob and the host-only pgm_fit_logprob_info) on the CPU,
// against hand-built families.  Links that unit alone; meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I include -I pgmpy_amd/csrc
//       tools/logp_plan_selftest.cpp pgmpy_amd/csrc/pgmfit_plan.cpp -o logp_plan_selftest
// Exit status 0 and "logp_plan_selftest ok" when every check holds.
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

// addresses are only inspected, never dereferenced
static const double *const kLogv = (const double *)0x10000;
static const uint8_t *const kCodes = (const uint8_t *)0x20000;
static double *const kLogp = (double *)0x30000;
static double *const kTotal = (double *)0x40000;
static int64_t *const kSkipped = (int64_t *)0x50000;

static int test_log_values_check() {
  const pgm_fit_family fams[] = {family({0}, {3}), family({2, 0}, {2, 3})};
  FitHandle h;
  CHECK(fit_plan_build(fams, 2, h.p) == PGM_OK);
  int64_t blocks = -1;
  CHECK(fit_log_values_check(&h, kLogv, kLogp, &blocks) == PGM_OK && blocks == 1);
  CHECK(fit_log_values_check(&h, kLogv, kLogv, &blocks) == PGM_OK);  // in place
  CHECK(fit_log_values_check(&h, kLogv, kLogp, nullptr) == PGM_OK);
  CHECK(fit_log_values_check(nullptr, kLogv, kLogp, &blocks) == PGM_EINVAL && g_last_err == "fit_log_values: null plan");
  CHECK(fit_log_values_check(&h, nullptr, kLogp, &blocks) == PGM_EINVAL && g_last_err == "fit_log_values: null values");
  CHECK(fit_log_values_check(&h, kLogv, nullptr, &blocks) == PGM_EINVAL && g_last_err == "fit_log_values: null logv");
  CHECK(fit_log_values_check(&h, (const double *)0x10004, kLogp, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_log_values: values and logv must be 8-byte aligned");
  CHECK(fit_log_values_check(&h, kLogv, (const double *)0x30001, &blocks) == PGM_EINVAL);
  // one workgroup per kLogpBlock entries: 257 entries take two
  const pgm_fit_family big[] = {family({0, 1}, {1, 255}), family({1}, {2})};
  FitHandle g;
  CHECK(fit_plan_build(big, 2, g.p) == PGM_OK && g.p.total_bins == 257);
  CHECK(fit_log_values_check(&g, kLogv, kLogp, &blocks) == PGM_OK && blocks == 2);
  return 0;
}

static int test_logprob_check() {
  const pgm_fit_family fams[] = {family({0}, {3}), family({2, 0}, {2, 3})};
  FitHandle h;
  CHECK(fit_plan_build(fams, 2, h.p) == PGM_OK);
  int64_t blocks = -1;
  const int64_t R = kLogpRowsPerBlock;
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_OK && blocks == 1);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 40, 60, nullptr, nullptr, nullptr, &blocks) == PGM_OK && blocks == 1);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 7, 0, kLogp, kTotal, kSkipped, &blocks) == PGM_OK && blocks == 0);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 5, 4 * R, 0, R, kLogp, kTotal, kSkipped, &blocks) == PGM_OK && blocks == 1);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 4 * R, 0, R + 1, kLogp, kTotal, kSkipped, &blocks) == PGM_OK && blocks == 2);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 4 * R, 5, 2 * R + 3, kLogp, kTotal, kSkipped, &blocks) == PGM_OK && blocks == 3);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 0, 100, kLogp, kTotal, kSkipped, nullptr) == PGM_OK);
  // the most rows of one call, and one more
  const int64_t most = R * kLogpMaxBlocks;
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, most + 8, 0, most, kLogp, kTotal, kSkipped, &blocks) == PGM_OK);
  CHECK(blocks == kLogpMaxBlocks);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, most + 8, 0, most + 1, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_logprob: 65537 workgroups, a call covers 65536 (score the rows in several calls)");
  // null and misaligned pointers
  CHECK(fit_logprob_check(nullptr, kLogv, kCodes, 3, 100, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_logprob: null plan");
  CHECK(fit_logprob_check(&h, nullptr, kCodes, 3, 100, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_logprob: null logv");
  CHECK(fit_logprob_check(&h, kLogv, nullptr, 3, 100, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_logprob: null codes");
  const char *aligned = "fit_logprob: logv, logp, total and n_skipped must be 8-byte aligned";
  CHECK(fit_logprob_check(&h, (const double *)0x10004, kCodes, 3, 100, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == aligned);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 0, 100, (double *)0x30004, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 0, 100, kLogp, (double *)0x40002, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 0, 100, kLogp, kTotal, (int64_t *)0x50001, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == aligned);
  CHECK(fit_logprob_check(&h, kLogv, kCodes + 1, 3, 100, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_OK);  // codes: any byte
  // the window and the columns
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 99, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);  // ld < n_rows
  CHECK(g_last_err == "fit_logprob: rows [0, 100) outside ld 99");
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 41, 60, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_logprob: rows [41, 101) outside ld 100");
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, -1, 50, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_logprob: n_rows 50 row0 -1");
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, 100, 0, -1, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 3, -4, 0, 0, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);  // negative ld
  CHECK(fit_logprob_check(&h, kLogv, kCodes, 2, 100, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "fit_logprob: the plan reads column 2, codes has 2 columns");
  CHECK(fit_logprob_check(&h, kLogv, kCodes, -1, 100, 0, 100, kLogp, kTotal, kSkipped, &blocks) == PGM_EINVAL);
  return 0;
}

static int test_info() {
  const pgm_fit_family fams[] = {family({0}, {3}), family({2, 0}, {2, 3})};
  void *plan = nullptr;
  CHECK(pgm_fit_plan_create(fams, 2, &plan) == PGM_OK);
  pgm_logp_info_t info;
  const int64_t R = kLogpRowsPerBlock;
  CHECK(pgm_fit_logprob_info(plan, kCodes, 4 * R, 0, 2 * R + 3, &info) == PGM_OK);
  CHECK(info.block == kLogpBlock && info.rows_per_block == R && info.vec4 == 1 && info.n_families == 2 && info.n_partials == 3);
  CHECK(pgm_fit_logprob_info(plan, kCodes, 4 * R, 4, R, &info) == PGM_OK && info.vec4 == 1 && info.n_partials == 1);
  CHECK(pgm_fit_logprob_info(plan, kCodes, 4 * R, 1, R, &info) == PGM_OK && info.vec4 == 0);
  CHECK(pgm_fit_logprob_info(plan, kCodes, 4 * R + 1, 0, R, &info) == PGM_OK && info.vec4 == 0);
  CHECK(pgm_fit_logprob_info(plan, kCodes + 2, 4 * R, 0, R, &info) == PGM_OK && info.vec4 == 0);
  CHECK(pgm_fit_logprob_info(plan, nullptr, 4 * R, 0, 0, &info) == PGM_OK && info.vec4 == 0 && info.n_partials == 0);
  CHECK(pgm_fit_logprob_info(nullptr, kCodes, 4 * R, 0, R, &info) == PGM_EINVAL && g_last_err == "fit_logprob_info: null plan");
  CHECK(pgm_fit_logprob_info(plan, kCodes, 4 * R, 0, R, nullptr) == PGM_EINVAL && g_last_err == "fit_logprob_info: null info");
  CHECK(pgm_fit_logprob_info(plan, kCodes, 100, 41, 60, &info) == PGM_EINVAL);
  CHECK(g_last_err == "fit_logprob_info: rows [41, 101) outside ld 100");
  delete static_cast<FitHandle *>(plan);  // nothing was uploaded: the handle owns host memory only
  return 0;
}

int main() {
  if (test_log_values_check() || test_logprob_check() || test_info()) return 1;
  printf("logp_plan_selftest ok\n");
  return 0;
}

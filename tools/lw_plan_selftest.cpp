// lw_plan_selftest.cpp — the host side of the likelihood-weighted posterior (pgmpy_amd/csrc/pgmlw_plan.cpp:
// the launch geometry, the argument checks of pgm_sample_posterior, pgm_sample_posterior_info) on the CPU.
// Links the host units alone; meant for a plain and for a sanitizer build:
//   c++ -std=c++17 -g [-fsanitize=address,undefined] -I include -I pgmpy_amd/csrc
//       tools/lw_plan_selftest.cpp pgmpy_amd/csrc/pgmlw_plan.cpp pgmpy_amd/csrc/pgmsample_plan.cpp
//       pgmpy_amd/csrc/pgmfit_plan.cpp -o lw_plan_selftest
// Exit status 0 and "lw_plan_selftest ok" when every check holds.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pgm_internal.h"
#include "pgm_lw.h"
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

static bool said(const char *what) { return g_last_err.find(what) != std::string::npos; }

static pgm_fit_family fam(std::vector<int> cols, std::vector<int> cards) {
  pgm_fit_family f;
  memset(&f, 0, sizeof f);
  f.n_vars = (int32_t)cols.size();
  for (size_t v = 0; v < cols.size(); ++v) f.col[v] = cols[v], f.card[v] = cards[v];
  return f;
}

int main() {
  // a sample plan over 400 binary roots and target plans of n bins (families of two bins over column 0)
  std::vector<pgm_fit_family> roots;
  for (int i = 0; i < 400; ++i) roots.push_back(fam({i}, {2}));
  SampleHandle sh;
  CHECK(sample_plan_build(roots.data(), (int32_t)roots.size(), sh.p) == PGM_OK);
  auto targets = [](int bins, FitHandle &t) {
    std::vector<pgm_fit_family> f((size_t)bins / 2, fam({0}, {2}));
    return fit_plan_build(f.data(), (int32_t)f.size(), t.p);
  };
  LwGeometry g;
  {
    const int bins[] = {2, 7424, 7426, 13824, 13826, 17024};
    const int block[] = {256, 256, 128, 128, 64, 64};
    for (int i = 0; i < 6; ++i) {
      FitHandle t;
      CHECK(targets(bins[i], t) == PGM_OK);
      CHECK(lw_geometry("t", &sh, &t, 100, 0, &g) == PGM_OK);
      CHECK(g.block == block[i] && g.lds_bytes == 8 * bins[i] + 2048 + 400 * block[i] && g.lds_bytes <= kLwLdsBudget);
      CHECK(g.n_cols == 400 && g.total_bins == bins[i] && g.chunks == 1 && g.rows_per_launch == 65535);
    }
    FitHandle t;
    CHECK(targets(17026, t) == PGM_OK);
    CHECK(lw_geometry("t", &sh, &t, 100, 0, &g) == PGM_EINVAL && said("17026 target bins") && said("163840"));
    CHECK(lw_geometry("t", &sh, &t, 100, 64, &g) == PGM_EINVAL && said("workgroup of 64"));
  }
  FitHandle t;
  CHECK(targets(4, t) == PGM_OK);
  {  // K and the chunks
    const int64_t S[] = {1, 2, 1024, 1025, 2048, 2051, 1 << 20};
    const int K[] = {52, 52, 52, 51, 51, 50, 42};
    const int64_t chunks[] = {1, 1, 1, 2, 2, 3, 1024};
    for (int i = 0; i < 7; ++i) {
      CHECK(lw_geometry("t", &sh, &t, S[i], 0, &g) == PGM_OK);
      CHECK(g.k == K[i] && g.chunks == chunks[i] && g.rows_per_launch * g.chunks <= kLwMaxGroups);
      CHECK((S[i] << g.k) <= ((int64_t)1 << 62));  // a bin cannot overflow
    }
    CHECK(lw_geometry("t", &sh, &t, 0, 0, &g) == PGM_EINVAL && said("n_samples 0"));
    CHECK(lw_geometry("t", &sh, &t, (1 << 20) + 1, 0, &g) == PGM_EINVAL && said("n_samples 1048577"));
    CHECK(lw_geometry("t", &sh, &t, 10, 96, &g) == PGM_EINVAL && said("block 96"));
  }
  // the argument checks: the addresses are never touched
  const double *d = reinterpret_cast<const double *>(0x10000);
  const uint8_t *e = reinterpret_cast<const uint8_t *>(0x20001);
  const void *a = d, *odd = reinterpret_cast<const void *>(0x10004);
#define POST(H, T, VALUES, CDF, MODES, EV, NCOLS, LD, ROW0, NROWS, S, FIRST, BLOCK, ACC, SCALE, POSTP, LE, ESS) \
  sample_posterior_check(H, T, VALUES, CDF, MODES, EV, NCOLS, LD, ROW0, NROWS, S, FIRST, BLOCK, ACC, SCALE, POSTP, LE, ESS, &g)
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_OK);
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, a, a, nullptr, nullptr, nullptr) == PGM_OK);
  CHECK(POST(nullptr, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("null plan"));
  CHECK(POST(&sh, nullptr, d, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("null targets"));
  CHECK(POST(&sh, &t, nullptr, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("null values"));
  CHECK(POST(&sh, &t, d, nullptr, nullptr, e, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("null cdf"));
  CHECK(POST(&sh, &t, d, d, nullptr, nullptr, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("null evidence"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, nullptr, a, a, a, a) == PGM_EINVAL && said("null acc"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, a, nullptr, a, a, a) == PGM_EINVAL && said("null scale"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, odd, a, a, a, a) == PGM_EINVAL && said("8-byte aligned"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, odd) == PGM_EINVAL && said("8-byte aligned"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 399, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("the plan reads column 399"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 14, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("outside ld 16"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, -1, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("n_rows -1"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, -1, 0, a, a, a, a, a) == PGM_EINVAL && said("stream rows"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, INT64_MAX - 399, 0, a, a, a, a, a) == PGM_EINVAL && said("stream rows"));
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 4, 100, INT64_MAX - 400, 0, a, a, a, a, a) == PGM_OK);
  CHECK(POST(&sh, &t, d, d, nullptr, e, 400, 16, 0, 0, 100, INT64_MAX, 0, a, a, a, a, a) == PGM_OK);
  std::vector<uint8_t> modes(400, PGM_SAMPLE_OBSERVED);
  CHECK(POST(&sh, &t, d, d, modes.data(), e, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_OK);
  modes[17] = 3;
  CHECK(POST(&sh, &t, d, d, modes.data(), e, 400, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("family 17 mode 3"));
  {  // targets against the sample plan
    SampleHandle two;
    const pgm_fit_family f2[] = {fam({1}, {2}), fam({0, 1}, {3, 2})};
    CHECK(sample_plan_build(f2, 2, two.p) == PGM_OK);
    FitHandle t1, t2, t3;
    const pgm_fit_family a1[] = {fam({2}, {2})}, a2[] = {fam({1, 0}, {2, 4})}, a3[] = {fam({1, 0}, {2, 3})};
    CHECK(fit_plan_build(a1, 1, t1.p) == PGM_OK && fit_plan_build(a2, 1, t2.p) == PGM_OK && fit_plan_build(a3, 1, t3.p) == PGM_OK);
    CHECK(POST(&two, &t1, d, d, nullptr, e, 3, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("node of no family"));
    CHECK(POST(&two, &t1, d, d, nullptr, e, 2, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("the targets read column 2"));
    CHECK(POST(&two, &t2, d, d, nullptr, e, 2, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_EINVAL && said("cardinality 4, the sample plan has 3"));
    CHECK(POST(&two, &t3, d, d, nullptr, e, 2, 16, 0, 4, 100, 0, 0, a, a, a, a, a) == PGM_OK);
    pgm_lw_info_t info;
    CHECK(pgm_sample_posterior_info(&two, &t3, 7, 2051, 0, &info) == PGM_OK);
    CHECK(info.block == 256 && info.k == 50 && info.chunks_per_row == 3 && info.workgroups == 21 && info.total_bins == 6);
    CHECK(info.lds_bytes == 8 * 6 + 2048 + 2 * 256 && info.lds_budget == PGM_LW_LDS_BUDGET && info.chunk == PGM_LW_CHUNK);
    CHECK(pgm_sample_posterior_info(&two, &t3, 7, 2051, 0, nullptr) == PGM_EINVAL && said("null info"));
  }
  printf("lw_plan_selftest ok\n");
  return 0;
}

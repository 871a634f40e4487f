// sample_plan_selftest.cpp — the host side of forward sampling (pgmpy_amd/csrc/pgmsample_plan.cpp: family
// validation, the argument checks of pgm_sample_cdf / pgm_sample_forward, the choice of the kernel path)
// and the counter-based random stream of pgm_sample.h on the CPU.  Links the two host units alone; meant
// for a plain and for a sanitizer build:
//   c++ -std=c++17 -g [-fsanitize=address,undefined] -I include -I pgmpy_amd/csrc
//       tools/sample_plan_selftest.cpp pgmpy_amd/csrc/pgmsample_plan.cpp pgmpy_amd/csrc/pgmfit_plan.cpp
//       -o sample_plan_selftest
// Exit status 0 and "sample_plan_selftest ok" when every check holds.  `--uniform SEED ROW COL` prints the
// 53-bit integer behind that uniform: the test suite compares it with its numpy restatement.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pgm_internal.h"
#include "pgm_sample.h"
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

static pgm_fit_family family(std::vector<int> cols, std::vector<int> cards) {
  pgm_fit_family f;
  memset(&f, 0, sizeof f);
  f.n_vars = (int32_t)cols.size();
  for (size_t v = 0; v < cols.size() && v < PGM_MAX_DIMS; ++v) f.col[v] = cols[v], f.card[v] = cards[v];
  return f;
}

// ---------------------------------------------------------------------------- the stream
static int test_stream() {
  // the known answers of Philox4x32-10 (Random123's kat_vectors)
  const uint32_t kat[3][10] = {
      {0, 0, 0, 0, 0, 0, 0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8},
      {0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0x408f276d, 0x41c83b0e, 0xa20bc7c6,
       0x6d5451fd},
      {0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0, 0xd16cfe09, 0x94fdcceb, 0x5001e420,
       0x24126ea1}};
  for (const auto &k : kat) {
    uint32_t x[4];
    philox4x32_10(k[0], k[1], k[2], k[3], k[4], k[5], x);
    CHECK(x[0] == k[6] && x[1] == k[7] && x[2] == k[8] && x[3] == k[9]);
  }
  // seed 0, row 0: columns 0 and 1 are the two halves of the first vector
  CHECK(sample_uniform(0, 0, 0) == (double)(((uint64_t)0x6627e8d5 << 21) | (0xe169c58du >> 11)) * 0x1.0p-53);
  CHECK(sample_uniform(0, 0, 1) == (double)(((uint64_t)0xbc57ac4c << 21) | (0x9b00dbd8u >> 11)) * 0x1.0p-53);
  // the row's high word is the second counter word, the seed's high word the second key word
  uint32_t x[4];
  philox4x32_10(0xffffffffu, 0, 3, 0, 7, 0, x);
  CHECK(sample_uniform(7, 0xffffffffull, 6) == (double)(((uint64_t)x[0] << 21) | (x[1] >> 11)) * 0x1.0p-53);
  philox4x32_10(0, 1, 3, 0, 7, 9, x);
  CHECK(sample_uniform(((uint64_t)9 << 32) | 7, 1ull << 32, 7) == (double)(((uint64_t)x[2] << 21) | (x[3] >> 11)) * 0x1.0p-53);
  for (uint64_t r = 0; r < 2000; ++r) {
    const double u = sample_uniform(12345, r * 0x100000001ull, (uint32_t)(r % 77));
    CHECK(u >= 0.0 && u < 1.0);
  }
  return 0;
}

// ---------------------------------------------------------------------------- accepted and rejected families
static int test_plan() {
  // a diamond in a topological order, columns not in plan order
  const pgm_fit_family fams[] = {family({3}, {2}), family({0, 3}, {3, 2}), family({2, 3}, {4, 2}),
                                 family({1, 0, 2}, {2, 3, 4})};
  SamplePlan p;
  CHECK(sample_plan_build(fams, 4, p) == PGM_OK);
  CHECK(p.fit.fams.size() == 4 && p.fit.n_cols == 4 && p.fit.total_bins == 2 + 6 + 8 + 24);
  CHECK(p.fit.fams[3].off == 16 && p.fit.fams[3].stride[0] == 12 && p.fit.fams[3].stride[1] == 4);
  const int64_t col_off[5] = {0, 1, 3, 5, 17};
  CHECK(memcmp(p.fit.col_off.data(), col_off, sizeof col_off) == 0);
  // the maximum number of parents: 12 binary ones, the rest of cardinality 1 (31 binary parents are
  // 2^31 parent configurations: past the fit plan's table limit, rejected below)
  for (int binary : {12, PGM_MAX_DIMS - 1}) {
    std::vector<pgm_fit_family> wide;
    std::vector<int> cols{PGM_MAX_DIMS - 1}, cards{3};
    for (int v = 0; v < PGM_MAX_DIMS - 1; ++v) {
      const int k = v < binary ? 2 : 1;
      wide.push_back(family({v}, {k})), cols.push_back(v), cards.push_back(k);
    }
    wide.push_back(family(cols, cards));
    const int st = sample_plan_build(wide.data(), (int32_t)wide.size(), p);
    if (binary == 12) {
      CHECK(st == PGM_OK && p.fit.fams.back().size == 3 * 4096 && p.fit.fams.back().stride[0] == 4096);
      CHECK(p.fit.fams.back().stride[1] == 2048 && p.fit.fams.back().stride[12] == 1 && p.fit.fams.back().stride[31] == 1);
    } else {
      CHECK(st == PGM_EINVAL && g_last_err == "fit_plan_create: family 31 table exceeds 2^31 - 1 bins");
    }
  }
  return 0;
}

static int rejected(const pgm_fit_family *fams, int n, const char *msg) {
  SamplePlan p;
  g_last_err.clear();
  const int st = sample_plan_build(fams, n, p);
  if (st != PGM_EINVAL || g_last_err != msg) {
    fprintf(stderr, "expected PGM_EINVAL \"%s\"\n     got %d \"%s\"\n", msg, st, g_last_err.c_str());
    return 1;
  }
  return 0;
}

static int test_rejected() {
  pgm_fit_family f = family({0}, {2});
  CHECK(!rejected(nullptr, 1, "sample_plan_create: null families"));
  CHECK(!rejected(&f, 0, "sample_plan_create: 0 families"));
  f.n_vars = PGM_MAX_DIMS + 1;
  CHECK(!rejected(&f, 1, "sample_plan_create: family 0 has 33 variables (1 .. 32)"));
  f.n_vars = 0;
  CHECK(!rejected(&f, 1, "sample_plan_create: family 0 has 0 variables (1 .. 32)"));
  f = family({0}, {0});
  CHECK(!rejected(&f, 1, "sample_plan_create: family 0 variable 0 cardinality 0 (1 .. 255)"));
  f = family({0}, {256});
  CHECK(!rejected(&f, 1, "sample_plan_create: family 0 variable 0 cardinality 256 (1 .. 255)"));
  f = family({-2}, {2});
  CHECK(!rejected(&f, 1, "sample_plan_create: family 0 variable 0 column -2"));
  const pgm_fit_family twice[] = {family({0}, {2}), family({1, 0}, {2, 2}), family({0, 1}, {2, 2})};
  CHECK(!rejected(twice, 3, "sample_plan_create: column 0 is the node of families 0 and 2"));
  const pgm_fit_family late[] = {family({1, 0}, {2, 2}), family({0}, {2})};  // not a topological order
  CHECK(!rejected(late, 2, "sample_plan_create: family 0 parent column 0 is not the node of an earlier family"));
  const pgm_fit_family self[] = {family({0, 0}, {2, 2})};
  CHECK(!rejected(self, 1, "sample_plan_create: family 0 parent column 0 is not the node of an earlier family"));
  const pgm_fit_family card[] = {family({0}, {3}), family({1, 0}, {2, 2})};
  CHECK(!rejected(card, 2, "sample_plan_create: family 1 parent column 0 cardinality 2, its own family 0 has 3"));
  // the table size limit is the fit plan's
  const pgm_fit_family big[] = {family({0}, {255}), family({1}, {255}), family({2}, {255}), family({3}, {255}),
                                family({4, 0, 1, 2, 3}, {255, 255, 255, 255, 255})};
  CHECK(!rejected(big, 5, "fit_plan_create: family 4 table exceeds 2^31 - 1 bins"));
  return 0;
}

// ---------------------------------------------------------------------------- argument checks
static int test_argument_checks() {
  const pgm_fit_family fams[] = {family({0}, {3}), family({2, 0}, {2, 3})};
  SampleHandle h;
  CHECK(sample_plan_build(fams, 2, h.p) == PGM_OK);
  const double *values = (const double *)0x30000, *cdf = (const double *)0x40000;  // only inspected
  const uint8_t *codes = (const uint8_t *)0x10000;
  const double *w = (const double *)0x50000;
  int64_t blocks = -1;
  const uint8_t modes[2] = {PGM_SAMPLE_GIVEN, PGM_SAMPLE_OBSERVED}, bad_modes[2] = {0, 3};
  CHECK(sample_forward_check(&h, values, cdf, modes, codes, 3, 100, 0, 100, 0, w, &blocks) == PGM_OK && blocks == 1);
  CHECK(sample_forward_check(&h, nullptr, cdf, nullptr, codes, 3, 100, 0, 100, 0, nullptr, &blocks) == PGM_OK);
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 3 * kSampleRowsPerBlock + 1, 0,
                             3 * kSampleRowsPerBlock + 1, 0, nullptr, &blocks) == PGM_OK && blocks == 4);
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 100, 0, 0, 0, nullptr, &blocks) == PGM_OK && blocks == 0);
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 100, 40, 60, INT64_MAX - 60, nullptr, &blocks) == PGM_OK);
  CHECK(sample_forward_check(nullptr, values, cdf, nullptr, codes, 3, 100, 0, 100, 0, nullptr, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "sample_forward: null plan");
  CHECK(sample_forward_check(&h, values, nullptr, nullptr, codes, 3, 100, 0, 100, 0, nullptr, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "sample_forward: null cdf");
  CHECK(sample_forward_check(&h, values, cdf, nullptr, nullptr, 3, 100, 0, 100, 0, nullptr, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "sample_forward: null codes");
  CHECK(sample_forward_check(&h, nullptr, cdf, nullptr, codes, 3, 100, 0, 100, 0, w, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "sample_forward: weights need the values");
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 99, 0, 100, 0, nullptr, &blocks) == PGM_EINVAL);   // ld < n_rows
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 100, -1, 50, 0, nullptr, &blocks) == PGM_EINVAL);  // row0 < 0
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 100, 41, 60, 0, nullptr, &blocks) == PGM_EINVAL);  // leaves ld
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 100, 0, -1, 0, nullptr, &blocks) == PGM_EINVAL);
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 100, 0, 100, -1, nullptr, &blocks) == PGM_EINVAL);
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, 100, 0, 100, INT64_MAX - 99, nullptr, &blocks) == PGM_EINVAL);
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 2, 100, 0, 100, 0, nullptr, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "sample_forward: the plan writes column 2, codes has 2 columns");
  CHECK(sample_forward_check(&h, values, cdf, bad_modes, codes, 3, 100, 0, 100, 0, nullptr, &blocks) == PGM_EINVAL);
  CHECK(g_last_err == "sample_forward: family 1 mode 3");
  const int64_t huge = (int64_t)kSampleRowsPerBlock * ((int64_t)INT32_MAX + 1);
  CHECK(sample_forward_check(&h, values, cdf, nullptr, codes, 3, huge, 0, huge, 0, nullptr, &blocks) == PGM_EINVAL);
  // four rows per lane only where every column's dwords are aligned
  CHECK(codes_vec4(codes, 100, 0) && codes_vec4(codes, 4096, 132) && codes_vec4(codes + 4, 8, 4));
  CHECK(!codes_vec4(codes, 101, 0) && !codes_vec4(codes, 100, 131) && !codes_vec4(codes + 2, 100, 0));
  CHECK(sample_cdf_check(&h, values, (double *)cdf) == PGM_OK);
  CHECK(sample_cdf_check(nullptr, values, cdf) == PGM_EINVAL && g_last_err == "sample_cdf: null plan");
  CHECK(sample_cdf_check(&h, nullptr, cdf) == PGM_EINVAL && g_last_err == "sample_cdf: null values");
  CHECK(sample_cdf_check(&h, values, nullptr) == PGM_EINVAL && g_last_err == "sample_cdf: null cdf");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "--uniform")) {
    const double u = sample_uniform(strtoull(argv[2], nullptr, 0), strtoull(argv[3], nullptr, 0),
                                    (uint32_t)strtoul(argv[4], nullptr, 0));
    printf("%llu\n", (unsigned long long)(u * 0x1.0p53));
    return 0;
  }
  if (test_stream() || test_plan() || test_rejected() || test_argument_checks()) return 1;
  printf("sample_plan_selftest ok\n");
  return 0;
}

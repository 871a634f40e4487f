// fit_plan_selftest.cpp — the host side of parameter learning (pgmpy_amd/csrc/pgmfit_plan.cpp: family
// validation, the layout of the flat count buffer, the grouping of families per workgroup, the argument
// checks of pgm_fit_count / pgm_fit_finish) on the CPU, against hand-built families.  Links that unit
// alone; meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I include -I pgmpy_amd/csrc
//       tools/fit_plan_selftest.cpp pgmpy_amd/csrc/pgmfit_plan.cpp -o fit_plan_selftest
// Exit status 0 and "fit_plan_selftest ok" when every check holds.  `--print FILE` reads families (one
// per line: "col:card col:card ...", the node first) and prints each one's offset, size, strides and
// group, then the totals: the test suite compares that with its numpy restatement.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
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

// ---------------------------------------------------------------------------- layout
static int test_layout() {
  // no parents; two parents; the maximum number of parents (31: ten of cardinality 2, the rest 1);
  // cardinalities 1 and 254
  std::vector<int> cols32(PGM_MAX_DIMS), cards32(PGM_MAX_DIMS, 1);
  for (int v = 0; v < PGM_MAX_DIMS; ++v) cols32[v] = v;
  cards32[0] = 3;
  for (int v = 1; v <= 10; ++v) cards32[v] = 2;
  const pgm_fit_family fams[] = {family({4}, {3}), family({2, 0, 1}, {2, 3, 4}), family(cols32, cards32),
                                 family({0, 1}, {254, 1}), family({1, 0}, {1, 254})};
  FitPlan p;
  CHECK(fit_plan_build(fams, 5, p) == PGM_OK);
  CHECK(p.fams.size() == 5 && p.n_cols == PGM_MAX_DIMS);
  CHECK(p.fams[0].off == 0 && p.fams[0].size == 3 && p.fams[0].stride[0] == 1);
  CHECK(p.fams[1].off == 3 && p.fams[1].size == 24);
  CHECK(p.fams[1].stride[0] == 12 && p.fams[1].stride[1] == 4 && p.fams[1].stride[2] == 1);
  CHECK(p.fams[2].off == 27 && p.fams[2].size == 3 * 1024 && p.fams[2].stride[0] == 1024);
  for (int v = 1; v <= 10; ++v) CHECK(p.fams[2].stride[v] == 1 << (10 - v));
  for (int v = 11; v < PGM_MAX_DIMS; ++v) CHECK(p.fams[2].stride[v] == 1);  // cardinality 1: never multiplied by > 0
  CHECK(p.fams[3].off == 27 + 3072 && p.fams[3].size == 254 && p.fams[3].stride[0] == 1 && p.fams[3].stride[1] == 1);
  CHECK(p.fams[4].off == 27 + 3072 + 254 && p.fams[4].size == 254 && p.fams[4].stride[0] == 254);
  CHECK(p.total_bins == 27 + 3072 + 254 + 254);
  // CPD columns: 1, 12, 1024, 1, 254
  const int64_t col_off[6] = {0, 1, 13, 1037, 1038, 1292};
  CHECK(p.col_off.size() == 6 && memcmp(p.col_off.data(), col_off, sizeof col_off) == 0);
  // 3,607 bins in all: one group, in LDS
  CHECK(p.groups.size() == 1 && p.groups[0].fam_begin == 0 && p.groups[0].fam_end == 5 && !p.groups[0].global);
  CHECK(p.groups[0].off == 0 && p.groups[0].bins == p.total_bins);
  for (int f = 0; f < 5; ++f) CHECK(p.group_of[f] == 0);
  return 0;
}

static int test_groups() {
  // the tile's edge: 4,095 and 4,096 bins stay in LDS, 4,097 go to global memory
  static_assert(kFitTileBins == 4096, "the families below are factorised for a 4,096-bin tile");
  const pgm_fit_family edge[] = {family({0, 1, 2, 3, 4}, {13, 3, 3, 5, 7}), family({0, 1, 2}, {16, 16, 16}),
                                 family({0, 1}, {17, 241})};
  FitPlan p;
  CHECK(fit_plan_build(edge, 3, p) == PGM_OK);
  CHECK(p.fams[0].size == 4095 && p.fams[1].size == 4096 && p.fams[2].size == 4097);
  CHECK(p.groups.size() == 3 && !p.groups[0].global && !p.groups[1].global && p.groups[2].global);
  CHECK(p.groups[2].off == 4095 + 4096 && p.groups[2].bins == 4097 && p.groups[1].off == 4095);
  // [two small][global][two that fill a tile together][one that no longer fits]
  const pgm_fit_family mix[] = {family({0}, {3}),           family({1, 0}, {2, 3}),    family({2, 3, 4}, {20, 20, 20}),
                                family({5, 0}, {100, 3}),   family({6, 5}, {30, 100}), family({7, 6}, {40, 30})};
  CHECK(fit_plan_build(mix, 6, p) == PGM_OK);
  const int32_t group_of[6] = {0, 0, 1, 2, 2, 3};
  CHECK(p.groups.size() == 4 && memcmp(p.group_of.data(), group_of, sizeof group_of) == 0);
  CHECK(p.groups[0].bins == 9 && p.groups[1].global && p.groups[1].bins == 8000 && p.groups[1].fam_end == 3);
  CHECK(p.groups[2].off == 8009 && p.groups[2].bins == 3300 && p.groups[2].fam_begin == 3 && p.groups[2].fam_end == 5);
  CHECK(p.groups[3].off == 11309 && p.groups[3].bins == 1200 && !p.groups[3].global);
  // a family never shares a global group
  for (const FitGroup &g : p.groups) CHECK(g.global ? g.fam_end == g.fam_begin + 1 : g.bins <= kFitTileBins);
  return 0;
}

// ---------------------------------------------------------------------------- rejected families
static int rejected(const pgm_fit_family *fams, int n, const char *msg) {
  FitPlan p;
  g_last_err.clear();
  const int st = fit_plan_build(fams, n, p);
  if (st != PGM_EINVAL || g_last_err != msg) {
    fprintf(stderr, "expected PGM_EINVAL \"%s\"\n     got %d \"%s\"\n", msg, st, g_last_err.c_str());
    return 1;
  }
  return 0;
}

static int test_rejected() {
  pgm_fit_family f = family({0, 1}, {2, 2});
  CHECK(!rejected(nullptr, 1, "fit_plan_create: null families"));
  CHECK(!rejected(&f, 0, "fit_plan_create: 0 families"));
  f.n_vars = PGM_MAX_DIMS + 1;  // 32 parents
  CHECK(!rejected(&f, 1, "fit_plan_create: family 0 has 33 variables (1 .. 32)"));
  f.n_vars = 0;
  CHECK(!rejected(&f, 1, "fit_plan_create: family 0 has 0 variables (1 .. 32)"));
  f = family({0, 1}, {2, 0});
  CHECK(!rejected(&f, 1, "fit_plan_create: family 0 variable 1 cardinality 0 (1 .. 255)"));
  f = family({0, 1}, {-3, 2});
  CHECK(!rejected(&f, 1, "fit_plan_create: family 0 variable 0 cardinality -3 (1 .. 255)"));
  f = family({0, 1}, {2, 256});
  CHECK(!rejected(&f, 1, "fit_plan_create: family 0 variable 1 cardinality 256 (1 .. 255)"));
  f = family({0, -1}, {2, 2});
  CHECK(!rejected(&f, 1, "fit_plan_create: family 0 variable 1 column -1"));
  f = family({0, 1, 2, 3, 4}, {255, 255, 255, 255, 255});  // 255^4 > 2^31 - 1
  CHECK(!rejected(&f, 1, "fit_plan_create: family 0 table exceeds 2^31 - 1 bins"));
  const pgm_fit_family two[] = {family({0}, {2}), family({1, 0}, {2, 0})};
  CHECK(!rejected(two, 2, "fit_plan_create: family 1 variable 1 cardinality 0 (1 .. 255)"));
  return 0;
}

// ---------------------------------------------------------------------------- argument checks
static int test_argument_checks() {
  const pgm_fit_family fams[] = {family({0}, {3}), family({2, 0}, {2, 3})};
  FitHandle h;
  CHECK(fit_plan_build(fams, 2, h.p) == PGM_OK);
  const uint8_t *codes = (const uint8_t *)0x10000;  // addresses are only inspected, never dereferenced
  void *tables = (void *)0x20000;
  int64_t blocks = -1;
  CHECK(fit_count_check(&h, codes, 3, 100, 0, 100, tables, &blocks) == PGM_OK && blocks == 1);
  CHECK(fit_count_check(&h, codes, 3, 3 * kFitRowsPerBlock + 1, 0, 3 * kFitRowsPerBlock + 1, tables, &blocks) == PGM_OK);
  CHECK(blocks == 4);
  CHECK(fit_count_check(&h, codes, 3, 100, 0, 0, tables, &blocks) == PGM_OK && blocks == 0);
  CHECK(fit_count_check(&h, codes, 3, 100, 40, 60, tables, &blocks) == PGM_OK);
  CHECK(fit_count_check(nullptr, codes, 3, 100, 0, 100, tables, &blocks) == PGM_EINVAL && g_last_err == "fit_count: null plan");
  CHECK(fit_count_check(&h, nullptr, 3, 100, 0, 100, tables, &blocks) == PGM_EINVAL && g_last_err == "fit_count: null codes");
  CHECK(fit_count_check(&h, codes, 3, 100, 0, 100, nullptr, &blocks) == PGM_EINVAL && g_last_err == "fit_count: null tables");
  CHECK(fit_count_check(&h, codes, 3, 99, 0, 100, tables, &blocks) == PGM_EINVAL);   // ld < n_rows
  CHECK(fit_count_check(&h, codes, 3, 100, -1, 50, tables, &blocks) == PGM_EINVAL);  // negative row0
  CHECK(fit_count_check(&h, codes, 3, 100, 41, 60, tables, &blocks) == PGM_EINVAL);  // the window leaves ld
  CHECK(fit_count_check(&h, codes, 3, 100, 0, -1, tables, &blocks) == PGM_EINVAL);
  CHECK(fit_count_check(&h, codes, 2, 100, 0, 100, tables, &blocks) == PGM_EINVAL);  // the plan reads column 2
  CHECK(g_last_err == "fit_count: the plan reads column 2, codes has 2 columns");
  const int64_t huge = (int64_t)kFitRowsPerBlock * ((int64_t)INT32_MAX + 1);  // more workgroups than one launch takes
  CHECK(fit_count_check(&h, codes, 3, huge, 0, huge, tables, &blocks) == PGM_EINVAL);
  // four rows per lane only where every column's dword loads are aligned
  CHECK(codes_vec4(codes, 100, 0) && codes_vec4(codes, 4096, 132) && codes_vec4(codes + 4, 8, 4));
  CHECK(!codes_vec4(codes, 101, 0) && !codes_vec4(codes, 100, 131) && !codes_vec4(codes + 2, 100, 0));
  const double *values = (const double *)0x30000;
  CHECK(fit_finish_check(&h, tables, PGM_FIT_MLE, values) == PGM_OK);
  CHECK(fit_finish_check(&h, tables, PGM_FIT_BAYES | PGM_FIT_WEIGHTED, values) == PGM_OK);
  CHECK(fit_finish_check(nullptr, tables, PGM_FIT_MLE, values) == PGM_EINVAL);
  CHECK(fit_finish_check(&h, nullptr, PGM_FIT_MLE, values) == PGM_EINVAL && g_last_err == "fit_finish: null counts");
  CHECK(fit_finish_check(&h, tables, PGM_FIT_MLE, nullptr) == PGM_EINVAL && g_last_err == "fit_finish: null values");
  CHECK(fit_finish_check(&h, tables, 4, values) == PGM_EINVAL && g_last_err == "fit_finish: mode 4");
  return 0;
}

// ---------------------------------------------------------------------------- --print FILE
static int print_layout(const char *path) {
  FILE *in = fopen(path, "r");
  if (!in) {
    fprintf(stderr, "cannot open %s\n", path);
    return 2;
  }
  std::vector<pgm_fit_family> fams;
  char line[4096];
  while (fgets(line, sizeof line, in)) {
    std::istringstream ss(line);
    std::string tok;
    std::vector<int> cols, cards;
    while (ss >> tok) {
      int c = 0, k = 0;
      if (sscanf(tok.c_str(), "%d:%d", &c, &k) != 2) {
        fprintf(stderr, "bad token %s\n", tok.c_str());
        fclose(in);
        return 2;
      }
      cols.push_back(c), cards.push_back(k);
    }
    if (cols.empty()) continue;
    pgm_fit_family f = family(cols, cards);
    f.n_vars = (int32_t)cols.size();  // may exceed PGM_MAX_DIMS: rejected below
    fams.push_back(f);
  }
  fclose(in);
  FitPlan p;
  const int st = fit_plan_build(fams.data(), (int32_t)fams.size(), p);
  if (st != PGM_OK) {
    printf("error %d %s\n", st, g_last_err.c_str());
    return 0;
  }
  for (size_t f = 0; f < p.fams.size(); ++f) {
    printf("family %zu off %lld size %d group %d strides", f, (long long)p.fams[f].off, p.fams[f].size, p.group_of[f]);
    for (int v = 0; v < p.fams[f].n_vars; ++v) printf(" %d", p.fams[f].stride[v]);
    printf("\n");
  }
  printf("total %lld columns %lld groups %zu\n", (long long)p.total_bins, (long long)p.col_off.back(), p.groups.size());
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 2 && !strcmp(argv[1], "--print")) return print_layout(argv[2]);
  if (test_layout() || test_groups() || test_rejected() || test_argument_checks()) return 1;
  printf("fit_plan_selftest ok\n");
  return 0;
}

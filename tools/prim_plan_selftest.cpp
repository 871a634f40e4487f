// prim_plan_selftest.cpp — the host side of the primitive factor operations (pgmpy_amd/csrc/pgmprim_plan.cpp:
// the dim coalescer, plan_contract's long-run split and split-K geometry, the 16-byte-pairs predicate of an
// n-ary product, the lanes-per-output and row-grid rules, the batch job assembly and the refusals of
// pgm_batch_finalize's host half) on the CPU.  Links that unit alone:
//   c++ -std=c++17 -g -I include -I pgmpy_amd/csrc
//       tools/prim_plan_selftest.cpp pgmpy_amd/csrc/pgmprim_plan.cpp -o prim_plan_selftest
// and is meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I include -I pgmpy_amd/csrc
//       tools/prim_plan_selftest.cpp pgmpy_amd/csrc/pgmprim_plan.cpp -o prim_plan_selftest
// Exit status 0 and "prim_plan_selftest ok" when every check holds.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pgmhip.h"
#include "pgm_internal.h"
#include "pgm_prim.h"

using namespace pgmprim;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

// ---------------------------------------------------------------------------- the library's hooks
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

void pgmi_stale_probe(const char *) {}

static bool err_is(const char *text) { return g_last_err == text; }

// stand-in device addresses (never dereferenced), 16-B aligned
static double *addr(uintptr_t a) { return reinterpret_cast<double *>(a); }
static const uintptr_t kBase = 0x10000000;

// ---------------------------------------------------------------------------- the coalescer
// every index of the original dims maps to the same offsets, row by row, after merging
static int check_coalesce(const Dims &in, int want_n) {
  Dims out = in;
  coalesce(out);
  CHECK(out.n == want_n && out.nops == in.nops);
  int64_t total = 1, total_out = 1;
  for (int i = 0; i < in.n; ++i) total *= in.card[i];
  for (int i = 0; i < out.n; ++i) {
    CHECK(out.card[i] > 1);
    total_out *= out.card[i];
  }
  CHECK(total == total_out);
  for (int64_t flat = 0; flat < total; ++flat) {
    for (int t = 0; t < in.nops; ++t) {
      int64_t a = 0, b = 0, idx = flat;
      for (int i = in.n - 1; i >= 0; --i) {
        a += (idx % in.card[i]) * in.s[t][i];
        idx /= in.card[i];
      }
      idx = flat;
      for (int i = out.n - 1; i >= 0; --i) {
        b += (idx % out.card[i]) * out.s[t][i];
        idx /= out.card[i];
      }
      CHECK(a == b);
    }
  }
  return 0;
}

// dims of the given extents, every row dense in C-order, row t scaled by t + 1
static Dims dense(const std::vector<int64_t> &card, int nops) {
  Dims d;
  d.n = (int)card.size();
  d.nops = nops;
  int64_t run = 1;
  for (int i = d.n - 1; i >= 0; --i) {
    d.card[i] = card[(size_t)i];
    for (int t = 0; t < nops; ++t) d.s[t][i] = run * (t + 1);
    run *= card[(size_t)i];
  }
  return d;
}

static int test_coalesce() {
  for (int nops : {1, 2, 3, MOPS, MOPS + 1}) {
    CHECK(check_coalesce(dense({2, 3, 4, 5}, nops), 1) == 0);           // fully mergeable
    CHECK(check_coalesce(dense({1, 2, 1, 1, 3, 1}, nops), 1) == 0);     // extent-1 dims among them
    CHECK(check_coalesce(dense({1, 1, 1}, nops), 0) == 0);              // nothing left
    CHECK(check_coalesce(dense({}, nops), 0) == 0);
    Dims d = dense({2, 3, 4, 5}, nops);                                 // one row alone blocks one merge
    d.s[nops - 1][1] += 1;  // between dims 1 and 2 (and 0 and 1) for the last row only
    CHECK(check_coalesce(d, 3) == 0);
    d = dense({4, 1, 3, 2}, nops);  // a broadcast (stride 0) innermost dim in one row: it cannot join its neighbour
    d.s[0][3] = 0;
    CHECK(check_coalesce(d, 2) == 0);
    d = dense({3, 4}, nops);  // an all-zero row merges like a dense one
    d.s[0][0] = d.s[0][1] = 0;
    CHECK(check_coalesce(d, 1) == 0);
    d = dense({2, 2, 2, 2, 2, 2}, nops);  // a padded leading dimension in the middle
    for (int t = 0; t < nops; ++t)
      for (int i = 0; i < 3; ++i) d.s[t][i] += d.s[t][i] / 8 * 3;
    CHECK(check_coalesce(d, 2) == 0);
  }
  return 0;
}

// ---------------------------------------------------------------------------- KMAX after merging
// n kept dims of extent 2 that cannot merge (every stride 4x the next one's)
static pgm_contract_desc unmergeable(int n_keep, int n_red) {
  pgm_contract_desc d;
  memset(&d, 0, sizeof d);
  d.combine = PGM_COMBINE_COPY;
  d.reduce = n_red ? PGM_RED_SUM : PGM_RED_NONE;
  d.n_keep = n_keep;
  d.n_red = n_red;
  for (int i = 0; i < n_keep; ++i) {
    d.keep_card[i] = 2;
    d.keep_sa[i] = d.keep_sc[i] = (int64_t)1 << (2 * (n_keep - 1 - i));
  }
  for (int i = 0; i < n_red; ++i) {
    d.red_card[i] = 2;
    d.red_sa[i] = (int64_t)1 << (30 + 2 * (n_red - 1 - i));
  }
  return d;
}

static int test_kmax() {
  ContractLaunch L;
  pgm_contract_desc d = unmergeable(KMAX, KMAX);
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nk == KMAX && L.k.nr == KMAX);
  d = unmergeable(KMAX + 1, 0);
  CHECK(plan_contract(&d, L) == PGM_EINVAL && err_is("contract: 13 keep / 0 reduce dims after coalescing (limit 12)"));
  d = unmergeable(1, KMAX + 1);
  CHECK(plan_contract(&d, L) == PGM_EINVAL && err_is("contract: 1 keep / 13 reduce dims after coalescing (limit 12)"));
  // extent-1 dims do not count: PGM_MAX_DIMS given, KMAX left
  d = unmergeable(KMAX, 0);
  for (int i = KMAX; i < PGM_MAX_DIMS; ++i) d.keep_card[i] = 1;
  d.n_keep = PGM_MAX_DIMS;
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nk == KMAX && L.k.n_out == (1u << KMAX));

  const double *ops[PMAX];
  for (int t = 0; t < PMAX; ++t) ops[t] = addr(kBase + 4096 * (uintptr_t)t);
  for (int n : {KMAX, KMAX + 1}) {
    pgm_productn_desc p;
    memset(&p, 0, sizeof p);
    p.n_ops = 2;
    p.n_keep = n;
    for (int i = 0; i < n; ++i) {
      p.keep_card[i] = 2;
      p.keep_sc[i] = p.keep_s[0][i] = (int64_t)1 << (2 * (n - 1 - i));
    }
    ProdNK k;
    if (n == KMAX)
      CHECK(plan_prodn(&p, ops, k) == PGM_OK && k.nk == KMAX);
    else
      CHECK(plan_prodn(&p, ops, k) == PGM_EINVAL && err_is("product_n: 13 dims after coalescing (limit 12)"));
    pgm_contractn_desc c;
    memset(&c, 0, sizeof c);
    c.n_ops = 2;
    c.reduce = PGM_RED_SUM;
    c.n_keep = c.n_red = n;
    for (int i = 0; i < n; ++i) {
      c.keep_card[i] = c.red_card[i] = 2;
      c.keep_sc[i] = c.keep_s[0][i] = c.red_s[1][i] = (int64_t)1 << (2 * (n - 1 - i));
    }
    ContractNK nk;
    if (n == KMAX)
      CHECK(plan_contract_n(&c, ops, nk) == PGM_OK && nk.nk == KMAX && nk.nr == KMAX);
    else
      CHECK(plan_contract_n(&c, ops, nk) == PGM_EINVAL &&
            err_is("contract_n: 13 kept / 13 reduced dims after merging (at most 12 each)"));
  }
  // the two planners differ on a zero extent, and that stays: contract_n's empty output wins over a
  // negative extent beside it; a negative one alone is refused; the others refuse <= 0
  pgm_contractn_desc c;
  memset(&c, 0, sizeof c);
  c.n_ops = 1;
  c.reduce = PGM_RED_SUM;
  c.n_keep = 2;
  c.keep_card[0] = -1;
  c.keep_card[1] = 0;
  ContractNK nk;
  CHECK(plan_contract_n(&c, ops, nk) == PGM_OK && nk.n_out == 0);
  c.keep_card[1] = 2;
  CHECK(plan_contract_n(&c, ops, nk) == PGM_EINVAL && err_is("contract_n: negative cardinality"));
  c.keep_card[0] = 2;
  c.n_red = 1;
  c.red_card[0] = 0;
  CHECK(plan_contract_n(&c, ops, nk) == PGM_EINVAL && err_is("contract_n: an empty reduction"));
  d = unmergeable(2, 0);
  d.keep_card[1] = 0;
  CHECK(plan_contract(&d, L) == PGM_EINVAL && err_is("contract: keep_card[1] = 0"));
  return 0;
}

// ---------------------------------------------------------------------------- splits
// C[o] = sum over (outer, run) of A: n_out outputs, `outer` reduction entries that cannot merge with the run
static pgm_contract_desc dot_desc(int64_t n_out, int64_t outer, int64_t run) {
  pgm_contract_desc d;
  memset(&d, 0, sizeof d);
  d.combine = PGM_COMBINE_COPY;
  d.reduce = PGM_RED_SUM;
  d.n_keep = 1;
  d.keep_card[0] = n_out;
  d.keep_sa[0] = 2 * outer * run;
  d.keep_sc[0] = 1;
  d.n_red = 2;
  d.red_card[0] = outer;
  d.red_sa[0] = 2 * run;
  d.red_card[1] = run;
  d.red_sa[1] = 1;
  return d;
}

static int test_long_run_split() {
  ContractLaunch L;
  pgm_contract_desc d = dot_desc(3, 1, 8192);
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nr == 2 && L.k.ri_card == 4096 && L.k.n_ro == 2);
  CHECK(L.k.rsa[0] == 4096 && L.k.rsa[1] == 1 && L.k.ri_sa == 1);
  d = dot_desc(3, 1, 8191);
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nr == 1 && L.k.ri_card == 8191 && L.k.n_ro == 1);
  d = dot_desc(3, 255, 8192);
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nr == 3 && L.k.ri_card == 4096 && L.k.n_ro == 510);
  d = dot_desc(3, 256, 8192);
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nr == 2 && L.k.ri_card == 8192 && L.k.n_ro == 256);
  d = dot_desc(3, 1, 8192 + 256);  // the largest power-of-two chunk from 4,096 down that divides the run
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nr == 2 && L.k.ri_card == 256 && L.k.n_ro == 33);
  d = dot_desc(3, 1, 8193);  // none divides it: left whole
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nr == 1 && L.k.ri_card == 8193);
  d = dot_desc(4097, 1, 8192);  // more than 4,096 outputs: left whole
  CHECK(plan_contract(&d, L) == PGM_OK && L.k.nr == 1 && L.k.ri_card == 8192);
  return 0;
}

// the splits of a planned contraction visit every reduction entry exactly once, walked as the kernels do
static int check_cover(const pgm_contract_desc &d, bool *row_mode_split, bool *flat_split, bool *inner_cut) {
  ContractLaunch L;
  CHECK(plan_contract(&d, L) == PGM_OK);
  const ContractK &k = L.k;
  CHECK(k.n_split >= 1 && (uint64_t)k.n_ro * k.ri_card == k.n_red);
  CHECK(L.ws_doubles == (k.n_split > 1 ? (uint64_t)k.n_split * k.n_out : 0));
  std::vector<uint8_t> seen((size_t)k.n_red, 0);
  const uint32_t ns = (uint32_t)k.n_split;
  if (k.row_mode) {
    CHECK(L.grid[2] == ns && k.n_v == k.n_ro * k.ri_nb && k.ri_nb >= 1);
    CHECK((uint64_t)k.ri_nb * k.ri_chunk >= k.ri_card && k.ri_card > (uint64_t)(k.ri_nb - 1) * k.ri_chunk);
    CHECK((uint64_t)ns * k.red_chunk >= k.n_v);
    for (uint32_t s = 0; s < ns; ++s) {
      const uint32_t v0 = s * k.red_chunk, v1 = std::min<uint32_t>(k.n_v, v0 + k.red_chunk);
      for (uint32_t v = v0; v < v1; ++v) {
        const uint32_t ro = v / k.ri_nb, bk = v - ro * k.ri_nb;
        const uint32_t ri1 = std::min<uint32_t>(k.ri_card, (bk + 1) * k.ri_chunk);
        for (uint32_t ri = bk * k.ri_chunk; ri < ri1; ++ri) ++seen[(size_t)ro * k.ri_card + ri];
      }
    }
    if (ns > 1) *row_mode_split = true;
    if (k.ri_nb > 1) *inner_cut = true;
  } else {
    CHECK(L.grid[1] == ns && L.grid[2] == 1 && k.g_log2 >= 0 && k.g_log2 <= 6 && (1u << k.g_log2) <= k.ri_card);
    CHECK((uint64_t)ns * k.red_chunk >= k.n_ro);
    for (uint32_t s = 0; s < ns; ++s) {
      const uint32_t r0 = s * k.red_chunk, r1 = std::min<uint32_t>(k.n_ro, r0 + k.red_chunk);
      for (uint32_t ro = r0; ro < r1; ++ro)
        for (uint32_t ri = 0; ri < k.ri_card; ++ri) ++seen[(size_t)ro * k.ri_card + ri];
    }
    if (ns > 1) *flat_split = true;
  }
  for (uint8_t c : seen) CHECK(c == 1);
  return 0;
}

static int test_split_cover() {
  bool row_split = false, flat_split = false, inner_cut = false;
  for (int64_t n_out : {1, 3, 64, 1000, 4096, 4097})
    for (int64_t outer : {1, 2, 7, 255, 256, 1000})
      for (int64_t run : {1, 2, 63, 64, 1000, 8191, 8192, 12288, 100000}) {
        if (outer * run > (1 << 22)) continue;
        const pgm_contract_desc d = dot_desc(n_out, outer, run);
        CHECK(check_cover(d, &row_split, &flat_split, &inner_cut) == 0);
      }
  // row mode: NX rows innermost in A and C, few outer outputs, a long reduction
  for (int64_t nx : {64, 100, 256, 257, 4096})
    for (int64_t n_outer : {1, 2, 5})
      for (int64_t outer : {1, 3, 17})
        for (int64_t run : {1, 15, 16, 63, 64, 65, 1000, 4096, 5000}) {
          pgm_contract_desc d;
          memset(&d, 0, sizeof d);
          d.combine = PGM_COMBINE_COPY;
          d.reduce = PGM_RED_MAX;
          d.n_keep = 2;
          d.keep_card[0] = n_outer;
          d.keep_card[1] = nx;
          d.keep_sa[0] = 3 * outer * run * nx;
          d.keep_sa[1] = 1;
          d.keep_sc[0] = nx;
          d.keep_sc[1] = 1;
          d.n_red = 2;
          d.red_card[0] = outer;
          d.red_card[1] = run;
          d.red_sa[0] = 2 * run * nx;
          d.red_sa[1] = nx;
          CHECK(check_cover(d, &row_split, &flat_split, &inner_cut) == 0);
        }
  CHECK(row_split && flat_split && inner_cut);  // the sweep reaches all three
  return 0;
}

// ---------------------------------------------------------------------------- the shared rules
static int test_rules() {
  CHECK(lanes_log2(1, 4096, 1) == 0 && lanes_log2(1, 4096, 2) == 1 && lanes_log2(1, 4096, 63) == 5);
  CHECK(lanes_log2(1, 4096, 64) == 6 && lanes_log2(1, 4096, 1 << 20) == 6);
  CHECK(lanes_log2(2048, 4096, 64) == 1 && lanes_log2(4096, 4096, 64) == 0 && lanes_log2(4095, 4096, 64) == 1);
  CHECK(lanes_log2(100, 256, 64) == 2);  // 100 -> 200 -> 400: stops once the lanes reach the cap
  uint32_t g[3];
  row_grid(1, 1000, g);
  CHECK(g[0] == 1000 && g[1] == 1 && g[2] == 1);
  row_grid(1, 5000, g);
  CHECK(g[0] == 2048 && g[1] == 1);
  row_grid(100, 1000, g);
  CHECK(g[0] == 20 && g[1] == 100);
  row_grid(5000, 7, g);
  CHECK(g[0] == 1 && g[1] == 5000);
  row_grid(1 << 20, 7, g);
  CHECK(g[0] == 1 && g[1] == 65535);
  return 0;
}

// ---------------------------------------------------------------------------- the product pairs predicate
static int test_prodn_pairs() {
  const double *ops[PMAX];
  for (int t = 0; t < PMAX; ++t) ops[t] = addr(kBase + 4096 * (uintptr_t)t);
  double *C = addr(kBase + 65536);
  pgm_productn_desc d;
  memset(&d, 0, sizeof d);
  d.n_ops = 3;  // X0[a, b] (padded rows) * X1[b] * X2[a] -> C[a, b] (padded rows)
  d.n_keep = 2;
  d.keep_card[0] = 5;
  d.keep_card[1] = 6;
  d.keep_sc[0] = 8;
  d.keep_sc[1] = 1;
  d.keep_s[0][0] = 10;
  d.keep_s[0][1] = 1;
  d.keep_s[1][0] = 0;
  d.keep_s[1][1] = 1;
  d.keep_s[2][0] = 1;  // broadcast along the innermost dim: read as a scalar, so its odd outer stride is fine
  d.keep_s[2][1] = 0;
  ProdNK base;
  CHECK(plan_prodn(&d, ops, base) == PGM_OK && base.nk == 2 && base.n_out == 30 && base.row_mode == 0);
  CHECK(prodn_pairs_ok(base, C));
  ProdNK k = base;
  k.kdiv[1] = make_fdiv(7);  // an odd innermost extent
  CHECK(!prodn_pairs_ok(k, C));
  k = base;
  k.ksc[1] = 2;  // the output is not unit-stride along it
  CHECK(!prodn_pairs_ok(k, C));
  CHECK(!prodn_pairs_ok(base, C + 1));  // the output base is 8 mod 16
  k = base;
  k.ksc[0] = 7;  // an odd outer stride of the output
  CHECK(!prodn_pairs_ok(k, C));
  k = base;
  k.ks[0][1] = 2;  // an operand neither unit-stride nor broadcast
  CHECK(!prodn_pairs_ok(k, C));
  k = base;
  k.ops[1] = ops[1] + 1;  // a unit-stride operand's base is 8 mod 16
  CHECK(!prodn_pairs_ok(k, C));
  k = base;
  k.ks[0][0] = 11;  // a unit-stride operand's odd outer stride
  CHECK(!prodn_pairs_ok(k, C));
  k = base;
  k.ops[2] = ops[2] + 1;  // a broadcast operand may sit anywhere
  k.ks[2][0] = 3;
  CHECK(prodn_pairs_ok(k, C));
  k = base;
  k.n_ops = 2;  // clauses of operands past n_ops are not read
  k.ks[2][1] = 2;
  CHECK(prodn_pairs_ok(k, C));
  k = base;
  k.nk = 0;  // a scalar product has no pair
  CHECK(!prodn_pairs_ok(k, C));
  return 0;
}

// ---------------------------------------------------------------------------- batch jobs and finalize's host half
static pgm_contract_desc marg_desc(int64_t n_out, int64_t n_red) {  // C[o] = sum_r A[o, r]
  pgm_contract_desc d;
  memset(&d, 0, sizeof d);
  d.combine = PGM_COMBINE_COPY;
  d.reduce = PGM_RED_SUM;
  d.n_keep = d.n_red = 1;
  d.keep_card[0] = n_out;
  d.keep_sa[0] = n_red;
  d.keep_sc[0] = 1;
  d.red_card[0] = n_red;
  d.red_sa[0] = 1;
  return d;
}

static int test_batch() {
  double *A = addr(kBase), *C = addr(kBase + 65536);
  int64_t blocks = -1;
  {  // lanes per output against the mode's cap; pairs when one lane per output is the choice anyway
    BatchHandle h;
    pgm_contract_desc d = marg_desc(1000, 64);
    CHECK(pgm_batch_add_contract(&h, &d, A, nullptr, C) == PGM_OK);
    CHECK(h.jobs[0].c.g_log2 == 3 && h.jobs[0].c.row_mode == 0 && h.jobs[0].nblocks == 32);  // 1000 << 3 >= 4096
    d = marg_desc(1000, 1);
    CHECK(pgm_batch_add_contract(&h, &d, A, nullptr, C) == PGM_OK);
    CHECK(h.jobs[1].c.g_log2 == 0 && h.jobs[1].c.row_mode == 2 && h.jobs[1].nblocks == 2);  // 500 pairs
    CHECK(pgm_batch_add_contract(&h, &d, A, nullptr, C + 1) == PGM_OK);
    CHECK(h.jobs[2].c.row_mode == 0 && h.jobs[2].nblocks == 4);
    CHECK(pgm_batch_blocks(&h, &blocks) == PGM_OK && blocks == 38 && h.jobs[2].block0 == 34);
    CHECK(pgm_batch_set_mode(&h, PGM_BATCH_ONE_WORKGROUP) == PGM_EINVAL && err_is("batch_set_mode: set before the first job"));
    CHECK(pgm_batch_add_level(&h) == PGM_EINVAL && err_is("batch_add_level: levels need PGM_BATCH_ONE_WORKGROUP"));
    std::vector<ChainJob> chain;
    size_t lds = 0;
    CHECK(batch_close(&h, chain, lds) == PGM_OK && chain.empty());
    CHECK(h.spec == PGM_COMBINE_COPY * 3 + PGM_RED_SUM && h.level_off.size() == 2 && h.level_off[1] == 38);
  }
  {
    BatchHandle h;
    CHECK(pgm_batch_set_mode(&h, 7) == PGM_EINVAL && err_is("batch_set_mode: mode 7"));
    CHECK(pgm_batch_set_mode(&h, PGM_BATCH_ONE_WORKGROUP) == PGM_OK);
    pgm_contract_desc d = marg_desc(1000, 64);
    CHECK(pgm_batch_add_contract(&h, &d, A, nullptr, C) == PGM_OK);
    CHECK(h.jobs[0].c.g_log2 == 0 && h.jobs[0].c.row_mode == 0);  // 1000 lanes are over one block's 256 already
    d = marg_desc(100, 64);
    CHECK(pgm_batch_add_level(&h) == PGM_OK && pgm_batch_add_level(&h) == PGM_OK);  // an empty level is not opened
    CHECK(pgm_batch_add_contract(&h, &d, A, nullptr, C) == PGM_OK && h.jobs[1].c.g_log2 == 2);
    std::vector<ChainJob> chain;
    size_t lds = 0;
    CHECK(batch_close(&h, chain, lds) == PGM_OK && chain.size() == 2);
    CHECK(h.level_off.size() == 3 && h.level_off[1] == 4 && h.level_off[2] == 6);
    CHECK(lds == 2 * sizeof(ChainJob) + 4 * (6 + 3) && lds <= kChainLdsMax);
    CHECK(chain[1].block0 == 4 && chain[1].nblocks == 2 && chain[1].A == A && chain[1].C == C &&
          chain[1].red == PGM_RED_SUM && chain[1].c.g_log2 == 2 && chain[1].c.n_out == 100);
    // refusal 1: a job that is not a contraction
    const double *ops[PMAX] = {A, A, A, A, A, A, A, A};
    pgm_productn_desc p;
    memset(&p, 0, sizeof p);
    p.n_ops = 1;
    p.n_keep = 1;
    p.keep_card[0] = 10;
    p.keep_sc[0] = p.keep_s[0][0] = 1;
    CHECK(pgm_batch_add_product_n(&h, &p, ops, C) == PGM_OK && h.jobs[2].pn.pairs == 1);
    CHECK(batch_close(&h, chain, lds) == PGM_EINVAL &&
          err_is("batch_finalize: a single-workgroup batch takes contractions only"));
    CHECK(h.spec == -1);
  }
  {  // refusal 2: tables over the LDS budget
    BatchHandle h;
    CHECK(pgm_batch_set_mode(&h, PGM_BATCH_ONE_WORKGROUP) == PGM_OK);
    const pgm_contract_desc d = marg_desc(10, 4);
    const size_t n = kChainLdsMax / sizeof(ChainJob) + 1;
    for (size_t i = 0; i < n; ++i) CHECK(pgm_batch_add_contract(&h, &d, A, nullptr, C) == PGM_OK);
    std::vector<ChainJob> chain;
    size_t lds = 0;
    CHECK(batch_close(&h, chain, lds) == PGM_EINVAL && chain.empty());
    char want[128];
    snprintf(want, sizeof want, "batch_finalize: single-workgroup tables of %zu bytes exceed the LDS budget",
             n * sizeof(ChainJob) + 4 * (n + 2));
    CHECK(err_is(want));
  }
  {  // a products-only batch, and a mixed one
    BatchHandle h;
    const double *ops[PMAX] = {A, A, A, A, A, A, A, A};
    pgm_productn_desc p;
    memset(&p, 0, sizeof p);
    p.n_ops = 2;
    p.n_keep = 1;
    p.keep_card[0] = 1000;
    p.keep_sc[0] = p.keep_s[0][0] = 1;
    CHECK(pgm_batch_add_product_n(&h, &p, ops, C + 1) == PGM_OK && h.jobs[0].pn.pairs == 0 && h.jobs[0].nblocks == 4);
    std::vector<ChainJob> chain;
    size_t lds = 0;
    CHECK(batch_close(&h, chain, lds) == PGM_OK && h.spec == kBatchSpecProducts);
    const pgm_contract_desc d = marg_desc(10, 4);
    CHECK(pgm_batch_add_contract(&h, &d, A, nullptr, C) == PGM_OK);
    CHECK(batch_close(&h, chain, lds) == PGM_OK && h.spec == -1);
    h.d_jobs = reinterpret_cast<BatchJob *>(A);  // as after pgm_batch_finalize
    CHECK(pgm_batch_add_contract(&h, &d, A, nullptr, C) == PGM_EINVAL && err_is("batch: already finalized"));
    CHECK(pgm_batch_add_level(&h) == PGM_EINVAL && err_is("batch_add_level: already finalized"));
    h.d_jobs = nullptr;
  }
  return 0;
}

// ---------------------------------------------------------------------------- the host-only queries
static int test_info() {
  pgm_contract_desc d = dot_desc(3, 1, 8192);
  pgm_contract_info_t info;
  CHECK(pgm_contract_info(&d, nullptr, nullptr, &info) == PGM_OK);
  CHECK(info.kernel == PGM_CK_FLAT && info.ri_card == 4096 && info.n_ro == 2 && info.n_red == 8192 && info.n_out == 3);
  CHECK(info.g_log2 == 6 && info.n_split == 2 && info.red_chunk == 1 && info.empty_splits == 0);
  size_t ws = 0;
  CHECK(pgm_contract_workspace(&d, &ws) == PGM_OK && ws == 2 * 3 * sizeof(double));
  CHECK(pgm_contract_info(&d, nullptr, nullptr, nullptr) == PGM_EINVAL && err_is("null pointer"));
  // the two-row kernel: COPY, even rows, unit stride, aligned
  memset(&d, 0, sizeof d);
  d.combine = PGM_COMBINE_COPY;
  d.reduce = PGM_RED_SUM;
  d.n_keep = 2;
  d.keep_card[0] = 3;
  d.keep_card[1] = 514;
  d.keep_sa[0] = 4 * 514;
  d.keep_sa[1] = 1;
  d.keep_sc[0] = 514;
  d.keep_sc[1] = 1;
  d.n_red = 1;
  d.red_card[0] = 4;
  d.red_sa[0] = 514;
  CHECK(pgm_contract_info(&d, addr(kBase), addr(kBase), &info) == PGM_OK && info.kernel == PGM_CK_ROWS_TAB2);
  CHECK(info.grid[0] == 2 && info.grid[1] == 3 && info.grid[2] == 1);
  CHECK(pgm_contract_info(&d, addr(kBase + 8), addr(kBase), &info) == PGM_OK && info.kernel == PGM_CK_ROWS_TAB);
  CHECK(info.grid[0] == 3);
  d.red_card[0] = RTAB_MAX + 1;
  CHECK(pgm_contract_info(&d, addr(kBase), addr(kBase), &info) == PGM_OK && info.kernel == PGM_CK_ROWS);
  return 0;
}

int main() {
  if (test_coalesce() || test_kmax() || test_long_run_split() || test_split_cover() || test_rules() ||
      test_prodn_pairs() || test_batch() || test_info())
    return 1;
  printf("prim_plan_selftest ok\n");
  return 0;
}

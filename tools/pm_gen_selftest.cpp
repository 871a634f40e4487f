// pm_gen_selftest.cpp — the generators of the specialised kernels (pgmpy_amd/csrc/pgmpm_gen.cpp: planner of
// the fused product + marginal step, its specialisation choice, the source of the fused / two-marginal /
// merged steps and of the specialised contraction batches) on the CPU, against hand-built descriptors.
// Links that unit and pgmrows_plan.cpp (for pgmi_appendf) alone; meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I include -I pgmpy_amd/csrc
//       tools/pm_gen_selftest.cpp pgmpy_amd/csrc/pgmpm_gen.cpp pgmpy_amd/csrc/pgmrows_plan.cpp -o pm_gen_selftest
// Exit status 0 and "pm_gen_selftest ok" when every check holds.  `--print` lists, per case, the length and
// SHA-256 of the generated source ("0 -": no specialised kernel) and checks nothing; `--dump DIR` writes each
// source to DIR/<case>.hip.
//
// The expected lengths and hashes below (and tests/golden/pm_source.json) were recorded from the pgmpm.cpp
// this unit was split out of: the same descriptors through its pgm_product_n_marginal_bind /
// pgm_product_n_bind / pgm_product_n_marginals_bind / pgm_pm_merge / pgmi_cs_bind and pgm_pm_bound_source.
// They pin the split to that code byte for byte.  (table513 alone needed a device there: that code allocated the
// pointer table before its source could be read back.)
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pgmhip.h"
#include "pgm_internal.h"
#include "pgm_pm.h"

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

// ---------------------------------------------------------------------------- SHA-256 (FIPS 180-4)
static std::string sha256(const void *data, size_t len) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98,
      0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
      0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8,
      0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
      0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819,
      0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
      0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7,
      0xc67178f2};
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  std::vector<uint8_t> m((const uint8_t *)data, (const uint8_t *)data + len);
  m.push_back(0x80);
  while (m.size() % 64 != 56) m.push_back(0);
  for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(((uint64_t)len * 8) >> (8 * i)));
  for (size_t off = 0; off < m.size(); off += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = (uint32_t)m[off + 4 * i] << 24 | (uint32_t)m[off + 4 * i + 1] << 16 | (uint32_t)m[off + 4 * i + 2] << 8 |
             (uint32_t)m[off + 4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
  }
  char out[65];
  for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
  return out;
}

// ---------------------------------------------------------------------------- hand-built cases
// Pointers are only inspected (alignment), never dereferenced.
static const double *fake_op(int t) { return (const double *)(uintptr_t)(0x10000000ull * (unsigned)(t + 1)); }
static double *const kFakeC = (double *)(uintptr_t)0x70000000ull;
static double *const kFakeM = (double *)(uintptr_t)0x60000000ull;
static double *const kFakeM2 = (double *)(uintptr_t)0x68000000ull;

// one fused step: the product of C-order operands over the dims `dims` (one letter each, the row dim last),
// stored C-order (store) and reduced onto the C-order marginal over `marg`; two: a second marginal `marg2`
// in the same pass (pgm_product_n_marginals_bind), no product
struct Step {
  pgm_productn_desc d;
  const double *ops[MOPS];
  double *C, *M, *M2;
  int64_t ms[PGM_MAX_DIMS], ms2[PGM_MAX_DIMS];
  int32_t reduce;
  bool has_m, two;
};

// C-order strides of the dims `sub` (a subsequence of `dims`) at the positions of `dims`, 0 elsewhere
static void c_strides(const char *dims, const int64_t *card, const char *sub, int64_t *out) {
  const int n = (int)strlen(dims);
  int64_t s = 1;
  for (int i = n - 1; i >= 0; --i) {
    out[i] = 0;
    if (strchr(sub, dims[i])) out[i] = s, s *= card[i];
  }
}

static Step mk_step(const char *dims, std::vector<int64_t> card, std::vector<const char *> ops, const char *marg,
                    int32_t reduce, bool store, std::vector<int> kinds = {}) {
  Step s;
  memset(&s, 0, sizeof s);
  const int n = (int)strlen(dims);
  s.d.n_ops = (int32_t)ops.size();
  s.d.n_keep = n;
  for (int i = 0; i < n; ++i) s.d.keep_card[i] = card[i];
  c_strides(dims, card.data(), dims, s.d.keep_sc);
  for (size_t t = 0; t < ops.size(); ++t) {
    s.d.op_kind[t] = t < kinds.size() ? kinds[t] : PGM_PRODN_MUL;
    c_strides(dims, card.data(), ops[t], s.d.keep_s[t]);
    s.ops[t] = fake_op((int)t);
  }
  c_strides(dims, card.data(), marg, s.ms);
  s.C = store ? kFakeC : nullptr;
  s.M = kFakeM;
  s.reduce = reduce;
  s.has_m = true;
  return s;
}

// XI = 1, no row tail (NP = 256), 3 blocks (total % 8 != 0), sum, product stored
static Step step_sum_store() { return mk_step("abR", {3, 4, 512}, {"abR", "bR"}, "aR", PGM_RED_SUM, true); }
// max, 8 blocks (total % 8 == 0), a row tail (NP = 300)
static Step step_max_store() { return mk_step("abR", {4, 4, 600}, {"abR", "b"}, "aR", PGM_RED_MAX, true); }
// the marginal alone (nontemporal marginal stores), two reduced dims
static Step step_marg_only() { return mk_step("abcR", {3, 2, 4, 512}, {"abcR", "bc", "acR"}, "aR", PGM_RED_SUM, false); }
// the product alone (pgm_product_n_bind: every dim kept, no marginal)
static Step step_product_only() {
  Step s = mk_step("abR", {3, 4, 512}, {"aR", "bR", "ab"}, "abR", PGM_RED_SUM, true);
  s.M = s.C;
  s.has_m = false;
  return s;
}
// a RATIO / DEN pair after a MUL operand
static Step step_ratio() {
  return mk_step("abR", {3, 4, 512}, {"abR", "aR", "aR"}, "aR", PGM_RED_SUM, true,
                 {PGM_PRODN_MUL, PGM_PRODN_RATIO, PGM_PRODN_DEN});
}
// the marginal divided by a row operand / by a row-less operand constant over the summed entries
static Step step_mdiv() { return mk_step("abR", {3, 4, 512}, {"abR", "aR"}, "aR", PGM_RED_SUM, true, {PGM_PRODN_MUL, PGM_PRODN_MDIV}); }
static Step step_mdiv_rowless() {
  return mk_step("abR", {3, 4, 512}, {"abR", "a"}, "aR", PGM_RED_MAX, false, {PGM_PRODN_MUL, PGM_PRODN_MDIV});
}
// XI = 2 (1,050 row pairs), a row operand varying over the reduced entries and one constant over them
static Step step_xi2() { return mk_step("abR", {5, 9, 2100}, {"abR", "aR", "ab"}, "aR", PGM_RED_SUM, true); }
// XI = 4: a 2-state reduction from 1,024 kept states x 2,000 row pairs
static Step step_xi4() { return mk_step("adbR", {32, 32, 2, 4000}, {"adb", "abR"}, "adR", PGM_RED_SUM, false); }
// a tiled kept dim: t (4 states) is carried by the row-less operand alone, 16,384 kept states
static Step step_tiled() { return mk_step("atrR", {4096, 4, 3, 128}, {"atr", "arR"}, "atR", PGM_RED_SUM, false); }
// 63 x 64 entries: one step below the 2^12 threshold (generic kernel); 64 x 64: at it
static Step step_below() { return mk_step("abR", {7, 9, 64}, {"abR", "b"}, "aR", PGM_RED_SUM, true); }
static Step step_at() { return mk_step("abR", {8, 8, 64}, {"abR", "b"}, "aR", PGM_RED_SUM, true); }

// two marginals in one pass: K = {k}, U = {u (M1 only), v (M2 only)}, Z = {z}; 256 blocks
static Step mk_two(std::vector<int64_t> card, int32_t reduce) {
  Step s = mk_step("kuvzR", card, {"kuvzR", "kz", "vR"}, "kuR", reduce, false);
  c_strides("kuvzR", card.data(), "kvR", s.ms2);
  s.M = kFakeM, s.M2 = kFakeM2;
  s.two = true;
  return s;
}
static Step step_two() { return mk_two({256, 2, 3, 2, 128}, PGM_RED_SUM); }
static Step step_two_max() { return mk_two({256, 3, 2, 2, 128}, PGM_RED_MAX); }  // M2 in registers
static Step step_two_odd() {  // an odd marginal stride
  Step s = step_two();
  s.ms[1] = 3;
  return s;
}
static Step step_two_acc() { return mk_two({256, 17, 18, 2, 128}, PGM_RED_SUM); }  // 17 accumulators
static Step step_two_few() { return mk_two({255, 2, 3, 2, 128}, PGM_RED_SUM); }    // 255 blocks

// a batch of contraction jobs (pgmi_cs_bind)
struct Batch {
  std::vector<pgmi_cs_job> jobs;
  std::vector<uint32_t> level_off;
  int one_wg = 0;
};

static FDiv fd(uint32_t d) { return FDiv{d, 0, 0}; }  // the generators read the divisor alone

static pgmi_cs_job blank_job(int kind, uint32_t block0, uint32_t nblocks) {
  pgmi_cs_job J;
  memset(&J, 0, sizeof J);
  J.kind = kind, J.block0 = block0, J.nblocks = nblocks;
  J.A = fake_op(0), J.B = fake_op(1), J.C = kFakeC;
  J.codes = (const uint8_t *)fake_op(2), J.err = (int32_t *)fake_op(3);
  for (int t = 0; t < MOPS; ++t) J.ops[t] = fake_op(t);
  return J;
}

// a pair job: kept dims kc (A / B / C strides ka / kb / kcs), reduction dims rc outermost first (the last
// one is the innermost dim, strides ra / rb)
static pgmi_cs_job pair_job(uint32_t block0, int cmb, int red, int g_log2, uint32_t row_mode, std::vector<uint32_t> kc,
                            std::vector<int64_t> ka, std::vector<int64_t> kb, std::vector<int64_t> kcs,
                            std::vector<uint32_t> rc, std::vector<int64_t> ra, std::vector<int64_t> rb) {
  pgmi_cs_job J = blank_job(0, block0, 1);
  J.cmb = cmb, J.red = red;
  ContractK &k = J.k;
  k.nk = (int32_t)kc.size(), k.nr = (int32_t)rc.size(), k.g_log2 = g_log2, k.n_split = 1, k.row_mode = row_mode;
  k.n_out = 1, k.n_red = 1, k.n_ro = 1;
  for (int i = 0; i < k.nk; ++i) k.kdiv[i] = fd(kc[i]), k.ksa[i] = ka[i], k.ksb[i] = kb[i], k.ksc[i] = kcs[i], k.n_out *= kc[i];
  for (int r = 0; r < k.nr; ++r) {
    k.n_red *= rc[r];
    if (r < k.nr - 1) k.rdiv[r] = fd(rc[r]), k.rsa[r] = ra[r], k.rsb[r] = rb[r], k.n_ro *= rc[r];
  }
  k.ri_card = rc.back(), k.ri_sa = ra.back(), k.ri_sb = rb.back();
  return J;
}

static pgmi_cs_job gather_job(uint32_t block0, std::vector<uint32_t> kc, std::vector<int64_t> ka, std::vector<int64_t> kcs,
                              int batch_dim, int n_ev) {
  pgmi_cs_job J = blank_job(1, block0, 1);
  GatherK &g = J.g;
  g.nk = (int32_t)kc.size(), g.n_ev = n_ev, g.batch_dim = batch_dim, g.n_out = 1, g.ld = 1000, g.row0 = 8;
  for (int i = 0; i < g.nk; ++i) g.kdiv[i] = fd(kc[i]), g.ksa[i] = ka[i], g.ksc[i] = kcs[i], g.n_out *= kc[i];
  for (int j = 0; j < n_ev; ++j) g.ev_col[j] = 2 * j + 1, g.ev_stride[j] = 100 * (j + 1), g.ev_card[j] = 3 + j;
  return J;
}

// an n-ary job of n_ops operands: operand t carries kept dim i iff bit i of kmask[t], reduced dim r iff bit r
// of rmask[t] (strides then 10^i-ish literals, distinct per operand)
static pgmi_cs_job nary_job(uint32_t block0, int n_ops, int red, int g_log2, std::vector<uint32_t> kc, std::vector<uint32_t> rc,
                            std::vector<unsigned> kmask, std::vector<unsigned> rmask) {
  pgmi_cs_job J = blank_job(2, block0, 1);
  ContractNK &k = J.n;
  k.n_ops = n_ops, k.nk = (int32_t)kc.size(), k.nr = (int32_t)rc.size(), k.red = red, k.g_log2 = g_log2;
  k.n_out = 1, k.n_red = 1;
  int64_t sc = 1;
  for (int i = k.nk - 1; i >= 0; --i) k.kcard[i] = kc[i], k.ksc[i] = sc, sc *= kc[i], k.n_out *= kc[i];
  for (int r = 0; r < k.nr; ++r) k.rcard[r] = rc[r], k.n_red *= rc[r];
  for (int t = 0; t < n_ops; ++t) {
    int64_t s = 1;
    for (int r = k.nr - 1; r >= 0; --r)
      if (rmask[t] >> r & 1) k.rs[t][r] = s, s *= rc[r];
    for (int i = k.nk - 1; i >= 0; --i)
      if (kmask[t] >> i & 1) k.ks[t][i] = s, s *= kc[i];
  }
  return J;
}

// one launch of pair jobs: every combine / reduce, G = 1, 4 and 64, row_mode 2, the unroll boundary of the
// reduction-outer loops (trip products 63 | 126, 64, 65)
static Batch batch_pairs() {
  Batch b;
  auto &j = b.jobs;
  j.push_back(pair_job(0, PGM_COMBINE_MUL, PGM_RED_SUM, 0, 0, {3, 5}, {5, 1}, {0, 1}, {5, 1}, {4}, {15}, {5}));
  j.push_back(pair_job(1, PGM_COMBINE_DIV, PGM_RED_MAX, 2, 0, {6}, {1}, {0}, {1}, {3, 10}, {60, 6}, {10, 1}));
  j.push_back(pair_job(2, PGM_COMBINE_COPY, PGM_RED_SUM, 6, 0, {2, 1, 4}, {4, 0, 1}, {0, 0, 0}, {4, 0, 1}, {200}, {8}, {0}));
  j.push_back(pair_job(3, PGM_COMBINE_ADD, PGM_RED_NONE, 0, 0, {7}, {1}, {1}, {1}, {1}, {0}, {0}));
  j.push_back(pair_job(4, PGM_COMBINE_DIV_RAW, PGM_RED_NONE, 3, 0, {7}, {1}, {0}, {1}, {1}, {0}, {0}));
  j.push_back(pair_job(5, PGM_COMBINE_MUL, PGM_RED_SUM, 0, 2, {3, 8}, {8, 1}, {1, 0}, {8, 1}, {2, 4}, {96, 24}, {12, 3}));
  j.push_back(pair_job(6, PGM_COMBINE_DIV_RAW, PGM_RED_NONE, 0, 2, {4}, {0}, {1}, {1}, {32}, {1}, {4}));
  j.push_back(pair_job(7, PGM_COMBINE_COPY, PGM_RED_MAX, 0, 2, {4}, {1}, {0}, {1}, {2}, {4}, {0}));
  j.push_back(pair_job(8, PGM_COMBINE_MUL, PGM_RED_SUM, 0, 0, {2}, {1}, {0}, {1}, {2, 9, 7}, {126, 14, 2}, {63, 7, 1}));
  j.push_back(pair_job(9, PGM_COMBINE_MUL, PGM_RED_SUM, 0, 0, {2}, {1}, {0}, {1}, {2, 8, 8}, {128, 16, 2}, {64, 8, 1}));
  j.push_back(pair_job(10, PGM_COMBINE_MUL, PGM_RED_SUM, 0, 0, {2}, {1}, {0}, {1}, {2, 13, 5}, {130, 10, 2}, {0, 5, 1}));
  j.push_back(pair_job(11, PGM_COMBINE_MUL, PGM_RED_MAX, 2, 0, {2}, {1}, {0}, {1}, {3, 16, 16}, {512, 32, 2}, {0, 16, 1}));
  j.push_back(pair_job(12, PGM_COMBINE_MUL, PGM_RED_SUM, 0, 0, {2}, {1}, {0}, {1}, {40}, {2}, {1}));
  return b;
}

// evidence gathers: a batch dim in the middle / first, none, no kept dim at all (one output)
static Batch batch_gathers() {
  Batch b;
  b.jobs.push_back(gather_job(0, {4, 100, 3}, {3, 0, 1}, {300, 3, 1}, 1, 2));
  b.jobs.push_back(gather_job(1, {100, 5}, {0, 1}, {5, 1}, 0, 1));
  b.jobs.push_back(gather_job(2, {6, 5}, {5, 1}, {5, 1}, -1, 0));
  b.jobs.push_back(gather_job(3, {}, {}, {}, -1, 3));
  return b;
}

// n-ary jobs: no reduction; G = 1 nested loops (unroll boundary 60 | 120); G = 4 split walk (sd 1 < nr 3) and
// flattened walk (sd == nr); G = 64 split and flattened; sum and max
static Batch batch_nary() {
  Batch b;
  auto &j = b.jobs;
  j.push_back(nary_job(0, 3, PGM_RED_SUM, 0, {4, 6}, {}, {3, 1, 2}, {0, 0, 0}));
  j.push_back(nary_job(1, 1, PGM_RED_SUM, 0, {}, {}, {0}, {0}));
  j.push_back(nary_job(2, 3, PGM_RED_SUM, 0, {5}, {2, 5, 12}, {1, 0, 1}, {7, 5, 2}));
  j.push_back(nary_job(3, 2, PGM_RED_MAX, 0, {5}, {7}, {1, 1}, {1, 0}));
  j.push_back(nary_job(4, 4, PGM_RED_SUM, 2, {3, 5}, {6, 4, 20}, {3, 2, 1, 0}, {7, 1, 6, 4}));
  j.push_back(nary_job(5, 2, PGM_RED_MAX, 2, {9}, {2, 3}, {1, 0}, {3, 2}));
  j.push_back(nary_job(6, 2, PGM_RED_SUM, 3, {9}, {2, 2, 5}, {1, 1}, {5, 6}));
  j.push_back(nary_job(7, 3, PGM_RED_SUM, 6, {2}, {64, 3}, {1, 0, 1}, {3, 1, 2}));
  j.push_back(nary_job(8, 2, PGM_RED_MAX, 6, {2}, {8, 16}, {1, 0}, {3, 3}));
  j.push_back(nary_job(9, 8, PGM_RED_SUM, 1, {2}, {2, 2}, {1, 0, 1, 0, 1, 0, 1, 0}, {1, 2, 3, 1, 2, 3, 1, 2}));
  return b;
}

// a single job in a launch of its own (no block-range tree); jobs spanning several blocks
static Batch batch_one() {
  Batch b;
  b.jobs.push_back(pair_job(0, PGM_COMBINE_MUL, PGM_RED_SUM, 0, 0, {3000}, {1}, {0}, {1}, {4}, {3000}, {1}));
  b.jobs[0].nblocks = 12;
  return b;
}

// the single-workgroup levelled form: levels of 2 jobs, no job, 1 job, 3 jobs
static Batch batch_levels() {
  Batch b;
  b.one_wg = 1;
  b.level_off = {0, 3, 3, 4, 9};
  b.jobs.push_back(pair_job(0, PGM_COMBINE_MUL, PGM_RED_SUM, 0, 0, {300}, {1}, {0}, {1}, {4}, {300}, {1}));
  b.jobs.push_back(gather_job(2, {10, 5}, {0, 1}, {5, 1}, 0, 1));
  b.jobs.push_back(nary_job(3, 2, PGM_RED_SUM, 0, {5}, {7}, {1, 1}, {1, 0}));
  b.jobs.push_back(pair_job(4, PGM_COMBINE_DIV, PGM_RED_NONE, 0, 0, {7}, {1}, {1}, {1}, {1}, {0}, {0}));
  b.jobs.push_back(nary_job(5, 3, PGM_RED_MAX, 2, {9}, {2, 3}, {1, 0, 1}, {3, 2, 1}));
  b.jobs.push_back(pair_job(8, PGM_COMBINE_COPY, PGM_RED_SUM, 0, 2, {4}, {1}, {0}, {1}, {2}, {4}, {0}));
  b.jobs[0].nblocks = 2, b.jobs[4].nblocks = 3;
  return b;
}

// n jobs of 9 pointers each (8-operand products without a reduction)
static Batch batch_ptrs(int n) {
  Batch b;
  for (int q = 0; q < n; ++q)
    b.jobs.push_back(nary_job((uint32_t)q, 8, PGM_RED_SUM, 0, {(uint32_t)(q % 7 + 2)}, {}, {1, 1, 1, 1, 1, 1, 1, 1},
                              {0, 0, 0, 0, 0, 0, 0, 0}));
  return b;
}
static Batch batch_args504() { return batch_ptrs(56); }   // the argument-array form's last size
static Batch batch_table513() { return batch_ptrs(57); }  // 513 pointers: through a table in device memory
static Batch batch_over() { return batch_ptrs(911); }     // 8,199 pointers: over the table budget, not taken
// forms the generator declines: a split reduction; a job outside the level table
static Batch batch_split() {
  Batch b = batch_one();
  b.jobs[0].k.n_split = 2;
  return b;
}
static Batch batch_outside() {
  Batch b = batch_levels();
  b.level_off = {0, 3, 3, 4, 8};
  return b;
}

// a case: one step, several steps merged (pgm_pm_merge), or a batch
struct Case {
  const char *name;
  std::vector<Step (*)()> steps;
  Batch (*batch)();
};

static const std::vector<Case> &cases() {
  static const std::vector<Case> c = {
      {"sum_store", {step_sum_store}, nullptr},
      {"max_store", {step_max_store}, nullptr},
      {"marg_only", {step_marg_only}, nullptr},
      {"product_only", {step_product_only}, nullptr},
      {"ratio", {step_ratio}, nullptr},
      {"mdiv", {step_mdiv}, nullptr},
      {"mdiv_rowless", {step_mdiv_rowless}, nullptr},
      {"xi2", {step_xi2}, nullptr},
      {"xi4", {step_xi4}, nullptr},
      {"tiled", {step_tiled}, nullptr},
      {"below", {step_below}, nullptr},
      {"at", {step_at}, nullptr},
      {"two", {step_two}, nullptr},
      {"two_max", {step_two_max}, nullptr},
      {"two_odd", {step_two_odd}, nullptr},
      {"two_acc", {step_two_acc}, nullptr},
      {"two_few", {step_two_few}, nullptr},
      {"merge1", {step_sum_store}, nullptr},  // pgm_pm_merge of one step: the step's own source
      {"merge2", {step_sum_store, step_max_store}, nullptr},
      {"merge3", {step_max_store, step_two, step_product_only}, nullptr},
      {"pairs", {}, batch_pairs},
      {"gathers", {}, batch_gathers},
      {"nary", {}, batch_nary},
      {"one", {}, batch_one},
      {"levels", {}, batch_levels},
      {"args504", {}, batch_args504},
      {"table513", {}, batch_table513},
      {"over", {}, batch_over},
      {"split", {}, batch_split},
      {"outside", {}, batch_outside},
  };
  return c;
}

// ---------------------------------------------------------------------------- the unit under test
struct Out {
  std::string src;  // empty: no specialised kernel
  std::vector<PMSpec> specs;
  std::vector<uint64_t> starts;
  uint64_t blocks = 0;
  CSBatch cs;
};

// plan -> specialise each step -> one source over them all (pgm_pm_merge; one step: the bind entry points)
static int gen_steps(const std::vector<Step> &steps, Out &o) {
  for (const Step &s : steps) {
    PMSpec sp;
    if (s.two) {
      const int r = plan_two_marginals(&s.d, s.ops, s.ms, s.ms2, s.M, s.M2, s.reduce, sp);
      if (r <= 0) return r;
    } else {
      ProdMK k;
      uint32_t grid[3];
      const int r = pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, grid);
      if (r <= 0) return r;
      if (!pm_specialise(k, s.reduce, s.C != nullptr, s.has_m, sp)) return 0;
    }
    o.specs.push_back(sp);
  }
  o.src = pm_source(o.specs, o.starts, &o.blocks);
  return 1;
}

static int gen_case(const Case &c, Out &o) {
  if (!c.batch) {
    std::vector<Step> steps;
    for (auto f : c.steps) steps.push_back(f());
    return gen_steps(steps, o);
  }
  const Batch b = c.batch();
  if (!cs_source(b.jobs.data(), (int)b.jobs.size(), b.level_off.data(), (int)b.level_off.size() - 1, b.one_wg, o.cs)) return 0;
  o.src = o.cs.src;
  return 1;
}

// ---------------------------------------------------------------------------- recorded sources
struct Golden {
  const char *name;
  size_t len;
  const char *sha;
};

// clang-format off
static const Golden kGolden[] = {
  {"sum_store", 1910, "afd74b51155f070781588258db3ae296efe5ce60638db3de7106d6817242724b"},
  {"max_store", 1908, "59f5ca51269365afb336448465e2e80ed212a4c11ece85453a0e8a8fbb866edd"},
  {"marg_only", 2099, "9b3154b3b66d8bbccf60f26824bf03d7f01f267ee1ddb69032de387a9dea4b50"},
  {"product_only", 1920, "adaf734d09c5bcdd93338211a6b6e1cb73e05ca3b0728afbb304b7f32ddfd601"},
  {"ratio", 2049, "fc56e8a3c0d97117997945b5dc00e1b4091a24e305e287aa0f9d52625b89a236"},
  {"mdiv", 1948, "56c6b18f63c0b3e0dce31454e8b76a9d428736d7a3736a5f31f4ba361faf5c06"},
  {"mdiv_rowless", 1891, "2cd27f775357ad8cb073739c8c6183a1292c32d370e76b105175e6007e298294"},
  {"xi2", 2557, "4fa4b59939bc76a9df1eb18bda95815509d400b6009461f7affa140cb415c7aa"},
  {"xi4", 2993, "331d3f900908270b2a53b1fd5aa64a57660958fa4ebe3d6bd0013b7649e196a8"},
  {"tiled", 2808, "59c5f7daad5ce80ce1823cdb98c056264262ad7a090b471babfb8c7dc5315d35"},
  {"below", 0, "-"},
  {"at", 1825, "4fa5ea80f3393a4e5b3bd2e10549667b1d855c08c97013ee01f01393b11725c9"},
  {"two", 2583, "78b15fcbb3dc82056ef40ad8086267df9d400b1c54c51528c887a8e48c7efc0c"},
  {"two_max", 2815, "137df79c08a2a8e66ae4ed2b47c8b502f972722069abd424860b382740155fa9"},
  {"two_odd", 0, "-"},
  {"two_acc", 0, "-"},
  {"two_few", 0, "-"},
  {"merge1", 1910, "afd74b51155f070781588258db3ae296efe5ce60638db3de7106d6817242724b"},
  {"merge2", 3343, "1c00af6c6e6cbe0462d4b6044829223015c3833207319afcd33189cbc9b5c72d"},
  {"merge3", 5468, "85f085c8c33b75f3c38055c0d82aaeb9c37b49b4e350d0f777ddbfb8f8d6c2cc"},
  {"pairs", 12680, "ba27d70b63e274ffaf2e0220497a42bf142b663566873db599d0c26a8fd5b9c9"},
  {"gathers", 3943, "1933b0440a2fa5a6dc65ca98eba2a83ff818404e535bb531e1a0f4aef367e874"},
  {"nary", 11852, "0be9a527e6a6c9f78fa925e7dad6ee05f27c9550245e44c9dc89fb32868a911b"},
  {"one", 1145, "b26f3330deae6375d95df028f6f877362ce6553b31d58e2e19f1b358a145858e"},
  {"levels", 5644, "129d03217db09ac9bccc6cd09d997aaebb219eaa118b9a29d9a22d040e8e1dd5"},
  {"args504", 67845, "9cb71e1c8e314e9437bd989c66745b26d4c8c4f4600f9d252896f472b7b64f70"},
  {"table513", 69075, "95865014c82be3ce8c213be1e10584ae43f7113b9960919ca84f2fc49d131295"},
  {"over", 0, "-"},
  {"split", 0, "-"},
  {"outside", 0, "-"},
};
// clang-format on

static int print_cases(const char *dump_dir) {
  for (const Case &c : cases()) {
    Out o;
    const int r = gen_case(c, o);
    if (r < 0) {
      printf("%s: %s\n", c.name, g_last_err.c_str());
      continue;
    }
    printf("  {\"%s\", %zu, \"%s\"},\n", c.name, o.src.size(), o.src.empty() ? "-" : sha256(o.src.data(), o.src.size()).c_str());
    if (dump_dir && !o.src.empty()) {
      const std::string path = std::string(dump_dir) + "/" + c.name + ".hip";
      FILE *f = fopen(path.c_str(), "wb");
      if (!f || fwrite(o.src.data(), 1, o.src.size(), f) != o.src.size()) return 1;
      fclose(f);
    }
  }
  return 0;
}

static int test_recorded() {
  const std::vector<Case> &cs = cases();
  CHECK(cs.size() == sizeof kGolden / sizeof kGolden[0]);
  for (size_t i = 0; i < cs.size(); ++i) {
    const Golden &g = kGolden[i];
    CHECK(!strcmp(cs[i].name, g.name));
    Out o;
    g_last_err.clear();
    const int r = gen_case(cs[i], o);
    if (r < 0) {
      fprintf(stderr, "%s: %s\n", g.name, g_last_err.c_str());
      return 1;
    }
    CHECK((r == 0) == o.src.empty());
    const std::string sha = o.src.empty() ? "-" : sha256(o.src.data(), o.src.size());
    if (o.src.size() != g.len || sha != g.sha) {
      fprintf(stderr, "%s: generated source differs from the recorded one (%zu bytes, %s)\n", g.name, o.src.size(), sha.c_str());
      return 1;
    }
  }
  return 0;
}

static const Case &case_of(const char *name) {
  for (const Case &c : cases())
    if (!strcmp(c.name, name)) return c;
  return cases()[0];
}

// ---------------------------------------------------------------------------- plans and specialisation
static int test_plan() {
  // the planner: kept dims, reduced dims, the row dim last, the generic kernel's grid
  Step s = step_marg_only();
  ProdMK k;
  uint32_t g[3] = {0, 0, 0};
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 1);
  CHECK(k.n_ops == 3 && k.nk == 2 && k.nr == 2 && k.n_red == 8 && k.n_outer == 3 && k.NP == 256 && k.mdiv == -1);
  CHECK(k.kdiv[0].d == 3 && k.kdiv[1].d == 512 && k.rdiv[0].d == 2 && k.rdiv[1].d == 4);
  CHECK(k.kdiv[0].m == make_fdiv(3).m && k.kdiv[0].s == 2);
  CHECK(k.vec[0] == 1 && k.vec[1] == 0 && k.vec[2] == 1 && k.jvar[0] == 1 && k.jvar[1] == 1 && k.jvar[2] == 1);
  CHECK(k.ksc[0] == 8 * 512 && k.ksm[0] == 512 && k.ks[1][0] == 0 && k.ks[2][0] == 4 * 512);
  CHECK(k.rsc[0] == 4 * 512 && k.rsc[1] == 512 && k.rs[1][0] == 4 && k.rs[1][1] == 1 && k.rs[2][0] == 0 && k.rs[2][1] == 512);
  CHECK(k.ops[0] == fake_op(0) && k.ops[3] == fake_op(0));  // unused slots alias operand 0
  CHECK(g[0] == 1 && g[1] == 3 && g[2] == 1);
  s = step_mdiv();
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 1 && k.mdiv == 1 && k.kind[1] == PGM_PRODN_MUL);
  // the grid: 65,535 rows of blocks at most, 2,048 blocks aimed at
  s = mk_step("aR", {100000, 64}, {"aR"}, "aR", PGM_RED_SUM, true);
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 1 && g[0] == 1 && g[1] == 65535);
  s = mk_step("aR", {4, 1 << 20}, {"aR"}, "aR", PGM_RED_SUM, true);
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 1 && g[0] == 512 && g[1] == 4);
  // shapes the fused kernel does not take, and errors
  s = step_sum_store();
  s.d.keep_card[2] = 62;
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 0);  // fewer than 64 rows
  s = step_sum_store();
  s.C = (double *)((uintptr_t)s.C + 8);
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 0);  // C at 8 mod 16
  s = mk_step("abR", {3, RMAX_MARG + 1, 64}, {"abR"}, "aR", PGM_RED_SUM, true);
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 0);  // more than RMAX_MARG reduced entries
  s = mk_step("abR", {3, 4, 512}, {"abR", "bR"}, "aR", PGM_RED_SUM, true, {PGM_PRODN_MUL, PGM_PRODN_MDIV});
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 0);  // the divisor varies over the summed entries
  s = step_sum_store();
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, nullptr, k, g) == PGM_EINVAL);
  CHECK(g_last_err == "product_n_marginal: null argument");
  s.d.op_kind[1] = 7;
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == PGM_EINVAL && g_last_err == "product_n_marginal: operand 1");
  s = step_mdiv();
  s.d.op_kind[0] = PGM_PRODN_MDIV;
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == PGM_EINVAL);
  CHECK(g_last_err == "product_n_marginal: more than one PGM_PRODN_MDIV operand");
  s = step_sum_store();
  s.d.keep_card[0] = 0;
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == PGM_EINVAL && g_last_err == "product_n_marginal: keep_card[0] <= 0");
  return 0;
}

struct SpecWant {
  const char *name;
  int XI, unroll, tdim;
  unsigned T, gx;
  uint64_t total;
  bool store, has_m;
};

static int test_specialise() {
  // XI: 2 from 512 row pairs; doubled while reduced entries x XI < 8, >= 2,048 blocks remain and the padding
  // stays under a quarter.  unroll: 8, fewer with many row operands varying over the reduced entries
  const SpecWant want[] = {
      {"sum_store", 1, 8, -1, 1, 1, 3, true, true},     {"max_store", 1, 8, -1, 1, 2, 8, true, true},
      {"marg_only", 1, 8, -1, 1, 1, 3, false, true},    {"product_only", 1, 8, -1, 1, 1, 12, true, false},
      {"ratio", 1, 8, -1, 1, 1, 3, true, true},         {"mdiv", 1, 8, -1, 1, 1, 3, true, true},
      {"xi2", 2, 8, -1, 1, 3, 15, true, true},          {"xi4", 4, 8, -1, 1, 2, 2048, false, true},
      {"tiled", 1, 8, 1, 4, 1, 4096, false, true},      {"at", 1, 8, -1, 1, 1, 8, true, true},
  };
  for (const SpecWant &w : want) {
    Out o;
    CHECK(gen_case(case_of(w.name), o) == 1 && o.specs.size() == 1);
    const PMSpec &sp = o.specs[0];
    if (sp.XI != w.XI || sp.unroll != w.unroll || sp.tdim != w.tdim || sp.T != w.T || sp.gx != w.gx || sp.total != w.total ||
        sp.store != w.store || sp.has_m != w.has_m) {
      fprintf(stderr, "%s: XI %d unroll %d tdim %d T %u gx %u total %llu store %d has_m %d\n", w.name, sp.XI, sp.unroll, sp.tdim,
              sp.T, sp.gx, (unsigned long long)sp.total, (int)sp.store, (int)sp.has_m);
      return 1;
    }
    CHECK(sp.multi == 0 && sp.xcd && sp.nt && o.blocks == w.total && o.starts == std::vector<uint64_t>({0}));
    CHECK(pm_nops(sp) == sp.k.n_ops);
  }
  // 48 / (row operands varying over the reduced entries x XI) entries unrolled: 4 such operands, XI 2 -> 6
  Step s = mk_step("abR", {5, 9, 2100}, {"abR", "abR", "bR", "abR", "a"}, "aR", PGM_RED_SUM, true);
  ProdMK k;
  uint32_t g[3];
  PMSpec sp;
  CHECK(pgmi_plan_product_marg(&s.d, s.ops, s.C, s.ms, s.M, k, g) == 1 && pm_specialise(k, PGM_RED_SUM, true, true, sp));
  CHECK(sp.XI == 2 && sp.unroll == 6);
  // one step below the entries threshold: the generic kernel
  Out o;
  CHECK(gen_case(case_of("below"), o) == 0 && o.src.empty());
  // the XCD remap's two forms
  CHECK(gen_case(case_of("max_store"), o) == 1 && o.src.find("b = (b % 8u) * 1u + b / 8u;") != std::string::npos);
  Out o3;
  CHECK(gen_case(case_of("sum_store"), o3) == 1 && o3.src.find("{ const unsigned x = b % 8u, y = b / 8u;") != std::string::npos);
  return 0;
}

static int test_two_marginals() {
  Out o;
  CHECK(gen_case(case_of("two"), o) == 1 && o.specs.size() == 1);
  const PMSpec &sp = o.specs[0];
  const PMMulti &q = sp.mm;
  CHECK(sp.multi == 1 && !sp.store && sp.xcd && sp.gx == 1 && sp.total == 256 && o.blocks == 256 && pm_nops(sp) == 3);
  CHECK(q.n_ops == 3 && q.nK == 1 && q.nU == 2 && q.nZ == 1 && q.n1 == 2 && q.n2 == 3 && q.n_outer == 256 && q.NP == 64);
  CHECK(q.kcard[0] == 256 && q.ucard[0] == 2 && q.ucard[1] == 3 && q.zcard[0] == 2);
  CHECK(q.k1[0] == 2 * 128 && q.k2[0] == 3 * 128 && q.u1[0] == 128 && q.u2[0] == 0 && q.u1[1] == 0 && q.u2[1] == 128);
  CHECK(q.vec[0] == 1 && q.vec[1] == 0 && q.vec[2] == 1 && q.zs[1][0] == 1 && q.us[2][1] == 128);
  for (const char *name : {"two_odd", "two_acc", "two_few"}) {
    Out r;
    CHECK(gen_case(case_of(name), r) == 0 && r.src.empty());
  }
  Step s = step_two();
  PMSpec e;
  CHECK(plan_two_marginals(&s.d, s.ops, s.ms, s.ms2, s.M, nullptr, s.reduce, e) == PGM_EINVAL);
  CHECK(g_last_err == "product_n_marginals: null argument");
  return 0;
}

static int test_merge() {
  // starts padded to multiples of 8; the pointer count of the argument struct
  Out o;
  CHECK(gen_case(case_of("merge2"), o) == 1);
  CHECK(o.starts == std::vector<uint64_t>({0, 8}) && o.blocks == 16);
  CHECK(o.src.find("struct pgm_pm_args { const double *p[8]; };") != std::string::npos);
  Out o3;
  CHECK(gen_case(case_of("merge3"), o3) == 1);
  CHECK(o3.starts == std::vector<uint64_t>({0, 8, 264}) && o3.blocks == 276);
  CHECK(o3.src.find("struct pgm_pm_args { const double *p[14]; };") != std::string::npos);
  CHECK(o3.src.find("  if (b < 8u) {\n    if (b < 8u) pm0(b - 0u") != std::string::npos);
  CHECK(o3.src.find("    if (b < 264u) {\n      if (b < 264u) pm1(b - 8u") != std::string::npos);
  Out o1, os;
  CHECK(gen_case(case_of("merge1"), o1) == 1 && gen_case(case_of("sum_store"), os) == 1 && o1.src == os.src);
  return 0;
}

// ---------------------------------------------------------------------------- batches
static int test_batches() {
  struct Want {
    const char *name;
    unsigned blocks, threads;
    size_t nptr;
    bool table;
  };
  const Want want[] = {
      {"pairs", 13, 256, 39, false}, {"gathers", 4, 256, 16, false},   {"nary", 10, 256, 40, false},
      {"one", 12, 256, 3, false},    {"levels", 1, 1024, 20, false},   {"args504", 56, 256, 504, false},
      {"table513", 57, 256, 513, true},
  };
  for (const Want &w : want) {
    Out o;
    CHECK(gen_case(case_of(w.name), o) == 1);
    if (o.cs.blocks != w.blocks || o.cs.threads != w.threads || o.cs.ptrs.size() != w.nptr || o.cs.table != w.table) {
      fprintf(stderr, "%s: blocks %u threads %u pointers %zu table %d\n", w.name, o.cs.blocks, o.cs.threads, o.cs.ptrs.size(),
              (int)o.cs.table);
      return 1;
    }
  }
  for (const char *name : {"over", "split", "outside"}) {
    Out o;
    CHECK(gen_case(case_of(name), o) == 0 && o.src.empty());
  }
  // the flat pointer list: per job A, B, C / A, codes, C, err / its operands, C
  Out o;
  CHECK(gen_case(case_of("levels"), o) == 1);
  const std::vector<const double *> p = {fake_op(0), fake_op(1), kFakeC, fake_op(0), fake_op(2), kFakeC, fake_op(3),
                                         fake_op(0), fake_op(1), kFakeC, fake_op(0), fake_op(1), kFakeC,
                                         fake_op(0), fake_op(1), fake_op(2), kFakeC, fake_op(0), fake_op(1), kFakeC};
  CHECK(o.cs.ptrs == p);
  CHECK(o.src.find("  for (unsigned b = 3u + vb; b < 3u; b += 4u) {\n  }\n  __syncthreads();\n") != std::string::npos);
  CHECK(gen_case(case_of("table513"), o) == 1);
  CHECK(o.src.find("struct pgm_pm_args { const double *const *__restrict__ p; };\n") != std::string::npos);
  // no batch at all
  CSBatch none;
  CHECK(!cs_source(nullptr, 0, nullptr, 0, 0, none));
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--print")) return print_cases(nullptr);
  if (argc > 2 && !strcmp(argv[1], "--dump")) return print_cases(argv[2]);
  CHECK(sha256("abc", 3) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
  CHECK(sha256("abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", 56) ==
        "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1");  // two blocks
  if (test_recorded() || test_plan() || test_specialise() || test_two_marginals() || test_merge() || test_batches()) return 1;
  printf("pm_gen_selftest ok\n");
  return 0;
}

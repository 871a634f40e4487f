// rows_plan_selftest.cpp — the host side of the fused row plan (pgmpy_amd/csrc/pgmrows_plan.cpp: plan
// compiler, generator of the plan-specialised kernel source, two-rows-per-thread predicates, launch choice) on the
// CPU, against hand-built pgm_rows_plan structs.  Links that unit alone; meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I include -I pgmpy_amd/csrc
//       tools/rows_plan_selftest.cpp pgmpy_amd/csrc/pgmrows_plan.cpp -o rows_plan_selftest
// Exit status 0 and "rows_plan_selftest ok" when every check holds.  `--print` lists, per plan, what
// the unit under test computes (descriptor words / SHA-256, source length / SHA-256) and checks nothing;
// `--source CASE WORD` writes a case's source under a cache-policy word (test_stream_policy) to stdout.
//
// The expected descriptor and source hashes below were recorded from the monolithic pgmhip.hip this
// unit was split out of (its pgm_rows_plan_create / pgm_rows_plan_source on the same structs), so
// they pin the split to that code word for word and byte for byte.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pgmhip.h"
#include "pgm_internal.h"
#include "pgm_rows.h"

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

// ---------------------------------------------------------------------------- hand-built plans
static int add_loop(pgm_rows_plan &p, int card, int marg_off, int map_stride) {
  const int k = p.n_loop++;
  p.loop_card[k] = card;
  p.loop_marg_off[k] = marg_off;
  p.loop_map_stride[k] = map_stride;
  return k;
}

// a factor at `base`; its evidence terms are the add_ev calls that follow
static int add_fac(pgm_rows_plan &p, int base) {
  const int f = p.n_fac++;
  p.fac_base[f] = base;
  p.fac_ev_begin[f] = p.fac_ev_end[f] = p.n_ev;
  return f;
}

static void add_ev(pgm_rows_plan &p, int col, int stride, int card) {
  const int j = p.n_ev++;
  p.ev_col[j] = col;
  p.ev_stride[j] = stride;
  p.ev_card[j] = card;
  p.fac_ev_end[p.n_fac - 1] = p.n_ev;
}

// the loops / factors added since the last component; the first nq of its loops are query dims
static void end_comp(pgm_rows_plan &p, int nq) {
  const int c = p.n_comp++;
  p.comp_loop_begin[c] = c ? p.comp_loop_end[c - 1] : 0;
  p.comp_n_query[c] = nq;
  p.comp_loop_end[c] = p.n_loop;
  p.comp_fac_begin[c] = c ? p.comp_fac_end[c - 1] : 0;
  p.comp_fac_end[c] = p.n_fac;
  p.n_query += nq;
}

static pgm_rows_plan blank() {
  pgm_rows_plan p;
  memset(&p, 0, sizeof p);
  return p;
}

// one affine component: query card 3 (stride 2), one factor, one evidence term (column 2, card 2)
static pgm_rows_plan plan_affine_nq1() {
  pgm_rows_plan p = blank();
  add_loop(p, 3, 0, 1);
  const int f = add_fac(p, 0);
  p.fac_stride[f][0] = 2;
  add_ev(p, 2, 1, 2);
  end_comp(p, 1);
  p.n_values = 6, p.n_marg = 3, p.n_joint = 3;
  return p;
}

// a component without a query dim (P = 1): the probability of the evidence only
static pgm_rows_plan plan_nq0() {
  pgm_rows_plan p = blank();
  add_fac(p, 0);
  add_ev(p, 0, 1, 4);
  end_comp(p, 0);
  p.n_values = 4, p.n_marg = 0, p.n_joint = 1;
  return p;
}

// two components; the second one's two factors read the same evidence column (0)
static pgm_rows_plan plan_two_comp() {
  pgm_rows_plan p = blank();
  add_loop(p, 2, 0, 3);
  int f = add_fac(p, 0);  // [q0 2][e 3]
  p.fac_stride[f][0] = 3;
  add_ev(p, 1, 1, 3);
  end_comp(p, 1);
  add_loop(p, 3, 2, 1);
  f = add_fac(p, 6);  // [e 2][q1 3]
  p.fac_stride[f][1] = 1;
  add_ev(p, 0, 3, 2);
  f = add_fac(p, 12);  // [q1 3][e 2]
  p.fac_stride[f][1] = 2;
  add_ev(p, 0, 1, 2);
  end_comp(p, 1);
  p.n_values = 18, p.n_marg = 5, p.n_joint = 6;
  return p;
}

// a table component: two query dims, cards 2 x 3, one factor [q0 2][e 2][q1 3]
static pgm_rows_plan plan_table_2x3() {
  pgm_rows_plan p = blank();
  add_loop(p, 2, 0, 3);
  add_loop(p, 3, 2, 1);
  const int f = add_fac(p, 0);
  p.fac_stride[f][0] = 6;
  p.fac_stride[f][1] = 1;
  add_ev(p, 0, 3, 2);
  end_comp(p, 2);
  p.n_values = 12, p.n_marg = 5, p.n_joint = 6;
  return p;
}

// a table component with a hidden dim: query card 2, hidden card 3, factors [q 2][h 3] and [h 3][e 2]
static pgm_rows_plan plan_table_hidden() {
  pgm_rows_plan p = blank();
  add_loop(p, 2, 0, 1);
  add_loop(p, 3, -1, 0);
  int f = add_fac(p, 0);
  p.fac_stride[f][0] = 3;
  p.fac_stride[f][1] = 1;
  f = add_fac(p, 6);
  p.fac_stride[f][1] = 2;
  add_ev(p, 4, 1, 2);
  end_comp(p, 1);
  p.n_values = 12, p.n_marg = 2, p.n_joint = 2;
  return p;
}

// one affine component (query card 2) with nt evidence terms of card 2 over two factors: the first
// takes ceil(nt / 2) of them, the second the rest; term j reads column 2 j
static pgm_rows_plan plan_terms(int nt) {
  pgm_rows_plan p = blank();
  add_loop(p, 2, 0, 1);
  const int n0 = (nt + 1) / 2, n1 = nt - n0;
  int f = add_fac(p, 0);  // [q 2][e ...]
  p.fac_stride[f][0] = 1 << n0;
  for (int j = 0; j < n0; ++j) add_ev(p, 2 * j, 1 << (n0 - 1 - j), 2);
  f = add_fac(p, 2 << n0);  // [e ...][q 2]
  p.fac_stride[f][0] = 1;
  for (int j = 0; j < n1; ++j) add_ev(p, 2 * (n0 + j), 2 << (n1 - 1 - j), 2);
  end_comp(p, 1);
  p.n_values = (2 << n0) + (2 << n1), p.n_marg = 2, p.n_joint = 2;
  return p;
}
static pgm_rows_plan plan_terms0() { return plan_terms(0); }
static pgm_rows_plan plan_terms3() { return plan_terms(3); }
static pgm_rows_plan plan_terms4() { return plan_terms(4); }
static pgm_rows_plan plan_terms5() { return plan_terms(5); }
static pgm_rows_plan plan_terms8() { return plan_terms(8); }
static pgm_rows_plan plan_terms9() { return plan_terms(9); }

// 8,000 CPT values (+ the 1.0): more than 48 KiB, so the generated kernels gather from global memory
static pgm_rows_plan plan_big_values() {
  pgm_rows_plan p = blank();
  add_loop(p, 32, 0, 1);
  const int f = add_fac(p, 0);  // [q 32][e 250]
  p.fac_stride[f][0] = 250;
  add_ev(p, 1, 1, 250);
  end_comp(p, 1);
  p.n_values = 8000, p.n_marg = 32, p.n_joint = 32;
  return p;
}

// the second component has no factor at all (fe == fb): its products are the constant 1.0
static pgm_rows_plan plan_no_factor() {
  pgm_rows_plan p = blank();
  add_loop(p, 2, 0, 2);
  const int f = add_fac(p, 0);
  p.fac_stride[f][0] = 1;
  end_comp(p, 1);
  add_loop(p, 2, 2, 1);
  end_comp(p, 1);
  p.n_values = 2, p.n_marg = 4, p.n_joint = 4;
  return p;
}

struct Case {
  const char *name;
  pgm_rows_plan (*make)();
  // recorded from the monolith: descriptor buffer (words, SHA-256 of the words followed by RowsK),
  // the handle's flags, the generated source ("" for table plans: none)
  size_t desc_words;
  const char *desc_sha;
  int max_nf, max_nt, any_table, all_affine, n_cols;
  size_t src_len;
  const char *src_sha;
};

// clang-format off
static const Case kCases[] = {
  {"affine_nq1", plan_affine_nq1, 117, "45ebf76692d20084680e4b7afc4462352a3cc59b951795e35c01f7e853001ab1", 1, 1, 0, 1, 3, 15006, "6f89f09d60d7ea3a9ad6a4c8061a831603bcf98eecd7998009908e844e8fbb57"},
  {"nq0", plan_nq0, 117, "f5150b46893a3dbda6173ace215ff454f0bde6ef2352f20fe225681ce8347d2d", 1, 1, 0, 1, 1, 12239, "b618144887b3341c7bc0f211416a1115a1a110e7b6d622a40cb59b890689c0b5"},
  {"two_comp", plan_two_comp, 229, "a75d6e63695f4d10dfbda6f8ed63fa027c1c5589f712175e9d22b4a3c1a5792b", 2, 2, 0, 1, 2, 20222, "bea0ada2de6e97608a8a86d4d6bba08a4add3385c824e62f3a6b3fda181ea1cf"},
  {"table_2x3", plan_table_2x3, 141, "dce117003974c25e4da08af5a89d3e62d3e8105c449d7b0b121b1eda940197f8", 1, 1, 1, 0, 1, 0, ""},
  {"table_hidden", plan_table_hidden, 133, "7fc5f03f3efc6fa35ae4e630ae1ec6e1a4df13528f2d266968309a11fa73a75b", 2, 1, 1, 0, 5, 0, ""},
  {"terms0", plan_terms0, 101, "be6c6c5f2ce678b49460259a136f02416886d7ddf7447fb3ecf8fa3548014d85", 2, 0, 0, 1, 0, 13172, "0897bc90683d77fb7d054686bc77c5e5388dfb576e4155ed0f12e3d62e062fb8"},
  {"terms3", plan_terms3, 117, "0af1ffd43a31ac949675f657d41ea807d2de02a204c9736177b5a14cdbfd139a", 2, 3, 0, 1, 5, 16154, "3a58ae7bdf99ddb0a3362625acd4399ab98a646e7e29aa8364edec42bf0d61f6"},
  {"terms4", plan_terms4, 117, "d6a1125d356470478d5aa79ec607c7b10d114b94d41d628585398887d341d6e6", 2, 4, 0, 1, 7, 17073, "94bd03b4130a247ff4668c043157d914792bd0042ff37c1cb245467458b5de00"},
  {"terms5", plan_terms5, 133, "e3dfedaa3822b0371202d9ee81a1d02b2602a646a0c1741588613109ae9cac69", 2, 5, 0, 1, 9, 17997, "fb11de21e0a712e989f3273e006c0bfcc70d32da7f27141fbcd882acfa1ff761"},
  {"terms8", plan_terms8, 133, "b220aa613b2bbed651ac70f5ac3a0efbb7f9b748a71b2e7eafc9e0e0ecae1e01", 2, 8, 0, 1, 15, 20779, "1df71f30de1d5beae74adab55f414574e636215bd4d5e04b2956f830dc5d208e"},
  {"terms9", plan_terms9, 137, "6a57d88adeefbc309bd86e77b0278380dff38cecca6dbb08afc6630fc3bb94fe", 2, 9, 0, 0, 17, 21708, "feea5e3189f137b654b3aa9c812140f3b71edeae9dcec99bf46f5fecbe813f66"},
  {"big_values", plan_big_values, 117, "91d52d9af38145b2836fd4896286df9f584c0f9b0613530ba0b91c16853fd190", 1, 1, 0, 1, 2, 47640, "3fb3367da4f6534d2e7f237167d1bcc0fdbd38b04723b9c4c4ad2f100c9b234a"},
  {"no_factor", plan_no_factor, 197, "8566e68c12f6dd5581e4b783e2c27a5d629b29a3a591a836c430cbb0ccc0c3e7", 1, 0, 0, 1, 0, 16127, "96dc97e50d15d497732f6f4f107e0dcda745952a40336a0679dcf6b355047caa"},
};
// clang-format on
static const size_t kNumCases = sizeof kCases / sizeof kCases[0];

static std::string plan_sha(const RowsPlan &r) {
  std::vector<uint8_t> b(r.desc.size() * 4 + sizeof r.k);
  if (!r.desc.empty()) memcpy(b.data(), r.desc.data(), r.desc.size() * 4);
  memcpy(b.data() + r.desc.size() * 4, &r.k, sizeof r.k);
  return sha256(b.data(), b.size());
}

static int print_cases() {
  for (size_t i = 0; i < kNumCases; ++i) {
    const pgm_rows_plan p = kCases[i].make();
    RowsPlan r;
    if (rows_plan_compile(&p, r) != PGM_OK) {
      printf("%s: %s\n", kCases[i].name, g_last_err.c_str());
      continue;
    }
    printf("  {\"%s\", plan_%s, %zu, \"%s\", %d, %d, %d, %d, %d, %zu, \"%s\"},\n", kCases[i].name, kCases[i].name,
           r.desc.size(), plan_sha(r).c_str(), r.max_nf, r.max_nt, (int)r.any_table, (int)r.all_affine, r.n_cols,
           r.jit_src.size(), r.jit_src.empty() ? "" : sha256(r.jit_src.data(), r.jit_src.size()).c_str());
  }
  return 0;
}

// ---------------------------------------------------------------------------- descriptors, word for word
static const RowsTerm kNoop{0, 0, 256, -1};  // the trailing term

static bool same_term(const RowsTerm &a, const RowsTerm &b) {
  return a.col == b.col && a.stride == b.stride && a.card == b.card && a.slot == b.slot;
}

static const RowsComp *comps_of(const RowsPlan &r) { return (const RowsComp *)r.desc.data(); }
static const RowsTerm *terms_of(const RowsPlan &r) { return (const RowsTerm *)(r.desc.data() + r.k.terms_off); }
static const int32_t *tab_of(const RowsPlan &r) { return r.desc.data() + r.k.tab_off; }

static int test_recorded() {
  for (size_t i = 0; i < kNumCases; ++i) {
    const Case &c = kCases[i];
    const pgm_rows_plan p = c.make();
    RowsPlan r;
    g_last_err.clear();
    if (rows_plan_compile(&p, r) != PGM_OK) {
      fprintf(stderr, "%s: %s\n", c.name, g_last_err.c_str());
      return 1;
    }
    if (r.desc.size() != c.desc_words || plan_sha(r) != c.desc_sha || r.max_nf != c.max_nf || r.max_nt != c.max_nt ||
        (int)r.any_table != c.any_table || (int)r.all_affine != c.all_affine || r.n_cols != c.n_cols) {
      fprintf(stderr, "%s: descriptor differs from the recorded one (%zu words, %s)\n", c.name, r.desc.size(),
              plan_sha(r).c_str());
      return 1;
    }
    CHECK(r.desc.back() == 0);  // the trailing 0 after the tables
    CHECK(r.k.terms_off == (int)(p.n_comp * sizeof(RowsComp) / 4) && r.k.tab_off <= (int)r.desc.size() - 1);
    CHECK(same_term(terms_of(r)[(r.k.tab_off - r.k.terms_off) / 4 - 1], kNoop));
    CHECK(r.jit_src.empty() == (r.any_table != 0));
    // the source: through the compiler and through pgm_rows_plan_source's check, both as recorded
    std::string src;
    const int st = rows_plan_source(&p, src);
    if (r.any_table) {
      CHECK(st == PGM_EINVAL && c.src_len == 0);
      continue;
    }
    CHECK(st == PGM_OK && src == r.jit_src);
    if (src.size() != c.src_len || sha256(src.data(), src.size()) != c.src_sha) {
      fprintf(stderr, "%s: generated source differs from the recorded one (%zu bytes, %s)\n", c.name, src.size(),
              sha256(src.data(), src.size()).c_str());
      return 1;
    }
    CHECK(src.find("#define BACKOFF 1\n") != std::string::npos);
  }
  return 0;
}

static int test_affine_nq1() {
  const pgm_rows_plan p = plan_affine_nq1();
  RowsPlan r;
  CHECK(rows_plan_compile(&p, r) == PGM_OK);
  RowsK k;
  memset(&k, 0, sizeof k);
  k.n_values = 7, k.n_marg = 3, k.n_joint = 3, k.n_comp = 1, k.n_waves = 0;
  k.terms_off = 96, k.tab_off = 96 + 5 * 4, k.one_idx = 6;
  k.q_marg_off[0] = 0, k.q_card[0] = 3;
  CHECK(memcmp(&k, &r.k, sizeof k) == 0);
  CHECK(sizeof(RowsComp) == 96 * 4 && r.desc.size() == 96 + 5 * 4 + 1);
  RowsComp e;
  memset(&e, 0, sizeof e);
  e.nf = 1, e.nt = 1, e.P = 3, e.H = 1, e.simple = 1, e.mstride = 1, e.q_lo = 0, e.q_hi = 1;
  e.off_base = 0, e.marg_base = 0, e.map_base = 0, e.ev_lo = 0, e.val_lo = 0, e.val_hi = 6, e.marg0 = 0, e.nq = 1;
  for (int j = 0; j < PGM_ROWS_MAX_FAC; ++j) e.fbase[j] = 6;  // unused slots: the trailing 1.0
  e.fbase[0] = 0, e.fstride[0] = 2;
  e.a_S[0][0] = 1;
  for (int j = 0; j < 8; ++j) e.a_col[j] = 2, e.a_card[j] = 256;  // padding terms re-read a real column
  e.a_card[0] = 2;
  CHECK(memcmp(&e, comps_of(r), sizeof e) == 0);
  const RowsTerm *t = terms_of(r);
  CHECK(same_term(t[0], RowsTerm{2, 1, 2, 0}));
  for (int j = 1; j < 4; ++j) CHECK(same_term(t[j], RowsTerm{2, 0, 256, -1}));  // padded to 4
  CHECK(same_term(t[4], kNoop) && tab_of(r)[0] == 0);
  CHECK(r.max_nf == 1 && r.max_nt == 1 && !r.any_table && r.all_affine && r.n_cols == 3);
  CHECK(r.cols == std::vector<int>({2}));
  return 0;
}

static int test_nq0() {
  const pgm_rows_plan p = plan_nq0();
  RowsPlan r;
  CHECK(rows_plan_compile(&p, r) == PGM_OK);
  const RowsComp &c = comps_of(r)[0];
  CHECK(c.nf == 1 && c.nt == 1 && c.P == 1 && c.H == 1 && c.simple == 1 && c.mstride == 0 && c.nq == 0);
  CHECK(c.q_lo == 0 && c.q_hi == 0 && c.marg0 == 0 && c.val_lo == 0 && c.val_hi == 4);
  CHECK(c.fbase[0] == 0 && c.fstride[0] == 0 && c.fbase[1] == 4 && c.a_S[0][0] == 1 && c.a_card[0] == 4);
  CHECK(r.k.n_values == 5 && r.k.one_idx == 4 && r.k.n_marg == 0 && r.all_affine && r.n_cols == 1);
  return 0;
}

static int test_two_comp() {
  const pgm_rows_plan p = plan_two_comp();
  RowsPlan r;
  CHECK(rows_plan_compile(&p, r) == PGM_OK);
  const RowsComp *c = comps_of(r);
  CHECK(c[0].q_lo == 0 && c[0].q_hi == 1 && c[1].q_lo == 1 && c[1].q_hi == 2);
  CHECK(r.k.q_marg_off[0] == 0 && r.k.q_card[0] == 2 && r.k.q_marg_off[1] == 2 && r.k.q_card[1] == 3);
  CHECK(c[0].marg0 == 0 && c[1].marg0 == 2 && c[0].mstride == 3 && c[1].mstride == 1);
  CHECK(c[0].nf == 1 && c[1].nf == 2 && c[0].nt == 1 && c[1].nt == 2);
  CHECK(c[0].val_lo == 0 && c[0].val_hi == 6 && c[1].val_lo == 6 && c[1].val_hi == 18);
  CHECK(c[1].fbase[0] == 6 && c[1].fbase[1] == 12 && c[1].fstride[0] == 1 && c[1].fstride[1] == 2);
  // term blocks padded to 4 each: the second component's starts at term 4 (cumulative ev_lo)
  CHECK(c[0].ev_lo == 0 && c[1].ev_lo == 4 && r.k.terms_off == 2 * 96 && r.k.tab_off == 2 * 96 + 9 * 4);
  const RowsTerm *t = terms_of(r);
  CHECK(same_term(t[0], RowsTerm{1, 1, 3, 0}) && same_term(t[1], RowsTerm{1, 0, 256, -1}));
  CHECK(same_term(t[4], RowsTerm{0, 3, 2, 0}) && same_term(t[5], RowsTerm{0, 1, 2, 1}));  // column 0 twice
  CHECK(same_term(t[6], RowsTerm{0, 0, 256, -1}) && same_term(t[7], RowsTerm{0, 0, 256, -1}) && same_term(t[8], kNoop));
  // the affine kernel's folded strides: term j of the component into factor slot k
  CHECK(c[1].a_S[0][0] == 3 && c[1].a_S[0][1] == 0 && c[1].a_S[1][0] == 0 && c[1].a_S[1][1] == 1);
  CHECK(c[1].a_col[0] == 0 && c[1].a_col[1] == 0 && c[1].a_card[0] == 2 && c[1].a_card[1] == 2 && c[1].a_card[2] == 256);
  CHECK(r.cols == std::vector<int>({0, 1}) && r.n_cols == 2 && r.max_nf == 2 && r.max_nt == 2 && r.all_affine);
  // the shared column is loaded once per row in the generated source
  const std::string one_row = r.jit_src.substr(0, r.jit_src.find("pgm_rows_jit2("));
  size_t loads = 0;
  for (size_t at = one_row.find("= cr["); at != std::string::npos; at = one_row.find("= cr[", at + 1)) ++loads;
  CHECK(loads == 2);
  return 0;
}

static int test_table_2x3() {
  const pgm_rows_plan p = plan_table_2x3();
  RowsPlan r;
  CHECK(rows_plan_compile(&p, r) == PGM_OK);
  const RowsComp &c = comps_of(r)[0];
  CHECK(c.simple == 0 && c.P == 6 && c.H == 1 && c.nq == 2 && c.nf == 1 && c.mstride == 0 && c.fstride[0] == 0);
  CHECK(r.any_table && !r.all_affine && r.jit_src.empty());
  CHECK(c.off_base == 0 && c.marg_base == 6 && c.map_base == 18 && r.desc.size() == (size_t)r.k.tab_off + 24 + 1);
  const int32_t off[6] = {0, 1, 2, 6, 7, 8};                            // entry (q0, q1): 6 q0 + q1
  const int32_t marg[12] = {0, 2, 0, 3, 0, 4, 1, 2, 1, 3, 1, 4};        // rows q0 and 2 + q1
  const int32_t map[6] = {0, 1, 2, 3, 4, 5};                            // 3 q0 + q1
  CHECK(memcmp(tab_of(r) + c.off_base, off, sizeof off) == 0);
  CHECK(memcmp(tab_of(r) + c.marg_base, marg, sizeof marg) == 0);
  CHECK(memcmp(tab_of(r) + c.map_base, map, sizeof map) == 0);
  CHECK(tab_of(r)[24] == 0);
  // one query dim x one hidden dim: entries (q, h), two factors per entry
  const pgm_rows_plan ph = plan_table_hidden();
  RowsPlan rh;
  CHECK(rows_plan_compile(&ph, rh) == PGM_OK);
  const RowsComp &ch = comps_of(rh)[0];
  CHECK(ch.simple == 0 && ch.P == 2 && ch.H == 3 && ch.nq == 1 && ch.nf == 2);
  CHECK(ch.off_base == 0 && ch.marg_base == 12 && ch.map_base == 14);
  const int32_t offh[12] = {0, 0, 1, 2, 2, 4, 3, 0, 4, 2, 5, 4};  // [3 q + h, 2 h] per entry
  const int32_t tailh[4] = {0, 1, 0, 1};                          // marginal rows, then MAP digits
  CHECK(memcmp(tab_of(rh), offh, sizeof offh) == 0 && memcmp(tab_of(rh) + 12, tailh, sizeof tailh) == 0);
  return 0;
}

static int test_term_padding() {
  const int nts[6] = {0, 3, 4, 5, 8, 9}, blocks[6] = {0, 4, 4, 8, 8, 9};
  for (int i = 0; i < 6; ++i) {
    const int nt = nts[i], n0 = (nt + 1) / 2;
    const pgm_rows_plan p = plan_terms(nt);
    RowsPlan r;
    CHECK(rows_plan_compile(&p, r) == PGM_OK);
    const RowsComp &c = comps_of(r)[0];
    CHECK(c.nt == nt && r.max_nt == nt && c.ev_lo == 0 && r.all_affine == (nt <= 8));
    CHECK(r.k.tab_off - r.k.terms_off == 4 * (blocks[i] + 1));  // the block + the trailing no-op term
    const RowsTerm *t = terms_of(r);
    for (int j = 0; j < nt; ++j) {
      CHECK(t[j].col == 2 * j && t[j].card == 2 && t[j].slot == (j < n0 ? 0 : 1));
      if (nt <= 8) CHECK(c.a_col[j] == 2 * j && c.a_card[j] == 2 && c.a_S[j][j < n0 ? 0 : 1] == t[j].stride);
    }
    for (int j = nt; j < blocks[i]; ++j) CHECK(same_term(t[j], RowsTerm{0, 0, 256, -1}));
    CHECK(same_term(t[blocks[i]], kNoop) && r.desc[r.k.tab_off] == 0 && r.desc.size() == (size_t)r.k.tab_off + 1);
    for (int j = nt <= 8 ? nt : 0; j < 8; ++j) CHECK(c.a_col[j] == 0 && c.a_card[j] == 256);
    CHECK(r.n_cols == (nt ? 2 * (nt - 1) + 1 : 0) && (int)r.cols.size() == nt);
  }
  return 0;
}

// ---------------------------------------------------------------------------- rejected plans
static int rejected(const pgm_rows_plan &p, const char *msg) {
  RowsPlan r;
  g_last_err.clear();
  const int st = rows_plan_compile(&p, r);
  if (st != PGM_EINVAL || g_last_err != msg) {
    fprintf(stderr, "expected PGM_EINVAL \"%s\"\n     got %d \"%s\"\n", msg, st, g_last_err.c_str());
    return 1;
  }
  return 0;
}

static int test_rejected() {
  pgm_rows_plan p = plan_affine_nq1();
  p.n_loop = 13;
  CHECK(!rejected(p, "rows_plan_create: plan out of range (loop 13 query 1 fac 1 ev 1 comp 1 marg 3)"));
  p = plan_affine_nq1();
  p.fac_ev_end[0] = 2;
  CHECK(!rejected(p, "rows_plan_create: factor 0 evidence range"));
  p = plan_affine_nq1();
  p.n_values = 5;
  CHECK(!rejected(p, "rows_plan_create: factor 0 reads past values"));
  p = plan_two_comp();
  p.fac_ev_begin[2] = 1;  // factor 2 claims factor 1's term too
  p.n_values = 32;
  CHECK(!rejected(p, "rows_plan_create: evidence term 1 feeds two factors"));
  p = plan_two_comp();
  p.comp_loop_begin[1] = 0;
  CHECK(!rejected(p, "rows_plan_create: component 1 ranges (loops [0,1,2) factors [1,3))"));
  p = plan_affine_nq1();
  p.loop_card[0] = 0;
  CHECK(!rejected(p, "rows_plan_create: loop_card[0] <= 0"));
  p = plan_affine_nq1();
  p.loop_marg_off[0] = 1;
  CHECK(!rejected(p, "rows_plan_create: loop 0 marginal rows out of range"));
  p = blank();  // three hidden dims of card 512: 2^27 entries
  for (int k = 0; k < 3; ++k) add_loop(p, 512, -1, 0);
  add_fac(p, 0);
  end_comp(p, 0);
  p.n_values = 1, p.n_joint = 1;
  CHECK(!rejected(p, "rows_plan_create: component 0 index space too large for the fused kernel"));
  p = plan_two_comp();
  p.fac_stride[0][1] = 1;  // (stays inside the values: reaches 7 of 18)
  CHECK(!rejected(p, "rows_plan_create: factor 0 strides a loop dim outside its component"));
  p = blank();  // factors 0, 1 | 2; terms 0 -> factor 0, 1 -> factor 2, 2 -> factor 1
  add_loop(p, 2, 0, 2);
  add_fac(p, 0);
  add_fac(p, 2);
  end_comp(p, 1);
  add_loop(p, 2, 2, 1);
  add_fac(p, 4);
  end_comp(p, 1);
  p.n_ev = 3;
  for (int j = 0; j < 3; ++j) p.ev_col[j] = j, p.ev_stride[j] = 1, p.ev_card[j] = 2;
  p.fac_ev_begin[0] = 0, p.fac_ev_end[0] = 1, p.fac_ev_begin[1] = 2, p.fac_ev_end[1] = 3;
  p.fac_ev_begin[2] = 1, p.fac_ev_end[2] = 2;
  p.n_values = 6, p.n_marg = 4, p.n_joint = 4;
  CHECK(!rejected(p, "rows_plan_create: component 0 evidence terms are not contiguous"));
  p = plan_affine_nq1();
  p.n_loop = 2;  // a loop dim no component covers
  p.loop_card[1] = 1;
  CHECK(!rejected(p, "rows_plan_create: components do not cover the loop dims / factors"));
  // pgm_rows_plan_source's own checks
  std::string src;
  g_last_err.clear();
  CHECK(rows_plan_source(nullptr, src) == PGM_EINVAL && g_last_err == "rows_plan_source: null plan");
  p = plan_affine_nq1();
  p.n_comp = 0;
  CHECK(rows_plan_source(&p, src) == PGM_EINVAL && g_last_err == "rows_plan_source: plan out of range");
  p = plan_table_2x3();
  CHECK(rows_plan_source(&p, src) == PGM_EINVAL &&
        g_last_err == "rows_plan_source: component 0 is not specialisable (query dims 2, loop dims 2)");
  p = plan_table_hidden();
  CHECK(rows_plan_source(&p, src) == PGM_EINVAL &&
        g_last_err == "rows_plan_source: component 0 is not specialisable (query dims 1, loop dims 2)");
  CHECK(src.empty());
  return 0;
}

// ---------------------------------------------------------------------------- launch predicates
static int test_rows2_aligned() {
  const int32_t M = PGM_ROWS_MARGINALS, P = PGM_ROWS_MAP, G = PGM_ROWS_MAPGAP;
  // addresses are only inspected, never dereferenced
  const uint8_t *codes = (const uint8_t *)0x10000;
  const double *marg = (const double *)0x20000, *gap = (const double *)0x30000;
  const int32_t *map = (const int32_t *)0x40000;
  const int32_t all = M | P | G;
  CHECK(rows2_aligned(all, codes, 1000, 0, 1000, marg, 1000, map, gap, 17));
  CHECK(!rows2_aligned(all, codes, 1000, 0, 999, marg, 1000, map, gap, 17));   // odd n_rows
  CHECK(!rows2_aligned(all, codes, 1001, 0, 1000, marg, 1002, map, gap, 17));  // odd ld_codes
  CHECK(!rows2_aligned(all, codes, 1000, 1, 1000, marg, 1000, map, gap, 17));  // odd row0
  CHECK(rows2_aligned(all, codes, 1000, 2, 1000, marg, 1000, map, gap, 17));
  CHECK(!rows2_aligned(all, codes + 1, 1000, 0, 1000, marg, 1000, map, gap, 17));  // odd code pointer
  CHECK(rows2_aligned(all, codes + 2, 1000, 0, 1000, marg, 1000, map, gap, 17));
  CHECK(!rows2_aligned(all, codes, 1000, 0, 1000, marg + 1, 1000, map, gap, 17));  // marg at 8 mod 16
  CHECK(rows2_aligned(P | G, codes, 1000, 0, 1000, marg + 1, 1000, map, gap, 17));  // ... unread without marginals
  CHECK(!rows2_aligned(all, codes, 1000, 0, 1000, marg, 1001, map, gap, 17));      // odd ld_out
  CHECK(!rows2_aligned(all, codes, 1000, 0, 1000, marg, 1000, map + 1, gap, 17));  // map at 4 mod 8
  CHECK(rows2_aligned(all, codes, 1000, 0, 1000, marg, 1000, map + 2, gap, 17));
  CHECK(rows2_aligned(M, codes, 1000, 0, 1000, marg, 1000, nullptr, nullptr, 17));
  CHECK(!rows2_aligned(all, codes, 1000, 0, 1000, marg, 1000, map, gap + 1, 17));  // gap at 8 mod 16
  CHECK(rows2_aligned(M | P, codes, 1000, 0, 1000, marg, 1000, map, gap + 1, 17));  // ... unread without MAPGAP
  // (n_marg + 1) * ld_out * 8 one below and exactly at 2^31: (3 + 1) * ld_out * 8, ld_out = 2^26 (- 2: even)
  const int64_t ld26 = (int64_t)1 << 26;
  CHECK(rows2_aligned(M, codes, 1000, 0, 1000, marg, ld26 - 2, nullptr, nullptr, 3));
  CHECK(!rows2_aligned(M, codes, 1000, 0, 1000, marg, ld26, nullptr, nullptr, 3));
  CHECK(rows2_aligned(P, codes, 1000, 0, 1000, marg, ld26, map, nullptr, 3));  // the limit is the marginals'
  // n_rows * 8 one (even) step below and exactly at 2^31
  const int64_t n28 = (int64_t)1 << 28;
  CHECK(rows2_aligned(P, codes, n28, 0, n28 - 2, nullptr, 0, map, nullptr, 3));
  CHECK(!rows2_aligned(P, codes, n28, 0, n28, nullptr, 0, map, nullptr, 3));
  // rows_jit2_ok: the same contract from 50,000 rows up
  CHECK(!rows_jit2_ok(all, codes, 50000, 0, 49998, marg, 50000, map, gap, 17));
  CHECK(rows_jit2_ok(all, codes, 50000, 0, 50000, marg, 50000, map, gap, 17));
  CHECK(!rows_jit2_ok(all, codes + 1, 50000, 0, 50000, marg, 50000, map, gap, 17));
  return 0;
}

// ---------------------------------------------------------------------------- launch choice
// rows_launch_info (what pgm_rows_launch_info returns and rows_plan_run launches) at its boundaries
static int test_launch_info() {
  const int32_t M = PGM_ROWS_MARGINALS, P = PGM_ROWS_MAP, G = PGM_ROWS_MAPGAP, all = M | P | G;
  const uint8_t *codes = (const uint8_t *)0x10000;
  const double *marg = (const double *)0x20000, *gap = (const double *)0x30000, *joint = (const double *)0x50000;
  const int32_t *map = (const int32_t *)0x40000;
  pgm_rows_launch_info_t li;
  auto info = [&](const pgm_rows_plan &p, int32_t mode, int64_t n, bool jit) {
    return rows_launch_info(&p, mode, codes, n, 0, n, marg, joint, n, map, gap, jit, &li);
  };
  // values in LDS up to 5,120 doubles with the trailing 1.0 (40 KiB), ahead-of-time kernels
  pgm_rows_plan p = plan_affine_nq1();
  p.n_values = 5119;
  CHECK(info(p, all, 197, false) == PGM_OK);
  CHECK(li.kernel == PGM_RK_AFFINE && li.values_lds == 1 && li.nf == 1 && li.nt == 4 && li.map == 1 && li.rg == 1);
  CHECK(li.blocks == 4 && li.wg == 64 && li.lds_bytes == 5120 * 8);  // one component: no exchange slots
  p.n_values = 5120;
  CHECK(info(p, all, 197, false) == PGM_OK);
  CHECK(li.kernel == PGM_RK_AFFINE && li.values_lds == 0 && li.lds_bytes == 0);
  CHECK(info(p, all | PGM_ROWS_GENERIC, 197, false) == PGM_OK);
  CHECK(li.kernel == PGM_RK_TABLE && li.values_lds == 0 && li.acc_lds == 0 && li.maxfc == 2 && li.maxt == 4);
  CHECK(li.lds_bytes == 64 * 20);
  // the specialised kernels stage up to 6,144 doubles (48 KiB)
  p.n_values = 6143;
  CHECK(info(p, all, 197, true) == PGM_OK);
  CHECK(li.kernel == PGM_RK_JIT && li.values_lds == 1 && li.wg == (uint32_t)jit_wg() && li.rg == 1);
  CHECK(li.blocks == (197 + li.wg - 1) / li.wg && li.lds_bytes == (6144 + li.wg - 1) / li.wg * li.wg * 8);
  p.n_values = 6144;
  CHECK(info(p, all, 197, true) == PGM_OK);
  CHECK(li.kernel == PGM_RK_JIT && li.values_lds == 0 && li.lds_bytes == 0);
  // every mode bit that rules the specialised kernel out; a plan without a generated source
  p = plan_affine_nq1();
  for (int32_t bit : {PGM_ROWS_GENERIC, PGM_ROWS_NO_JIT, PGM_ROWS_VALUES_GLOBAL, PGM_ROWS_ONE_GROUP}) {
    CHECK(info(p, all | bit, 197, true) == PGM_OK);
    CHECK(li.kernel == (bit == PGM_ROWS_GENERIC ? PGM_RK_TABLE : PGM_RK_AFFINE));
  }
  CHECK(info(p, M | PGM_ROWS_JOINT, 197, true) == PGM_OK);
  CHECK(li.kernel == PGM_RK_TABLE && li.acc_lds == 0);  // no table component: no accumulators
  CHECK(info(p, M, 197, false) == PGM_OK);
  CHECK(li.kernel == PGM_RK_AFFINE && li.map == 0);
  // two rows per thread from 50,000 rows
  CHECK(info(p, all, 49999, true) == PGM_OK && li.kernel == PGM_RK_JIT);
  CHECK(info(p, all, 49998, true) == PGM_OK && li.kernel == PGM_RK_JIT);
  CHECK(info(p, all, 50000, true) == PGM_OK && li.kernel == PGM_RK_JIT2);
  CHECK(li.blocks == (50000 + 2 * li.wg - 1) / (2 * li.wg));
  CHECK(rows_launch_info(&p, all, codes, 50000, 0, 50000, marg + 1, joint, 50000, map, gap, true, &li) == PGM_OK);
  CHECK(li.kernel == PGM_RK_JIT);
  // row groups per workgroup: groups / 4096, from 8,192 groups (524,225 rows) up, at most 8
  CHECK(info(p, all, 524224, false) == PGM_OK && li.rg == 1 && li.blocks == 8191);
  CHECK(info(p, all, 524225, false) == PGM_OK && li.rg == 2 && li.blocks == 4096);
  CHECK(info(p, all | PGM_ROWS_ONE_GROUP, 524225, false) == PGM_OK && li.rg == 1 && li.blocks == 8192);
  CHECK(info(p, all | PGM_ROWS_VALUES_GLOBAL, 524225, false) == PGM_OK && li.rg == 1);
  CHECK(info(p, all | PGM_ROWS_GENERIC, 524225, false) == PGM_OK && li.kernel == PGM_RK_TABLE && li.rg == 2);
  CHECK(info(p, all, 64ll * 4096 * 9, false) == PGM_OK && li.rg == 8 && li.blocks == 4096 * 9 / 8);
  // marginal accumulators in LDS while values + exchange slots + 512 B per marginal row fit 64 KiB
  p = plan_table_hidden();  // 12 values: 112 B; one component: 1,280 B of exchange slots
  p.n_marg = 125;
  CHECK(info(p, all, 197, true) == PGM_OK);
  CHECK(li.kernel == PGM_RK_TABLE && li.acc_lds == 1 && li.lds_bytes == 112 + 1280 + 125 * 512);
  p.n_marg = 126;
  CHECK(info(p, all, 197, true) == PGM_OK);
  CHECK(li.kernel == PGM_RK_TABLE && li.acc_lds == 0 && li.values_lds == 1 && li.lds_bytes == 112 + 1280);
  p.n_marg = 125;
  CHECK(info(p, P | G, 197, true) == PGM_OK && li.acc_lds == 0);  // no marginals: no accumulators
  // template arguments from the plan's widest component
  p = plan_terms9();
  CHECK(info(p, all, 197, false) == PGM_OK && li.kernel == PGM_RK_TABLE && li.maxfc == 2 && li.maxt == PGM_ROWS_MAX_EV);
  p = plan_terms8();
  CHECK(info(p, all, 197, false) == PGM_OK && li.kernel == PGM_RK_AFFINE && li.nf == 2 && li.nt == 8);
  p = plan_terms4();
  CHECK(info(p, all, 197, false) == PGM_OK && li.kernel == PGM_RK_AFFINE && li.nf == 2 && li.nt == 4);
  // a component without factors: all-affine, one slot
  p = plan_no_factor();
  CHECK(info(p, all, 197, false) == PGM_OK);
  CHECK(li.kernel == PGM_RK_AFFINE && li.values_lds == 1 && li.nf == 1 && li.wg == 128);
  CHECK(info(p, all, 197, true) == PGM_OK && li.kernel == PGM_RK_JIT);
  // the argument checks of pgm_rows_plan_run, in its order; nothing to launch
  p = plan_two_comp();
  CHECK(rows_launch_info(&p, all, nullptr, 10, 0, 10, nullptr, joint, 10, map, gap, true, &li) == PGM_EINVAL);
  CHECK(g_last_err == "rows_plan_run: null codes");
  CHECK(rows_launch_info(&p, all, codes, 10, 0, 10, nullptr, joint, 5, nullptr, gap, true, &li) == PGM_EINVAL);
  CHECK(g_last_err == "rows_plan_run: marginals requested, marg is null");
  CHECK(rows_launch_info(&p, PGM_ROWS_JOINT, codes, 10, 0, 10, marg, joint, 10, map, gap, true, &li) == PGM_EINVAL);
  CHECK(g_last_err == "rows_plan_run: joint output needs a single-component plan");
  CHECK(rows_launch_info(&p, all, codes, 10, 0, 10, marg, joint, 5, map, gap, true, &li) == PGM_EINVAL);
  CHECK(g_last_err == "rows_plan_run: ld_out 5 < n_rows 10");
  CHECK(info(p, all, 0, true) == PGM_OK && li.kernel == PGM_RK_NONE && li.blocks == 0);
  CHECK(rows_launch_info(nullptr, all, codes, 10, 0, 10, marg, joint, 10, map, gap, true, &li) == PGM_EINVAL);
  return 0;
}

// ---------------------------------------------------------------------------- source shape
static int test_source_shape() {
  // LDS staging up to 6,144 values (48 KiB), global gathers above
  pgm_rows_plan p = plan_big_values();
  RowsPlan r;
  CHECK(rows_plan_compile(&p, r) == PGM_OK);
  CHECK(r.jit_src.find("#define VAL(i) V[i]\n") != std::string::npos);
  const std::string one_row = r.jit_src.substr(0, r.jit_src.find("pgm_rows_jit2("));
  CHECK(one_row.find("__shared__") == std::string::npos);
  p = plan_affine_nq1();
  CHECK(rows_plan_compile(&p, r) == PGM_OK);
  CHECK(r.jit_src.find("#define VAL(i) S[i]\n") != std::string::npos);
  // a component without factors multiplies nothing
  p = plan_no_factor();
  CHECK(rows_plan_compile(&p, r) == PGM_OK);
  CHECK(r.jit_src.find("const double p1_0_0 = 1.0;\n") != std::string::npos);
  const RowsComp &c = comps_of(r)[1];
  CHECK(c.nf == 0 && c.val_lo == 0 && c.val_hi == 0 && c.fbase[0] == 2 && r.max_nf == 1);
  // the five kernels of a source, the workgroup sizes the launchers use
  for (const char *name : {"pgm_rows_jit(", "pgm_rows_jit2(", "pgm_rows_floor(", "pgm_rows_floor2(", "pgm_rows_ring("})
    CHECK(r.jit_src.find(name) != std::string::npos);
  char bound[64];
  snprintf(bound, sizeof bound, "__launch_bounds__(%d) pgm_rows_jit(", jit_wg());
  CHECK(r.jit_src.find(bound) != std::string::npos);
  snprintf(bound, sizeof bound, "__launch_bounds__(%d) pgm_rows_ring(", ring_wg());
  CHECK(r.jit_src.find(bound) != std::string::npos);
  return 0;
}

// ---------------------------------------------------------------------------- cache policy of the stream
// policy word as PGM_ROWS_STREAM reads it: bit 0 nontemporal code loads, bits 1-2 the store form
static RowsPolicy policy_of(int w) {
  RowsPolicy pol;
  pol.nt_loads = (w & 1) != 0;
  pol.stores = (w >> 1) & 3;
  return pol;
}

static size_t count_of(const std::string &s, const char *what) {
  size_t n = 0;
  for (size_t at = s.find(what); at != std::string::npos; at = s.find(what, at + 1)) ++n;
  return n;
}

static void replace_all(std::string &s, const std::string &from, const std::string &to) {
  for (size_t at = s.find(from); at != std::string::npos; at = s.find(from, at + to.size())) s.replace(at, from.size(), to);
}

// `--source CASE WORD`: the source of a case under a policy word, for the compile test
static int print_source(const char *name, int word) {
  for (size_t i = 0; i < kNumCases; ++i) {
    if (strcmp(kCases[i].name, name)) continue;
    const pgm_rows_plan p = kCases[i].make();
    std::string src;
    if (word < 0 || word > 5 || rows_plan_source(&p, src, policy_of(word)) != PGM_OK) return 1;
    fwrite(src.data(), 1, src.size(), stdout);
    return 0;
  }
  return 1;
}

static int test_stream_policy() {
  CHECK(RowsPolicy().is_default() && policy_of(0).is_default() && !policy_of(1).is_default() && !policy_of(2).is_default());
  for (size_t i = 0; i < kNumCases; ++i) {
    const pgm_rows_plan p = kCases[i].make();
    RowsPlan r;
    CHECK(rows_plan_compile(&p, r) == PGM_OK);
    if (r.any_table) continue;
    std::string def;
    CHECK(rows_plan_source(&p, def, policy_of(0)) == PGM_OK && def == r.jit_src);  // the default policy: today's bytes
    const size_t body0 = def.find("extern \"C\"");
    CHECK(body0 != std::string::npos);
    const size_t n_plain1 = count_of(def, " = cr[") + count_of(def, " += cr[");
    const size_t n_plain2 = count_of(def, " = *(const unsigned short *)(cr + ") + count_of(def, " += *(const unsigned short *)(cr + ");
    const size_t n_coherent = count_of(def, "__hip_atomic_load((__attribute__((address_space(1))) unsigned short *)(cr + ");
    CHECK(n_plain1 == n_plain2 && n_plain1 == 2 * n_coherent);  // jit + floor, jit2 + floor2, ring
    for (int w = 1; w <= 5; ++w) {
      const RowsPolicy pol = policy_of(w);
      std::string src;
      CHECK(rows_plan_source(&p, src, pol) == PGM_OK);
      CHECK((src != def) == (pol.stores != RowsPolicy::kStoreSc1 || n_plain1 > 0));  // a plan may read no evidence
      const size_t body = src.find("extern \"C\"");
      CHECK(body != std::string::npos);
      // loads: every plain code load and no other carries the hint; the ring's and the CPT's are untouched
      CHECK(count_of(src, "__builtin_nontemporal_load(") == (pol.nt_loads ? n_plain1 + n_plain2 : 0));
      CHECK(count_of(src, "__hip_atomic_load((__attribute__((address_space(1))) unsigned short *)(cr + ") == n_coherent);
      CHECK(count_of(src, "V[") == count_of(def, "V["));
      // stores: the macros alone change
      const std::string pre = src.substr(0, body);
      CHECK(count_of(pre, "#define PGM_WT") == 3);
      if (pol.stores == RowsPolicy::kStoreSc1) {
        CHECK(pre == def.substr(0, body0));
      } else {
        const bool sc0 = pol.stores == RowsPolicy::kStoreSc0Sc1Nt;
        CHECK(count_of(pre, sc0 ? "off sc0 sc1 nt\"" : "off sc1 nt\"") == 2 && count_of(pre, "__hip_atomic_store") == 0);
        CHECK(count_of(pre, sc0 ? ", 0, 19); }" : ", 0, 18); }") == 1);
        CHECK(count_of(pre, "global_store_dword %0") == 1 && count_of(pre, "global_store_dwordx2 %0") == 1);
      }
      // the bodies are the default's once the hint is taken off
      std::string b = src.substr(body);
      replace_all(b, "__builtin_nontemporal_load(&cr[", "cr[");
      replace_all(b, "__builtin_nontemporal_load((const unsigned short *)(cr + ", "*(const unsigned short *)(cr + ");
      if (pol.nt_loads) {
        replace_all(b, " * ldc]);\n", " * ldc];\n");
        replace_all(b, " * ldc));\n", " * ldc);\n");
      }
      CHECK(b == def.substr(body0));
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--print")) return print_cases();
  if (argc > 3 && !strcmp(argv[1], "--source")) return print_source(argv[2], atoi(argv[3]));
  CHECK(sha256("abc", 3) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
  CHECK(sha256("abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", 56) ==
        "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1");  // two blocks
  if (test_recorded() || test_affine_nq1() || test_nq0() || test_two_comp() || test_table_2x3() ||
      test_term_padding() || test_rejected() || test_rows2_aligned() || test_launch_info() || test_source_shape() ||
      test_stream_policy())
    return 1;
  printf("rows_plan_selftest ok\n");
  return 0;
}

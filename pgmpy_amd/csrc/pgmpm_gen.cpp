// pgmpm_gen.cpp — the host-only half of the plan-specialised batched-BP steps: the planner of the fused
// product + marginal step (pgmi_plan_product_marg; the generic kernels of pgmhip.hip run the same plan), the
// choice of a step's specialisation, and the generators of the specialised sources — the fused steps, the
// two-marginal pass, several steps merged per dependency level into one kernel, and the specialised
// contraction batches (C1 / C2).  Plain structs in, a source string plus launch geometry out (pgm_pm.h); no
// HIP: pgmpm.cpp compiles, loads and launches what this unit writes.  CPU self-test:
// tools/pm_gen_selftest.cpp, which pins every emission branch's source (tests/golden/pm_source.json).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "pgm_internal.h"
#include "pgm_pm.h"
#include "pgmhip.h"

// ----------------------------------------------------------------------------- shared emitters
// an offset variable of a generated kernel and its stride per dim of the index being decoded
struct Off {
  std::string name;
  const int64_t *stride;
};

// Peel the digits of the dims `order` (fastest first) off the index variable `var` with literal divisors
// card(q), one line per dim, adding digit x stride to every offset whose stride along that dim is not 0.
// Temporaries are q<sfx> / g<sfx>.  whole_last: the last dim's digit is what is left of `var` (no division).
// row_dim: the dim whose digit is also kept in `row` (-1: none).
template <class Card>
static void emit_digits(std::string &o, const char *ind, const char *var, const char *sfx, const std::vector<int> &order,
                        bool whole_last, Card card, const std::vector<Off> &offs, int row_dim = -1) {
  for (size_t n = 0; n < order.size(); ++n) {
    const int q = order[n];
    const unsigned d = card(q);
    if (whole_last && n + 1 == order.size())
      pgmi_appendf(o, "%s{ const unsigned g%s = %s;", ind, sfx, var);
    else
      pgmi_appendf(o, "%s{ const unsigned q%s = %s / %uu, g%s = %s - q%s * %uu; %s = q%s;", ind, sfx, var, d, sfx, var, sfx, d,
                   var, sfx);
    for (const Off &f : offs)
      if (f.stride[q]) pgmi_appendf(o, " %s += (long long)g%s * %lldLL;", f.name.c_str(), sfx, (long long)f.stride[q]);
    if (q == row_dim) pgmi_appendf(o, " row = g%s;", sfx);
    o += " }\n";
  }
}

// dims hi-1 .. lo in that order
static std::vector<int> descending(int hi, int lo = 0) {
  std::vector<int> v;
  for (int i = hi - 1; i >= lo; --i) v.push_back(i);
  return v;
}

// Which of the nested loops [lo, hi) (hi - 1 innermost, trip counts trip(r)) unroll: the innermost ones while
// their trip product — times `inner`, the trips of what they enclose — stays <= limit.  Returns the first
// unrolled loop (hi: none).
template <class Trip>
static int first_unrolled(int lo, int hi, uint64_t inner, uint64_t limit, Trip trip) {
  int first = hi;
  for (int r = hi - 1; r >= lo; --r) {
    inner *= trip(r);
    if (inner > limit) break;
    first = r;
  }
  return first;
}

// Items [lo, hi) of a kernel by block index b: a balanced tree of literal comparisons with first(i), the
// first block of item i (the items' block ranges ascend) — log2 of the items instead of up to one compare
// per item; leaf(i, ind) emits item i's line.
static void block_tree(std::string &o, size_t lo, size_t hi, const std::string &ind,
                       const std::function<unsigned long long(size_t)> &first,
                       const std::function<void(size_t, const std::string &)> &leaf) {
  if (hi - lo == 1) return leaf(lo, ind);
  const size_t mid = (lo + hi) / 2;
  pgmi_appendf(o, "%sif (b < %lluu) {\n", ind.c_str(), first(mid));
  block_tree(o, lo, mid, ind + "  ", first, leaf);
  o += ind + "} else {\n";
  block_tree(o, mid, hi, ind + "  ", first, leaf);
  o += ind + "}\n";
}

// ----------------------------------------------------------------------------- the fused step's plan
// 1 = the fused kernel applies (k filled; grid: the generic kernel's), 0 = it does not (use product_n +
// contract), < 0 error
int pgmi_plan_product_marg(const pgm_productn_desc *d, const double *const *ops, const double *C,
                           const int64_t *marg_s, const double *M, ProdMK &k, uint32_t grid[3]) {
  if (!d || !ops || !marg_s || !M) return pgmi_failf(PGM_EINVAL, "product_n_marginal: null argument");
  if (d->n_ops < 1 || d->n_ops > PMAX || d->n_keep < 1 || d->n_keep > PGM_MAX_DIMS)
    return pgmi_failf(PGM_EINVAL, "product_n_marginal: n_ops %d / n_keep %d out of range", d->n_ops, d->n_keep);
  if (d->n_ops > MOPS || d->n_keep < 2) return 0;
  memset(&k, 0, sizeof k);
  const int last = d->n_keep - 1;
  const int64_t NX = d->keep_card[last];
  if (NX < 64 || NX % 2 || d->keep_sc[last] != 1 || marg_s[last] != 1) return 0;
  if (((uintptr_t)C & 15) || ((uintptr_t)M & 15)) return 0;
  k.n_ops = d->n_ops;
  k.mdiv = -1;
  for (int t = 0; t < MOPS; ++t) {
    const bool real = t < d->n_ops;
    k.ops[t] = real ? ops[t] : ops[0];
    k.kind[t] = real ? d->op_kind[t] : PGM_PRODN_MUL;
    if (real && (!ops[t] || d->op_kind[t] < 0 || d->op_kind[t] > PGM_PRODN_MDIV))
      return pgmi_failf(PGM_EINVAL, "product_n_marginal: operand %d", t);
    if (real && d->op_kind[t] == PGM_PRODN_MDIV) {  // a factor of the product, and the marginal's divisor
      if (k.mdiv >= 0) return pgmi_failf(PGM_EINVAL, "product_n_marginal: more than one PGM_PRODN_MDIV operand");
      k.mdiv = t;
      k.kind[t] = PGM_PRODN_MUL;
    }
    const int64_t sx = real ? d->keep_s[t][last] : 0;
    if (sx != 0 && sx != 1) return 0;
    if (sx == 1 && ((uintptr_t)ops[t] & 15)) return 0;
    k.vec[t] = sx == 1;
  }
  uint64_t n_outer = 1, n_red = 1;
  for (int i = 0; i < last; ++i) {
    const int64_t c = d->keep_card[i];
    if (c <= 0) return pgmi_failf(PGM_EINVAL, "product_n_marginal: keep_card[%d] <= 0", i);
    if (c == 1) continue;
    const bool kept = marg_s[i] != 0;
    if (d->keep_sc[i] % 2 || (kept && marg_s[i] % 2)) return 0;
    for (int t = 0; t < d->n_ops; ++t)
      if (k.vec[t] && d->keep_s[t][i] % 2) return 0;
    if (kept) {
      if (k.nk >= KMAX - 1) return 0;
      k.kdiv[k.nk] = make_fdiv((uint32_t)c);
      k.ksc[k.nk] = d->keep_sc[i];
      k.ksm[k.nk] = marg_s[i];
      for (int t = 0; t < d->n_ops; ++t) k.ks[t][k.nk] = d->keep_s[t][i];
      ++k.nk;
      n_outer *= (uint64_t)c;
    } else {
      if (k.nr >= KMAX) return 0;
      k.rdiv[k.nr] = make_fdiv((uint32_t)c);
      k.rsc[k.nr] = d->keep_sc[i];
      for (int t = 0; t < d->n_ops; ++t) k.rs[t][k.nr] = d->keep_s[t][i];
      ++k.nr;
      n_red *= (uint64_t)c;
    }
  }
  if (n_red > RMAX_MARG || n_outer >= (1ull << 31)) return 0;
  // kept-dim order of the block schedule: blocks are dispatched with the LAST kept dim fastest.  A
  // row-dim operand that lacks a kept dim is read again by every block along that dim, so the dims
  // lacked by the largest such operands go innermost: the blocks sharing an operand slice then run
  // back to back and find it in L2 (pathfinder's root: 129-258 MB separator aggregates broadcast over
  // its other variables).
  if (k.nk > 1) {
    double score[KMAX];
    for (int i = 0; i < k.nk; ++i) {
      score[i] = 0.0;
      for (int t = 0; t < d->n_ops; ++t) {
        if (!k.vec[t] || k.ks[t][i] != 0) continue;
        double size = 1.0;  // the operand's elements per row
        for (int q = 0; q < k.nk; ++q)
          if (k.ks[t][q] != 0) size *= (double)k.kdiv[q].d;
        for (int r = 0; r < k.nr; ++r)
          if (k.rs[t][r] != 0) size *= (double)k.rdiv[r].d;
        score[i] += size;
      }
    }
    int ord[KMAX];
    for (int i = 0; i < k.nk; ++i) ord[i] = i;
    std::stable_sort(ord, ord + k.nk, [&](int a, int b) { return score[a] < score[b]; });
    ProdMK k2 = k;
    for (int i = 0; i < k.nk; ++i) {
      const int o = ord[i];
      k2.kdiv[i] = k.kdiv[o];
      k2.ksc[i] = k.ksc[o];
      k2.ksm[i] = k.ksm[o];
      for (int t = 0; t < MOPS; ++t) k2.ks[t][i] = k.ks[t][o];
    }
    k = k2;
  }
  for (int t = 0; t < MOPS; ++t) {
    k.jvar[t] = 0;
    for (int r = 0; t < d->n_ops && r < k.nr; ++r) k.jvar[t] |= k.rs[t][r] != 0;
  }
  if (k.mdiv >= 0 && k.jvar[k.mdiv]) return 0;  // the divisor varies over the summed entries: not this kernel
  k.kdiv[k.nk] = make_fdiv((uint32_t)NX);  // the row dim, last
  ++k.nk;
  k.n_red = (int32_t)n_red;
  k.n_outer = (uint32_t)n_outer;
  k.NP = (uint32_t)(NX / 2);
  const uint64_t xb = (k.NP + 255) / 256;
  const uint64_t gy = std::min<uint64_t>(n_outer, 65535);
  // target block count
  static constexpr uint64_t target = 2048;
  const uint64_t gx = std::min<uint64_t>(xb, std::max<uint64_t>(1, target / gy));
  // too few blocks to fill the chip: the two-kernel path (product_n + contract) was faster for a lone
  // launch below 512 blocks, but inside a levelled schedule it costs a second dependency level.  C4
  // (r03ae, two runs each): floor 512 / 256 / 128 / 64 -> 0.87-0.88 / 0.92 / 0.95 / 0.85 M
  // calibrations/s at 1,000 rows, 1.20-1.21 / 1.25 / 1.24-1.25 / 1.24-1.25 M at 4,000.  Once small steps are specialised and merged into their level's launch
  // (PGM_PM_JIT_MIN 2^14, r03ag) a small fused pass costs no launch of its own: floor 128 -> 32 gives
  // 1.03 -> 1.09 M at 1,000 rows, 4,000 rows unchanged at 1.29-1.30 M (r03ah); 32 / 8 / 2 -> 1.08 / 1.08
  // / 1.09-1.10 M (r03ai): no floor by default.
  static constexpr uint64_t min_blocks = 1;
  // (also accepting short reductions on 16+ blocks was slower at 1,000 rows, 0.95 -> 0.87 M: each such
  // pass is a launch of its own, where the two-kernel path's jobs join the level's batch launch; r03af)
  if (gx * gy < min_blocks) return 0;
  grid[0] = (uint32_t)gx, grid[1] = (uint32_t)gy, grid[2] = 1;
  return 1;
}


// ----------------------------------------------------------------------------- specialised product+marginal
// The fused batched-BP step (k_productn_marg_jx) with its plan baked in as literals: outer digits
// decoded with constant divisors, the reduced entries walked as nested loops with literal bounds and
// strides (inner ones unrolled, so several entries' operand loads are in flight together), operands
// that lack the row axis read at wave-uniform addresses (scalar loads), one 1-D grid with an optional
// XCD-grouped block order.  Compiled once per shape (hipRTC, cached by source), bound to its
// pointers, launched by pgm_pm_bound_run (capturable in a HIP graph).

// Decode order of a step's kept outer dims, fastest first (the last one is the slowest: with the XCD
// grouping each XCD takes a contiguous range of it).  The kept dim carried by the most row-operand bytes
// becomes the slowest, so each XCD reads a disjoint slice of every operand that carries it (instead of
// all 8 re-reading an operand that lacks the belief's slowest dim), and the other dims vary fastest in
// order of the bytes that carry them (least first), so consecutive blocks re-read the same operand
// entries while they are in the XCD's L2 (C4 pathfinder, 4,000 rows: fetch 7.75 -> 6.32 GB per sweep,
// 1.04x the steps' own reads; r03's belief order and r04's partition-only and reversed forms measured
// slower, profiles/r04c/).  cards[q], bytes_of(q) = row-operand bytes that vary along kept dim q.
template <class BytesOf>
static std::vector<int> pm_kept_order(int kx, const unsigned *cards, BytesOf bytes_of) {
  std::vector<int> ord;
  for (int qi = 0; qi < kx; ++qi) ord.push_back(kx - 1 - qi);
  if (kx < 2) return ord;
  int p = -1;
  double best = -1.0;
  for (int q = 0; q < kx; ++q) {
    if (cards[q] < 2) continue;
    const double b = bytes_of(q);
    if (b > best || (b == best && p >= 0 && cards[q] > cards[p])) best = b, p = q;
  }
  if (p < 0) return ord;
  ord.erase(std::find(ord.begin(), ord.end(), p));
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return bytes_of(a) < bytes_of(b); });
  ord.push_back(p);
  return ord;
}

// blocks that share an XCD (b % 8, the dispatcher's round robin) take consecutive tiles: XCD label x
// gets tiles [x q + min(x, r), ...) with q = total / 8, r = total % 8 — a bijection for any total
// (the plain (b % 8) q + b / 8 only when 8 divides total)
static std::string pm_xcd_remap(uint64_t total) {
  const unsigned long long q = total / 8, r = total % 8;
  std::string o;
  if (r == 0)
    pgmi_appendf(o, "  b = (b %% 8u) * %lluu + b / 8u;  // blocks of one XCD are consecutive tiles\n", q);
  else
    pgmi_appendf(o, "  { const unsigned x = b %% 8u, y = b / 8u; b = (x < %lluu ? x * %lluu : %lluu + (x - %lluu) * %lluu) + y; }"
                    "  // blocks of one XCD are consecutive tiles\n", r, q + 1, r * (q + 1), r, q);
  return o;
}

// a body's signature: its block index, its n operands, then the product (C) and marginal (M) outputs
static std::string pm_signature(const std::string &name, int n) {
  std::string o = "__device__ __forceinline__ void " + name + "(unsigned b";
  for (int i = 0; i < n; ++i) o += ", const double *__restrict__ o" + std::to_string(i);
  o += ", double *__restrict__ C, double *__restrict__ M) {\n  (void)C; (void)M;\n";
  return o;
}

// operand pointers a body takes (its kernel arguments are these, then C and M)
int pm_nops(const PMSpec &sp) { return sp.multi ? sp.mm.n_ops : sp.k.n_ops; }

// body `name` of one step: a device function of its block index within the step
static std::string pm_body(const PMSpec &sp, const std::string &name) {
  const ProdMK &k = sp.k;
  const int red = sp.red, XI = sp.XI, unroll = sp.unroll;
  const bool store = sp.store, xcd = sp.xcd, nt = sp.nt, has_m = sp.has_m;
  const unsigned gx = sp.gx;
  const uint64_t total = sp.total;
  const int td = sp.tdim;
  const unsigned T = td >= 0 ? sp.T : 1;
  auto tsfx = [&](unsigned t) { return T > 1 ? "t" + std::to_string(t) : std::string(); };
  auto tiled = [&](int i) { return td >= 0 && k.ks[i][td] != 0; };  // operand i varies along the tile dim
  std::string o;
  o += pm_signature(name, k.n_ops);
  if (xcd) o += pm_xcd_remap(total);
  pgmi_appendf(o, "  const unsigned xb = b %% %uu, ob = b / %uu;\n", gx, gx);
  o += "  unsigned idx = ob;\n  long long oc = 0, om = 0";
  for (int i = 0; i < k.n_ops; ++i) pgmi_appendf(o, ", f%d = 0", i);
  o += ";\n  (void)oc; (void)idx;\n";
  const int kx = k.nk - 1;  // kept outer dims 0..kx-1 (kx-1 fastest), the row dim last
  unsigned kc[KMAX] = {};
  for (int q = 0; q < kx; ++q) kc[q] = k.kdiv[q].d;
  auto op_bytes = [&](int i) {  // entries of operand i over the step's index space (rows included)
    double b = k.vec[i] ? 16.0 * k.NP : 8.0;
    for (int q = 0; q < kx; ++q)
      if (k.ks[i][q]) b *= kc[q];
    for (int r = 0; r < k.nr; ++r)
      if (k.rs[i][r]) b *= k.rdiv[r].d;
    return b;
  };
  std::vector<int> kord = pm_kept_order(kx, kc, [&](int q) {
    double t = 0.0;
    for (int i = 0; i < k.n_ops; ++i)
      if (k.vec[i] && k.ks[i][q]) t += op_bytes(i);
    return t;
  });
  kord.erase(std::remove(kord.begin(), kord.end(), td), kord.end());  // the tile dim is walked inside the block
  std::vector<Off> offs = {{"oc", k.ksc}, {"om", k.ksm}};
  for (int i = 0; i < k.n_ops; ++i) offs.push_back({"f" + std::to_string(i), k.ks[i]});
  emit_digits(o, "  ", "idx", "", kord, false, [&](int q) { return kc[q]; }, offs);
  const uint32_t NP = k.NP;
  const bool tail = NP % (256u * XI) != 0;
  pgmi_appendf(o, "  const unsigned xbase = xb * %uu + threadIdx.x;\n", 256u * XI);
  for (int u = 0; u < XI; ++u) {
    pgmi_appendf(o, "  const unsigned x%d = xbase + %uu;\n", u, 256u * u);
    if (tail)
      pgmi_appendf(o, "  const unsigned c%d = x%d < %uu ? x%d : %uu;\n", u, u, NP, u, NP - 1);
    else
      pgmi_appendf(o, "  const unsigned c%d = x%d;\n", u, u);
  }
  // operands constant over the reduced entries: once per block
  for (int i = 0; i < k.n_ops; ++i) {
    if (k.jvar[i]) continue;
    if (k.vec[i]) {
      for (int u = 0; u < XI; ++u)
        pgmi_appendf(o, "  const pgm_d2 h%d_%d = ((const pgm_d2 *)(o%d + f%d))[c%d];\n", i, u, i, i, u);
    } else if (tiled(i)) {
      for (unsigned t = 0; t < T; ++t)
        pgmi_appendf(o, "  const double h%d%s = o%d[f%d + %lldLL];\n", i, tsfx(t).c_str(), i, i,
                     (long long)t * (long long)k.ks[i][td]);
    } else {
      pgmi_appendf(o, "  const double h%d = o%d[f%d];\n", i, i, i);
    }
  }
  const char *init = red == PGM_RED_MAX ? "-__builtin_inf()" : "0.0";
  for (unsigned t = 0; t < T && has_m; ++t)
    for (int u = 0; u < XI; ++u) pgmi_appendf(o, "  pgm_d2 a%d%s = {%s, %s};\n", u, tsfx(t).c_str(), init, init);
  // reduced dims as nested loops (dim 0 outermost: the generic kernel's entry order); the innermost
  // dims whose trip product stays within `unroll` are unrolled
  const int unrolled = first_unrolled(0, k.nr, 1, (uint64_t)unroll, [&](int r) { return k.rdiv[r].d; });
  std::string ind = "  ";
  for (int r = 0; r < k.nr; ++r) {
    if (r >= unrolled)
      pgmi_appendf(o, "%s#pragma unroll\n", ind.c_str());
    else if (r == k.nr - 1)  // an innermost loop too long to unroll fully: `unroll` entries at a time
      pgmi_appendf(o, "%s#pragma unroll %d\n", ind.c_str(), std::max(1, unroll));
    else
      pgmi_appendf(o, "%s#pragma unroll 1\n", ind.c_str());
    pgmi_appendf(o, "%sfor (int r%d = 0; r%d < %u; ++r%d) {\n", ind.c_str(), r, r, k.rdiv[r].d, r);
    ind += "  ";
  }
  auto lin = [&](const int64_t *s) {  // literal offset of the current reduced entry
    std::string e = "0LL";
    for (int r = 0; r < k.nr; ++r)
      if (s[r]) e += " + (long long)r" + std::to_string(r) + " * " + std::to_string((long long)s[r]) + "LL";
    return e;
  };
  for (int i = 0; i < k.n_ops; ++i) {
    if (!k.jvar[i]) continue;
    const std::string J = lin(k.rs[i]);
    if (k.vec[i]) {
      pgmi_appendf(o, "%sconst pgm_d2 *p%d = (const pgm_d2 *)(o%d + f%d + %s);\n", ind.c_str(), i, i, i, J.c_str());
      for (int u = 0; u < XI; ++u) pgmi_appendf(o, "%sconst pgm_d2 v%d_%d = p%d[c%d];\n", ind.c_str(), i, u, i, u);
    } else if (tiled(i)) {
      for (unsigned t = 0; t < T; ++t)
        pgmi_appendf(o, "%sconst double s%d%s = o%d[f%d + %s + %lldLL];\n", ind.c_str(), i, tsfx(t).c_str(), i, i,
                     J.c_str(), (long long)t * (long long)k.ks[i][td]);
    } else {
      pgmi_appendf(o, "%sconst double s%d = o%d[f%d + %s];\n", ind.c_str(), i, i, i, J.c_str());
    }
  }
  for (unsigned t = 0; t < T; ++t) {
    const std::string ts = tsfx(t);
    for (int u = 0; u < XI; ++u) {
      for (int h = 0; h < 2; ++h) {
        const char cx = h ? 'y' : 'x';
        auto term = [&](int i) {
          char buf[64];
          const char *sf = tiled(i) ? ts.c_str() : "";
          if (k.jvar[i] && k.vec[i]) snprintf(buf, sizeof buf, "v%d_%d.%c", i, u, cx);
          else if (k.jvar[i]) snprintf(buf, sizeof buf, "s%d%s", i, sf);
          else if (k.vec[i]) snprintf(buf, sizeof buf, "h%d_%d.%c", i, u, cx);
          else snprintf(buf, sizeof buf, "h%d%s", i, sf);
          return std::string(buf);
        };
        std::string e = "1.0";
        for (int i = 0; i < k.n_ops; ++i) {
          if (k.kind[i] == PGM_PRODN_MUL) e = "(" + e + " * " + term(i) + ")";
          else if (k.kind[i] == PGM_PRODN_RATIO && i + 1 < MOPS)
            e = "(" + e + " * pgm_ratio(" + term(i) + ", " + term(i + 1) + "))";
        }
        pgmi_appendf(o, "%sconst double w%d%s%c = %s;\n", ind.c_str(), u, ts.c_str(), cx, e.c_str());
      }
      pgmi_appendf(o, "%sconst pgm_d2 w%d%s = {w%d%sx, w%d%sy};\n", ind.c_str(), u, ts.c_str(), u, ts.c_str(), u,
                   ts.c_str());
    }
  }
  if (store) {
    pgmi_appendf(o, "%spgm_d2 *cj = (pgm_d2 *)(C + oc + %s);\n", ind.c_str(), lin(k.rsc).c_str());
    for (int u = 0; u < XI; ++u) {
      const std::string guard = tail ? "if (x" + std::to_string(u) + " < " + std::to_string(NP) + "u) " : "";
      if (nt)
        pgmi_appendf(o, "%s%s__builtin_nontemporal_store(w%d, cj + x%d);\n", ind.c_str(), guard.c_str(), u, u);
      else
        pgmi_appendf(o, "%s%scj[x%d] = w%d;\n", ind.c_str(), guard.c_str(), u, u);
    }
  }
  for (unsigned t = 0; t < T && has_m; ++t) {
    const std::string tss = tsfx(t);
    const char *ts = tss.c_str();
    for (int u = 0; u < XI; ++u) {
      if (red == PGM_RED_MAX)
        pgmi_appendf(o, "%sa%d%s.x = pgm_maxn(a%d%s.x, w%d%s.x); a%d%s.y = pgm_maxn(a%d%s.y, w%d%s.y);\n", ind.c_str(),
                     u, ts, u, ts, u, ts, u, ts, u, ts, u, ts);
      else
        pgmi_appendf(o, "%sa%d%s += w%d%s;\n", ind.c_str(), u, ts, u, ts);
    }
  }
  for (int r = k.nr - 1; r >= 0; --r) {
    ind.resize(ind.size() - 2);
    pgmi_appendf(o, "%s}\n", ind.c_str());
  }
  // a marginal divided by an operand constant over the summed entries (PGM_PRODN_MDIV: sigma' / mu)
  if (has_m && k.mdiv >= 0) {
    const int i = k.mdiv;
    for (int u = 0; u < XI; ++u) {
      if (k.vec[i])
        pgmi_appendf(o, "  a%d = (pgm_d2){pgm_ratio(a%d.x, h%d_%d.x), pgm_ratio(a%d.y, h%d_%d.y)};\n", u, u, i, u, u, i, u);
      else
        pgmi_appendf(o, "  a%d = (pgm_d2){pgm_ratio(a%d.x, h%d), pgm_ratio(a%d.y, h%d)};\n", u, u, i, u, i);
    }
  }
  // marginal stores: nontemporal when the step stores no product (a marginal-only pass writes nothing
  // else), plain (write-back L2) otherwise
  for (unsigned t = 0; t < T && has_m; ++t) {
    const std::string ts = tsfx(t);
    const std::string mo = T > 1 ? "M + om + " + std::to_string((long long)t * (long long)k.ksm[td]) + "LL" : "M + om";
    for (int u = 0; u < XI; ++u) {
      const std::string guard = tail ? "if (x" + std::to_string(u) + " < " + std::to_string(NP) + "u) " : "";
      if (!store)
        pgmi_appendf(o, "  %s__builtin_nontemporal_store(a%d%s, (pgm_d2 *)(%s) + x%d);\n", guard.c_str(), u, ts.c_str(),
                     mo.c_str(), u);
      else
        pgmi_appendf(o, "  %s((pgm_d2 *)(%s))[x%d] = a%d%s;\n", guard.c_str(), mo.c_str(), u, u, ts.c_str());
    }
  }
  o += "}\n";
  return o;
}

static std::string pm_multi_body(const PMSpec &sp, const std::string &name) {
  // the target with fewer states of its own dims (R_reg) keeps one register accumulator per state,
  // its dims unrolled innermost; the other target's own dims (R_str) are runtime loops outermost, and
  // its marginal is complete after each of their iterations (everything inside is summed), so it is
  // stored there — registers stay bounded by the smaller target
  const PMMulti &q = sp.mm;
  const int red = sp.red;
  const int treg = q.n1 <= q.n2 ? 0 : 1;  // 0: M1 (C slot) in registers, 1: M2 (M slot)
  const int64_t *sreg = treg == 0 ? q.u1 : q.u2;
  const int64_t *sstr = treg == 0 ? q.u2 : q.u1;
  const char *preg = treg == 0 ? "C" : "M", *pstr = treg == 0 ? "M" : "C";
  const char *mreg = treg == 0 ? "m1" : "m2", *mstr = treg == 0 ? "m2" : "m1";
  const unsigned nreg = treg == 0 ? q.n1 : q.n2;
  std::string o;
  o += pm_signature(name, q.n_ops);
  if (sp.xcd) o += pm_xcd_remap(sp.total);
  pgmi_appendf(o, "  const unsigned xb = b %% %uu, ob = b / %uu;\n", sp.gx, sp.gx);
  o += "  unsigned idx = ob;\n  long long m1 = 0, m2 = 0";
  for (int i = 0; i < q.n_ops; ++i) pgmi_appendf(o, ", f%d = 0", i);
  o += ";\n  (void)idx;\n";
  auto op_bytes = [&](int i) {
    double b = q.vec[i] ? 16.0 * q.NP : 8.0;
    for (int d = 0; d < q.nK; ++d)
      if (q.ks[i][d]) b *= q.kcard[d];
    for (int d = 0; d < q.nU; ++d)
      if (q.us[i][d]) b *= q.ucard[d];
    for (int d = 0; d < q.nZ; ++d)
      if (q.zs[i][d]) b *= q.zcard[d];
    return b;
  };
  const std::vector<int> kord = pm_kept_order(q.nK, q.kcard, [&](int d) {
    double t = 0.0;
    for (int i = 0; i < q.n_ops; ++i)
      if (q.vec[i] && q.ks[i][d]) t += op_bytes(i);
    return t;
  });
  std::vector<Off> offs = {{"m1", q.k1}, {"m2", q.k2}};
  for (int i = 0; i < q.n_ops; ++i) offs.push_back({"f" + std::to_string(i), q.ks[i]});
  emit_digits(o, "  ", "idx", "", kord, false, [&](int d) { return q.kcard[d]; }, offs);
  const bool tail = q.NP % 256u != 0;
  o += "  const unsigned x = xb * 256u + threadIdx.x;\n";
  if (tail) pgmi_appendf(o, "  const unsigned c = x < %uu ? x : %uu;\n", q.NP, q.NP - 1);
  else o += "  const unsigned c = x;\n";
  const std::string guard = tail ? "if (x < " + std::to_string(q.NP) + "u) " : "";
  const char *init = red == PGM_RED_MAX ? "-__builtin_inf()" : "0.0";
  for (unsigned a = 0; a < nreg; ++a) pgmi_appendf(o, "  pgm_d2 ar_%u = {%s, %s};\n", a, init, init);
  // runtime loops: the streamed target's own dims (u), then the dims neither keeps (z)
  std::string ind = "  ";
  std::vector<int> ustr, ureg;
  for (int d = 0; d < q.nU; ++d) (sstr[d] ? ustr : ureg).push_back(d);
  for (int d : ustr) {
    pgmi_appendf(o, "%s#pragma unroll 1\n%sfor (int u%d = 0; u%d < %u; ++u%d) {\n", ind.c_str(), ind.c_str(), d, d,
            q.ucard[d], d);
    ind += "  ";
  }
  pgmi_appendf(o, "%spgm_d2 as = {%s, %s};\n", ind.c_str(), init, init);
  for (int z = 0; z < q.nZ; ++z) {
    pgmi_appendf(o, "%s#pragma unroll %s\n", ind.c_str(), z == q.nZ - 1 ? "2" : "1");
    pgmi_appendf(o, "%sfor (int z%d = 0; z%d < %u; ++z%d) {\n", ind.c_str(), z, z, q.zcard[z], z);
    ind += "  ";
  }
  auto runtime_off = [&](const int64_t *zs, const int64_t (*us)[KMAX], int i) {
    std::string e;
    for (int z = 0; z < q.nZ; ++z)
      if (zs[z]) e += " + (long long)z" + std::to_string(z) + " * " + std::to_string((long long)zs[z]) + "LL";
    for (int d : ustr)
      if (us[i][d]) e += " + (long long)u" + std::to_string(d) + " * " + std::to_string((long long)us[i][d]) + "LL";
    return e;
  };
  uint64_t nr = 1;
  for (int d : ureg) nr *= q.ucard[d];
  for (uint64_t ra = 0; ra < nr; ++ra) {
    unsigned dig[KMAX] = {};
    uint64_t rem = ra;
    for (int k = (int)ureg.size() - 1; k >= 0; --k) {
      dig[ureg[k]] = (unsigned)(rem % q.ucard[ureg[k]]);
      rem /= q.ucard[ureg[k]];
    }
    int64_t off[MOPS] = {};
    for (int d : ureg)
      for (int i = 0; i < q.n_ops; ++i) off[i] += (int64_t)dig[d] * q.us[i][d];
    pgmi_appendf(o, "%s{\n", ind.c_str());
    for (int i = 0; i < q.n_ops; ++i) {
      const std::string ro = runtime_off(q.zs[i], q.us, i);
      if (q.vec[i])
        pgmi_appendf(o, "%s  const pgm_d2 v%d = ((const pgm_d2 *)(o%d + f%d + %lldLL%s))[c];\n", ind.c_str(), i, i, i,
                (long long)off[i], ro.c_str());
      else
        pgmi_appendf(o, "%s  const double s%d = o%d[f%d + %lldLL%s];\n", ind.c_str(), i, i, i, (long long)off[i],
                ro.c_str());
    }
    for (int h = 0; h < 2; ++h) {
      const char cx = h ? 'y' : 'x';
      auto term = [&](int i) {
        char buf[32];
        if (q.vec[i]) snprintf(buf, sizeof buf, "v%d.%c", i, cx);
        else snprintf(buf, sizeof buf, "s%d", i);
        return std::string(buf);
      };
      std::string e = "1.0";
      for (int i = 0; i < q.n_ops; ++i) {
        if (q.kind[i] == PGM_PRODN_MUL) e = "(" + e + " * " + term(i) + ")";
        else if (q.kind[i] == PGM_PRODN_RATIO && i + 1 < MOPS)
          e = "(" + e + " * pgm_ratio(" + term(i) + ", " + term(i + 1) + "))";
      }
      pgmi_appendf(o, "%s  const double w%c = %s;\n", ind.c_str(), cx, e.c_str());
    }
    pgmi_appendf(o, "%s  const pgm_d2 w = {wx, wy};\n", ind.c_str());
    if (red == PGM_RED_MAX)
      pgmi_appendf(o, "%s  ar_%llu.x = pgm_maxn(ar_%llu.x, w.x); ar_%llu.y = pgm_maxn(ar_%llu.y, w.y); "
                 "as.x = pgm_maxn(as.x, w.x); as.y = pgm_maxn(as.y, w.y);\n",
              ind.c_str(), (unsigned long long)ra, (unsigned long long)ra, (unsigned long long)ra,
              (unsigned long long)ra);
    else
      pgmi_appendf(o, "%s  ar_%llu += w; as += w;\n", ind.c_str(), (unsigned long long)ra);
    pgmi_appendf(o, "%s}\n", ind.c_str());
  }
  for (int z = q.nZ - 1; z >= 0; --z) {
    ind.resize(ind.size() - 2);
    pgmi_appendf(o, "%s}\n", ind.c_str());
  }
  {  // the streamed target's marginal for this iteration is complete
    std::string e;
    for (int d : ustr)
      e += " + (long long)u" + std::to_string(d) + " * " + std::to_string((long long)sstr[d]) + "LL";
    pgmi_appendf(o, "%s%s((pgm_d2 *)(%s + %s%s))[x] = as;\n", ind.c_str(), guard.c_str(), pstr, mstr, e.c_str());
  }
  for (size_t k = 0; k < ustr.size(); ++k) {
    ind.resize(ind.size() - 2);
    pgmi_appendf(o, "%s}\n", ind.c_str());
  }
  for (uint64_t ra = 0; ra < nr; ++ra) {  // register target: accumulator ra at its digits' offset
    uint64_t rem = ra;
    int64_t off = 0;
    for (int k = (int)ureg.size() - 1; k >= 0; --k) {
      off += (int64_t)(rem % q.ucard[ureg[k]]) * sreg[ureg[k]];
      rem /= q.ucard[ureg[k]];
    }
    pgmi_appendf(o, "  %s((pgm_d2 *)(%s + %s + %lldLL))[x] = ar_%llu;\n", guard.c_str(), preg, mreg, (long long)off,
            (unsigned long long)ra);
  }
  o += "}\n";
  return o;
}

// kernel pgm_pm over the bodies (kernel argument: each body's operand pointers, then C and M); starts[i] = first block of
// body i, returns the grid size through *blocks
std::string pm_source(const std::vector<PMSpec> &specs, std::vector<uint64_t> &starts, uint64_t *blocks) {
  std::string o =
      "#pragma clang fp contract(off)\n"  // products rounded before they are summed, as numpy does
      "typedef double pgm_d2 __attribute__((ext_vector_type(2)));\n"
      "typedef unsigned int pgm_u32x4 __attribute__((ext_vector_type(4)));\n"
      "__device__ __forceinline__ double pgm_ratio(double a, double b) { const double r = a / b; "
      "return r != r ? 0.0 : r; }\n"
      "__device__ __forceinline__ double pgm_maxn(double a, double b) { return (a > b || a != a) ? a : b; }\n";
  const size_t n = specs.size();
  starts.assign(n, 0);
  uint64_t at = 0;
  for (size_t i = 0; i < n; ++i) {
    at = (at + 7) / 8 * 8;
    starts[i] = at;
    at += specs[i].total;
    o += specs[i].multi ? pm_multi_body(specs[i], "pm" + std::to_string(i)) : pm_body(specs[i], "pm" + std::to_string(i));
  }
  *blocks = at;
  size_t nptr = 0;
  for (const PMSpec &sp : specs) nptr += (size_t)pm_nops(sp) + 2;
  pgmi_appendf(o, "struct pgm_pm_args { const double *p[%zu]; };\n", nptr);
  o += "extern \"C\" __global__ void __launch_bounds__(256) pgm_pm(const pgm_pm_args a) {\n"
       "  const unsigned b = blockIdx.x;\n";
  std::vector<std::string> calls(n);
  size_t base = 0;
  for (size_t i = 0; i < n; ++i) {
    const int no = pm_nops(specs[i]);
    std::string call = "pm" + std::to_string(i) + "(b - " + std::to_string((unsigned long long)starts[i]) + "u";
    for (int t = 0; t < no; ++t) call += ", a.p[" + std::to_string(base + t) + "]";
    call += ", (double *)a.p[" + std::to_string(base + no) + "], (double *)a.p[" + std::to_string(base + no + 1) + "])";
    base += (size_t)no + 2;
    calls[i] = call;
  }
  if (n == 1) {
    o += "  " + calls[0] + ";\n";
  } else {
    // a block finds its body through the tree of block-range comparisons (C4 rate unchanged against one compare
    // per body, r05p); blocks in the padding between bodies fall out at the leaf's upper bound
    block_tree(
        o, 0, n, "  ", [&](size_t i) { return (unsigned long long)starts[i]; },
        [&](size_t i, const std::string &ind) {
          pgmi_appendf(o, "%sif (b < %lluu) %s;\n", ind.c_str(), (unsigned long long)(starts[i] + specs[i].total),
                       calls[i].c_str());
        });
  }
  o += "}\n";
  return o;
}

// ----------------------------------------------------------------------------- the specialisation choice
bool pm_specialise(const ProdMK &k, int32_t reduce, bool store, bool has_m, PMSpec &sp) {
  // defaults measured on MI355X, pathfinder C4 (4,000 / 1,000 rows: generic 781K / 515K calibrations/s;
  // specialised above 2M entries 911K / 601K; + one row pair per lane, nontemporal belief stores and
  // XCD-grouped blocks 933K; threshold 256K entries 648K at 1,000 rows)
  // r03ag, after the schedule changes (direct collect operands, 128-block fused floor): 2^18 / 2^16 / 2^14
  // -> 0.96-0.97 / 1.024-1.026 / 1.026-1.028 M calibrations/s at 1,000 rows, 1.27-1.28 / 1.28-1.29 /
  // 1.29 M at 4,000 (small steps specialised join their level's merged launch instead of launching alone)
  // r06at: 2^12 (was 2^14) — C4's smallest steps (the 4-state F29/F92 clique) join their level's merged launch
  // instead of running as generic kernels: +0.5-0.7 % at 4,000 / 1,000 rows
  static constexpr uint64_t min_entries = 1ull << 12;
  // per step, at least this many row pairs per lane when the rows fill them: 2 measured (MI355X, C4
  // 4,000 rows: 1.146 -> 1.18 M calibrations/s; 1,000 rows unchanged, too few rows; forced 2 / 4 for
  // every step, or a minimum of 4: slower, profiles/r02bw_c4_xi.txt)
  static constexpr int xi_min = 2;
  // reduced entries unrolled (4 / 16: -2 % / -10 % at 4,000 rows, profiles/r04v/; 16 on the steps of few
  // blocks only: +1.7 % at 1,000 rows, -3 to -5 % at 4,000, profiles/r04z/)
  static constexpr int unroll = 8;
  // nontemporal belief stores (default-policy stores: -5 % / -9 % at 4,000 / 1,000 rows; write-through
  // product stores: -4 % / -8 %; profiles/r04v/)
  static constexpr bool nt = true;
  const uint64_t entries = (uint64_t)k.n_outer * (uint64_t)k.n_red * 2ull * k.NP;
  if (entries < min_entries) return false;
  // row pairs per lane: a block of a step with few reduced entries (separator messages from small
  // operands, products without a reduction) does little work per lane — one 16-B store and a few
  // loads — so its lifetime, not HBM, bounds the step; XI pairs per lane give each lane ~8 entries of
  // work while keeping >= 2,048 blocks (8 per CU) in the step
  int XI = (uint64_t)k.NP >= 256ull * xi_min ? xi_min : 1;
  {
    const uint64_t red = std::max<uint64_t>(1, (uint64_t)k.n_red);
    while (XI < 8 && red * (uint64_t)XI < 8) {
      const int nx = XI * 2;
      const uint64_t gx2 = (k.NP + 256ull * nx - 1) / (256ull * nx);
      const uint64_t pad = gx2 * 256ull * nx - k.NP;  // idle lanes in the last block of a row range
      if (gx2 * (uint64_t)k.n_outer < 2048 || pad * 4 > k.NP) break;
      XI = nx;
    }
  }
  const uint64_t gx = (k.NP + 256ull * XI - 1) / (256ull * XI);
  const uint64_t total = gx * (uint64_t)k.n_outer;
  if (total >= (1ull << 31)) return false;
  sp = PMSpec();
  sp.k = k;
  sp.red = reduce;
  sp.XI = XI;
  // entries unrolled: `unroll`, fewer when many row operands vary over the reduced entries (each unrolled
  // entry keeps XI 16-B loads per such operand in flight: at most ~48, the 3-operand steps' budget)
  int nvj = 0;
  for (int t = 0; t < k.n_ops; ++t) nvj += k.vec[t] && k.jvar[t];
  sp.unroll = std::max(1, std::min(unroll, 48 / std::max(1, nvj * XI)));
  sp.store = store;
  sp.has_m = has_m;
  sp.xcd = true;  // blocks grouped by XCD for any block count (bijective remap; r04c)
  sp.nt = nt;
  sp.gx = (unsigned)gx;
  sp.total = total;
  // a marginal-only pass re-loads its row operands (child messages) for every state of a kept dim that
  // only row-less operands (psi) carry — an L2-bound walk (C4 level 2: 64 states of the 32,256-state
  // clique); walk the largest such dim (2..8 states) inside the block instead, its states sharing the
  // loaded values, while >= 2,048 blocks remain and T x XI accumulators fit (C4, 4,000 rows: one batch in
  // flight 1.32-1.33 -> 1.36 M calibrations/s, two 1.39-1.43 -> 1.42-1.45 M; 1,000 rows unchanged; r05ac)
  if (!store && has_m && k.mdiv < 0) {
    unsigned best = 1;
    for (int q = 0; q + 1 < k.nk; ++q) {
      const unsigned d = k.kdiv[q].d;
      bool rowless = d >= 2 && d <= 8 && k.ksm[q] != 0;
      for (int t = 0; rowless && t < k.n_ops; ++t)
        if (k.vec[t] && k.ks[t][q]) rowless = false;
      if (rowless && d > best && total / d >= 2048 && d * (unsigned)XI <= 16) best = d, sp.tdim = q;
    }
    if (sp.tdim >= 0) {
      sp.T = best;
      sp.total = total / best;
    }
  }
  return true;
}

int plan_two_marginals(const pgm_productn_desc *d, const double *const *ops, const int64_t *s1, const int64_t *s2,
                       const double *M1, const double *M2, int32_t reduce, PMSpec &sp) {
  sp = PMSpec();
  PMMulti &q = sp.mm;
  if (!d || !ops || !s1 || !s2 || !M1 || !M2) return pgmi_failf(PGM_EINVAL, "product_n_marginals: null argument");
  if (d->n_ops < 1 || d->n_ops > MOPS || d->n_keep < 2 || d->n_keep > PGM_MAX_DIMS) return 0;
  const int last = d->n_keep - 1;
  const int64_t NX = d->keep_card[last];
  if (NX < 64 || NX % 2 || d->keep_sc[last] != 1 || s1[last] != 1 || s2[last] != 1) return 0;
  if (((uintptr_t)M1 & 15) || ((uintptr_t)M2 & 15)) return 0;
  q.n_ops = d->n_ops;
  for (int t = 0; t < d->n_ops; ++t) {
    if (!ops[t] || d->op_kind[t] < 0 || d->op_kind[t] > 2) return pgmi_failf(PGM_EINVAL, "product_n_marginals: operand %d", t);
    const int64_t sx = d->keep_s[t][last];
    if (sx != 0 && sx != 1) return 0;
    if (sx == 1 && ((uintptr_t)ops[t] & 15)) return 0;
    q.vec[t] = sx == 1;
    q.kind[t] = d->op_kind[t];
  }
  uint64_t nk = 1;
  for (int i = 0; i < last; ++i) {
    const int64_t c = d->keep_card[i];
    if (c <= 0) return pgmi_failf(PGM_EINVAL, "product_n_marginals: keep_card[%d] <= 0", i);
    if (c == 1) continue;
    if ((s1[i] && s1[i] % 2) || (s2[i] && s2[i] % 2)) return 0;
    for (int t = 0; t < d->n_ops; ++t)
      if (q.vec[t] && d->keep_s[t][i] % 2) return 0;
    if (s1[i] && s2[i]) {
      if (q.nK >= KMAX) return 0;
      q.kcard[q.nK] = (unsigned)c;
      q.k1[q.nK] = s1[i];
      q.k2[q.nK] = s2[i];
      for (int t = 0; t < d->n_ops; ++t) q.ks[t][q.nK] = d->keep_s[t][i];
      ++q.nK;
      nk *= (uint64_t)c;
    } else if (s1[i] || s2[i]) {
      if (q.nU >= KMAX) return 0;
      q.ucard[q.nU] = (unsigned)c;
      q.u1[q.nU] = s1[i];
      q.u2[q.nU] = s2[i];
      for (int t = 0; t < d->n_ops; ++t) q.us[t][q.nU] = d->keep_s[t][i];
      ++q.nU;
      if (s1[i]) q.n1 *= (unsigned)c;
      else q.n2 *= (unsigned)c;
    } else {
      if (q.nZ >= KMAX) return 0;
      q.zcard[q.nZ] = (unsigned)c;
      for (int t = 0; t < d->n_ops; ++t) q.zs[t][q.nZ] = d->keep_s[t][i];
      ++q.nZ;
    }
  }
  // register accumulators: the smaller target's own states, unrolled (8 / 32: no better, profiles/r02bv_c4_knobs.txt)
  static constexpr unsigned max_acc = 16u;
  if (std::min(q.n1, q.n2) > max_acc || nk >= (1ull << 31)) return 0;
  q.n_outer = (uint32_t)nk;
  q.NP = (uint32_t)(NX / 2);
  const uint64_t gx = (q.NP + 255) / 256;
  if (gx * nk < 256) return 0;  // fewer blocks than CUs: two single-marginal passes fill the chip better
  sp.multi = 1;
  sp.red = reduce;
  sp.store = false;
  sp.gx = (unsigned)gx;
  sp.total = gx * nk;
  sp.xcd = true;
  return 1;
}

// ----------------------------------------------------------------------------- specialised contraction batches
// A batch of contraction jobs (one dependency level of a compiled contraction path, C1 / C2; or the
// single-workgroup chain of its tiny last levels) as ONE generated kernel: each job's output decode
// (literal divisors), operand strides, reduction walk (literal nested loops, the generic kernels' entry
// order: reduction-outer dims slowest first, the innermost dim last) and lanes per output are
// literals, and a block finds its job by comparing its index with literal ranges — no block map, no
// descriptor loads (the generic k_batch_c reads a block map entry, then ~600 B of descriptor, before
// its first operand load; k_batch_wg_c reads its descriptors field by field from LDS).

static constexpr uint64_t kUnrollProd = 64;  // trip product up to which a job's innermost reduction loops unroll

static std::string cs_combine(int cmb, const std::string &a, const std::string &b) {
  switch (cmb) {
    case PGM_COMBINE_MUL: return "(" + a + " * " + b + ")";
    case PGM_COMBINE_ADD: return "(" + a + " + " + b + ")";
    case PGM_COMBINE_DIV: return "pgm_div0(" + a + ", " + b + ")";
    case PGM_COMBINE_DIV_RAW: return "(" + a + " / " + b + ")";
    default: return a;  // COPY
  }
}

static std::string cs_red(int red, const std::string &acc, const std::string &v) {
  if (red == PGM_RED_SUM) return acc + " = " + acc + " + " + v + ";";
  if (red == PGM_RED_MAX) return acc + " = pgm_maxn(" + acc + ", " + v + ");";
  return acc + " = " + v + ";";
}

// the job's output index decode: oa / ob / oc from idx (the kept dims, the last one fastest)
static void cs_decode(std::string &o, const ContractK &k, bool use_b) {
  std::vector<Off> offs = {{"oa", k.ksa}};
  if (use_b) offs.push_back({"ob", k.ksb});
  offs.push_back({"oc", k.ksc});
  emit_digits(o, "    ", "idx", "_", descending(k.nk), true, [&](int i) { return k.kdiv[i].d; }, offs);
}

// nested loops over the reduction-outer dims (dim 0 outermost) opening; returns the offset expressions
static void cs_red_loops_open(std::string &o, const ContractK &k, std::string &ind, uint64_t inner_trip) {
  // the innermost reduction dims are unrolled while their trip product stays <= 64, so a 48-entry walk issues
  // its loads together instead of in six dependent rounds (r06q/r06r: C2 91.4 -> 88.6 us; 16 before, 256 no
  // better)
  const int unrolled = first_unrolled(0, k.nr - 1, inner_trip, kUnrollProd, [&](int r) { return k.rdiv[r].d; });
  for (int r = 0; r < k.nr - 1; ++r) {
    pgmi_appendf(o, "%s#pragma unroll%s\n", ind.c_str(), r >= unrolled ? "" : " 1");
    pgmi_appendf(o, "%sfor (unsigned r%d = 0; r%d < %uu; ++r%d) {\n", ind.c_str(), r, r, k.rdiv[r].d, r);
    ind += "  ";
  }
}

static void cs_red_loops_close(std::string &o, const ContractK &k, std::string &ind) {
  for (int r = 0; r < k.nr - 1; ++r) {
    ind.resize(ind.size() - 2);
    pgmi_appendf(o, "%s}\n", ind.c_str());
  }
}

static std::string cs_ro_off(const ContractK &k, bool a) {
  std::string e = "0LL";
  for (int r = 0; r < k.nr - 1; ++r) {
    const long long s = a ? (long long)k.rsa[r] : (long long)k.rsb[r];
    if (s) e += " + (long long)r" + std::to_string(r) + " * " + std::to_string(s) + "LL";
  }
  return e;
}

static std::string cs_job_body(const pgmi_cs_job &J, const std::string &name) {
  const ContractK &k = J.k;
  const bool use_b = J.cmb != PGM_COMBINE_COPY;
  const char *init = J.red == PGM_RED_MAX ? "-__builtin_inf()" : "0.0";
  std::string o;
  pgmi_appendf(o, "__device__ __forceinline__ void %s(unsigned tid, unsigned nth, const double *__restrict__ A, "
                  "const double *__restrict__ B, double *__restrict__ C) {\n  (void)B;\n", name.c_str());
  const std::string ra = cs_ro_off(k, true), rb = cs_ro_off(k, false);
  const unsigned RI = k.ri_card;
  if (k.row_mode == 2) {  // output pairs along the innermost kept dim, 16-B accesses (contract_flat2)
    const int kx = k.nk - 1;
    const bool va = k.ksa[kx] != 0, vb = use_b && k.ksb[kx] != 0;
    pgmi_appendf(o, "  for (unsigned q = tid; q < %uu; q += nth) {\n", k.n_out >> 1);
    o += "    unsigned idx = q << 1;\n    long long oa = 0, ob = 0, oc = 0; (void)ob;\n";
    cs_decode(o, k, use_b);
    pgmi_appendf(o, "    double lo = %s, hi = %s;\n", init, init);
    std::string ind = "    ";
    cs_red_loops_open(o, k, ind, RI);
    pgmi_appendf(o, "%s#pragma unroll%s\n", ind.c_str(), RI <= 16 ? "" : " 4");
    pgmi_appendf(o, "%sfor (unsigned ri = 0; ri < %uu; ++ri) {\n", ind.c_str(), RI);
    const std::string in = ind + "  ";
    pgmi_appendf(o, "%sconst double *a_ = A + oa + %s + (long long)ri * %lldLL;\n", in.c_str(), ra.c_str(), (long long)k.ri_sa);
    if (va) pgmi_appendf(o, "%sconst pgm_d2 xa = *(const pgm_d2 *)a_;\n", in.c_str());
    else pgmi_appendf(o, "%sconst double xs_ = *a_; const pgm_d2 xa = {xs_, xs_};\n", in.c_str());
    if (use_b) {
      pgmi_appendf(o, "%sconst double *b_ = B + ob + %s + (long long)ri * %lldLL;\n", in.c_str(), rb.c_str(), (long long)k.ri_sb);
      if (vb) pgmi_appendf(o, "%sconst pgm_d2 xb = *(const pgm_d2 *)b_;\n", in.c_str());
      else pgmi_appendf(o, "%sconst double ys_ = *b_; const pgm_d2 xb = {ys_, ys_};\n", in.c_str());
    }
    pgmi_appendf(o, "%s%s\n", in.c_str(), cs_red(J.red, "lo", cs_combine(J.cmb, "xa.x", "xb.x")).c_str());
    pgmi_appendf(o, "%s%s\n", in.c_str(), cs_red(J.red, "hi", cs_combine(J.cmb, "xa.y", "xb.y")).c_str());
    pgmi_appendf(o, "%s}\n", ind.c_str());
    cs_red_loops_close(o, k, ind);
    o += "    *(pgm_d2 *)(C + oc) = (pgm_d2){lo, hi};\n  }\n}\n";
    return o;
  }
  const unsigned G = 1u << k.g_log2;
  // G lanes of an output at stride 64/G within a wave, as the n-ary jobs (cs_nary_body)
  const bool lm = G > 1 && G < 64;
  if (lm) {
    const unsigned P = 64u / G;
    pgmi_appendf(o, "  const unsigned lane_g = (tid & 63u) / %uu;\n", P);
    pgmi_appendf(o, "  for (unsigned out = (tid >> 6) * %uu + (tid & %uu); out < %uu; out += (nth >> 6) * %uu) {\n", P, P - 1,
                 k.n_out, P);
  } else {
    if (G > 1) pgmi_appendf(o, "  const unsigned lane_g = tid & %uu;\n", G - 1);
    pgmi_appendf(o, "  for (unsigned out = tid >> %d; out < %uu; out += nth >> %d) {\n", k.g_log2, k.n_out, k.g_log2);
  }
  o += "    unsigned idx = out;\n    long long oa = 0, ob = 0, oc = 0; (void)ob;\n";
  cs_decode(o, k, use_b);
  pgmi_appendf(o, "    double acc = %s;\n", init);
  std::string ind = "    ";
  cs_red_loops_open(o, k, ind, G > 1 ? (RI + G - 1) / G : RI);
  if (G > 1) {
    pgmi_appendf(o, "%sfor (unsigned ri = lane_g; ri < %uu; ri += %uu) {\n", ind.c_str(), RI, G);
  } else {
    pgmi_appendf(o, "%s#pragma unroll%s\n", ind.c_str(), RI <= 16 ? "" : " 8");
    pgmi_appendf(o, "%sfor (unsigned ri = 0; ri < %uu; ++ri) {\n", ind.c_str(), RI);
  }
  const std::string in = ind + "  ";
  std::string va = "A[oa + " + ra + " + (long long)ri * " + std::to_string((long long)k.ri_sa) + "LL]";
  std::string vb = "B[ob + " + rb + " + (long long)ri * " + std::to_string((long long)k.ri_sb) + "LL]";
  pgmi_appendf(o, "%s%s\n", in.c_str(), cs_red(J.red, "acc", cs_combine(J.cmb, va, vb)).c_str());
  pgmi_appendf(o, "%s}\n", ind.c_str());
  cs_red_loops_close(o, k, ind);
  if (G > 1 && J.red != PGM_RED_NONE)
    for (unsigned off = lm ? 32u : G >> 1; off > 0 && off >= (lm ? 64u / G : 1u); off >>= 1)
      pgmi_appendf(o, "    %s\n", cs_red(J.red, "acc", "__shfl_xor(acc, " + std::to_string(off) + ", 64)").c_str());
  pgmi_appendf(o, "    %sC[oc] = acc;\n  }\n}\n", G > 1 ? "if (lane_g == 0) " : "");
  return o;
}

// an evidence gather job (gather_body): C[out] = A[kept offset + sum_j code_j x stride_j], a code out of its
// variable's range raises the error flag and reads state 0
static std::string cs_gather_body(const pgmi_cs_job &J, const std::string &name) {
  const GatherK &g = J.g;
  std::string o;
  pgmi_appendf(o, "__device__ __forceinline__ void %s(unsigned tid, unsigned nth, const double *__restrict__ A, "
                  "const unsigned char *__restrict__ K, double *__restrict__ C, int *__restrict__ E) {\n"
                  "  (void)K; (void)E;\n", name.c_str());
  pgmi_appendf(o, "  for (unsigned out = tid; out < %uu; out += nth) {\n", g.n_out);
  o += "    unsigned idx = out, row = 0;\n    long long oa = 0, oc = 0;\n    (void)row;\n";
  emit_digits(o, "    ", "idx", "_", descending(g.nk), true, [&](int i) { return g.kdiv[i].d; },
              {{"oa", g.ksa}, {"oc", g.ksc}}, g.batch_dim);
  for (int j = 0; j < g.n_ev; ++j) {
    pgmi_appendf(o, "    { unsigned c_ = K[%lldLL + (long long)row];", (long long)(g.ev_col[j] * g.ld + g.row0));
    pgmi_appendf(o, " if (c_ >= %uu) { if (E) atomicOr(E, 1); c_ = 0; }", (unsigned)g.ev_card[j]);
    pgmi_appendf(o, " oa += (long long)c_ * %lldLL; }\n", (long long)g.ev_stride[j]);
  }
  o += "    C[oc] = A[oa];\n  }\n}\n";
  return o;
}

// an n-ary contraction job (r06; pgm_batch_add_contract_n): C[out] = reduce over the reduction space of
// X_0 * X_1 * ... (a left fold), every decode and stride a literal; G lanes per output stride through the
// flattened reduction index (its digits decoded with literal divisors), else literal nested loops
static std::string cs_nary_body(const pgmi_cs_job &J, const std::string &name) {
  const ContractNK &k = J.n;
  const int n = k.n_ops;
  const bool mx = k.red == PGM_RED_MAX;
  const char *init = mx ? "-__builtin_inf()" : "0.0";
  std::string o;
  pgmi_appendf(o, "__device__ __forceinline__ void %s(unsigned tid, unsigned nth", name.c_str());
  for (int t = 0; t < n; ++t) pgmi_appendf(o, ", const double *__restrict__ X%d", t);
  o += ", double *__restrict__ C) {\n";
  const unsigned G = 1u << k.g_log2;
  // lanes of an output: 1 < G < 64 takes the G lanes of an output at stride 64/G within a wave (lane_g = the
  // high lane bits), so a wave's consecutive lanes hold consecutive outputs and an operand that is unit-stride
  // along the output's fastest dim is read in runs instead of one line per lane (G = 64: the whole wave)
  const bool lm = G > 1 && G < 64;
  if (lm) {
    const unsigned P = 64u / G;
    pgmi_appendf(o, "  const unsigned lane_g = (tid & 63u) / %uu;\n", P);
    pgmi_appendf(o, "  for (unsigned out = (tid >> 6) * %uu + (tid & %uu); out < %uu; out += (nth >> 6) * %uu) {\n", P, P - 1,
                 k.n_out, P);
  } else {
    if (G > 1) pgmi_appendf(o, "  const unsigned lane_g = tid & %uu;\n", G - 1);
    pgmi_appendf(o, "  for (unsigned out = tid >> %d; out < %uu; out += nth >> %d) {\n", k.g_log2, k.n_out, k.g_log2);
  }
  o += "    unsigned idx = out; long long oc = 0;";
  for (int t = 0; t < n; ++t) pgmi_appendf(o, " long long o%d = 0;", t);
  o += "\n";
  {
    std::vector<Off> offs = {{"oc", k.ksc}};
    for (int t = 0; t < n; ++t) offs.push_back({"o" + std::to_string(t), k.ks[t]});
    emit_digits(o, "    ", "idx", "_", descending(k.nk), true, [&](int i) { return k.kcard[i]; }, offs);
  }
  auto prod = [&](const std::vector<std::string> &off) {
    std::string e = "X0[" + off[0] + "]";
    for (int t = 1; t < n; ++t) e = "(" + e + " * X" + std::to_string(t) + "[" + off[t] + "])";
    return e;
  };
  auto rcard = [&](int r) { return k.rcard[r]; };
  auto upd = [&](const std::string &v) {
    return mx ? "acc = pgm_maxn(acc, " + v + ");" : "acc = acc + " + v + ";";
  };
  pgmi_appendf(o, "    double acc = %s;\n", init);
  if (k.nr == 0) {
    std::vector<std::string> off;
    for (int t = 0; t < n; ++t) off.push_back("o" + std::to_string(t));
    o += "    acc = " + prod(off) + ";\n";
  } else if (G > 1) {
    // the G lanes of an output stride over the flattened index of the OUTER reduction dims [0, s) only — the
    // fewest outer dims whose product reaches G — and walk the inner dims [s, nr) as literal nested loops:
    // digits are decoded once per outer index instead of once per summed entry (r06).  When no proper prefix
    // reaches G the whole reduction index is flattened and decoded per entry
    int sd = k.nr;
    uint64_t pout = 1;
    for (int i = 0; i < k.nr; ++i) {
      pout *= k.rcard[i];
      if (pout >= G) {
        sd = i + 1;
        break;
      }
    }
    if (sd == k.nr) pout = k.n_red;
    pgmi_appendf(o, "    #pragma unroll %d\n    for (unsigned r = lane_g; r < %lluu; r += %uu) {\n      unsigned ri = r;",
                 sd == k.nr ? 4 : 1, (unsigned long long)pout, G);
    for (int t = 0; t < n; ++t) pgmi_appendf(o, " long long p%d = o%d;", t, t);
    o += "\n";
    std::vector<Off> poffs;
    for (int t = 0; t < n; ++t) poffs.push_back({"p" + std::to_string(t), k.rs[t]});
    emit_digits(o, "      ", "ri", "_", descending(sd), true, rcard, poffs);
    if (sd < k.nr) {
      const int unrolled = first_unrolled(sd, k.nr, 1, kUnrollProd, rcard);
      std::string ind = "      ";
      for (int r = sd; r < k.nr; ++r) {
        pgmi_appendf(o, "%s#pragma unroll%s\n", ind.c_str(), r >= unrolled ? "" : " 2");
        pgmi_appendf(o, "%sfor (unsigned r%d = 0; r%d < %uu; ++r%d) {\n", ind.c_str(), r, r, k.rcard[r], r);
        ind += "  ";
      }
      std::vector<std::string> off;
      for (int t = 0; t < n; ++t) {
        std::string e = "p" + std::to_string(t);
        for (int r = sd; r < k.nr; ++r)
          if (k.rs[t][r]) e += " + (long long)r" + std::to_string(r) + " * " + std::to_string((long long)k.rs[t][r]) + "LL";
        off.push_back(e);
      }
      o += ind + upd(prod(off)) + "\n";
      for (int r = sd; r < k.nr; ++r) {
        ind.resize(ind.size() - 2);
        o += ind + "}\n";
      }
      o += "    }\n";
    } else {
      std::vector<std::string> off;
      for (int t = 0; t < n; ++t) off.push_back("p" + std::to_string(t));
      o += "      " + upd(prod(off)) + "\n    }\n";
    }
  } else {
    std::string ind = "    ";
    const int unrolled = first_unrolled(0, k.nr, 1, kUnrollProd, rcard);
    for (int r = 0; r < k.nr; ++r) {
      pgmi_appendf(o, "%s#pragma unroll%s\n", ind.c_str(), r >= unrolled ? "" : " 2");
      pgmi_appendf(o, "%sfor (unsigned r%d = 0; r%d < %uu; ++r%d) {\n", ind.c_str(), r, r, k.rcard[r], r);
      ind += "  ";
    }
    std::vector<std::string> off;
    for (int t = 0; t < n; ++t) {
      std::string e = "o" + std::to_string(t);
      for (int r = 0; r < k.nr; ++r)
        if (k.rs[t][r]) e += " + (long long)r" + std::to_string(r) + " * " + std::to_string((long long)k.rs[t][r]) + "LL";
      off.push_back(e);
    }
    o += ind + upd(prod(off)) + "\n";
    for (int r = 0; r < k.nr; ++r) {
      ind.resize(ind.size() - 2);
      o += ind + "}\n";
    }
  }
  if (lm)
    for (unsigned off = 32; off >= 64u / G; off >>= 1)
      pgmi_appendf(o, "    %s\n", upd("__shfl_xor(acc, " + std::to_string(off) + ", 64)").c_str());
  else if (G > 1)
    for (unsigned off = G >> 1; off > 0; off >>= 1)
      pgmi_appendf(o, "    %s\n", upd("__shfl_xor(acc, " + std::to_string(off) + ", 64)").c_str());
  pgmi_appendf(o, "    %sC[oc] = acc;\n  }\n}\n", G > 1 ? "if (lane_g == 0) " : "");
  return o;
}

static int cs_nptrs(const pgmi_cs_job &J) { return J.kind == 2 ? J.n.n_ops + 1 : J.kind == 1 ? 4 : 3; }

bool cs_source(const pgmi_cs_job *jobs, int n, const uint32_t *level_off, int n_levels, int one_wg, CSBatch &out) {
  out = CSBatch();
  std::vector<int> base(n > 0 ? n + 1 : 1, 0);
  for (int j = 0; j < n; ++j) base[j + 1] = base[j] + cs_nptrs(jobs[j]);
  if (n < 1 || base[n] > (int)kPmMaxTablePtrs) return false;
  // over 512 pointers (4 KB of kernel arguments) the kernel reads them from a table in device memory instead
  // (r06: C2's first path level is 106 jobs / ~600 pointers; as two kernels its second packet cost ~2.5 us)
  out.table = base[n] > (int)kPmMaxArgPtrs;
  for (int j = 0; j < n; ++j) {
    if (jobs[j].kind == 1) {
      const GatherK &g = jobs[j].g;
      if (g.nk < 0 || g.nk > KMAX || g.n_ev < 0 || g.n_ev > PGM_MAX_DIMS) return false;  // nk 0: one output
      continue;
    }
    if (jobs[j].kind == 2) {
      const ContractNK &c = jobs[j].n;
      if (c.n_ops < 1 || c.n_ops > MOPS || c.nk < 0 || c.nk > KMAX || c.nr < 0 || c.nr > KMAX) return false;
      continue;
    }
    const ContractK &k = jobs[j].k;
    if (k.n_split != 1 || (k.row_mode != 0 && k.row_mode != 2) || k.nk < 0 || k.nk > KMAX || k.nr > KMAX ||
        (k.row_mode == 2 && k.nk < 1))
      return false;
  }
  std::string &o = out.src;
  o = "#pragma clang fp contract(off)\n"  // products rounded before they are summed, as numpy does
      "typedef double pgm_d2 __attribute__((ext_vector_type(2)));\n"
      "__device__ __forceinline__ double pgm_div0(double a, double b) { const double r = a / b; "
      "return r != r ? 0.0 : r; }\n"
      "__device__ __forceinline__ double pgm_maxn(double a, double b) { return (a > b || a != a) ? a : b; }\n";
  for (int j = 0; j < n; ++j)
    o += jobs[j].kind == 1   ? cs_gather_body(jobs[j], "cj" + std::to_string(j))
         : jobs[j].kind == 2 ? cs_nary_body(jobs[j], "cj" + std::to_string(j))
                             : cs_job_body(jobs[j], "cj" + std::to_string(j));
  if (out.table)
    o += "struct pgm_pm_args { const double *const *__restrict__ p; };\n";
  else
    pgmi_appendf(o, "struct pgm_pm_args { const double *p[%d]; };\n", base[n]);
  // jobs [j0, j1) by block b through the tree of block-range comparisons: with a linear chain the
  // 130 / 87 / 64-job C2 levels ran 3-4x slower than the generic kernel; with the tree every level is
  // faster specialised, r05i: C2 0.148 ms/query with 24 jobs at most per specialised level, 0.129 with
  // no limit but the kernel-argument budget of 170 jobs
  auto call = [&](size_t j, const std::string &ind) {
    const pgmi_cs_job &J = jobs[j];
    const int p0 = base[j];
    if (J.kind == 1)
      pgmi_appendf(o, "%scj%zu((b - %uu) * 256u + lt, %uu, a.p[%d], (const unsigned char *)a.p[%d], (double *)a.p[%d], "
                      "(int *)a.p[%d]);\n", ind.c_str(), j, J.block0, J.nblocks * 256u, p0, p0 + 1, p0 + 2, p0 + 3);
    else if (J.kind == 2) {
      pgmi_appendf(o, "%scj%zu((b - %uu) * 256u + lt, %uu", ind.c_str(), j, J.block0, J.nblocks * 256u);
      for (int t = 0; t < J.n.n_ops; ++t) pgmi_appendf(o, ", a.p[%d]", p0 + t);
      pgmi_appendf(o, ", (double *)a.p[%d]);\n", p0 + J.n.n_ops);
    } else
      pgmi_appendf(o, "%scj%zu((b - %uu) * 256u + lt, %uu, a.p[%d], a.p[%d], (double *)a.p[%d]);\n", ind.c_str(), j,
                   J.block0, J.nblocks * 256u, p0, p0 + 1, p0 + 2);
  };
  auto dispatch = [&](int j0, int j1, const char *ind) {
    block_tree(o, (size_t)j0, (size_t)j1, ind, [&](size_t j) { return (unsigned long long)jobs[j].block0; }, call);
  };
  if (!one_wg) {
    uint64_t nb = 0;
    for (int j = 0; j < n; ++j) nb = std::max<uint64_t>(nb, (uint64_t)jobs[j].block0 + jobs[j].nblocks);
    if (nb == 0 || nb >= (1ull << 31)) return false;
    out.blocks = (unsigned)nb;
    o += "extern \"C\" __global__ void __launch_bounds__(256) pgm_pm(const pgm_pm_args a) {\n"
         "  const unsigned b = blockIdx.x, lt = threadIdx.x;\n";
    dispatch(0, n, "  ");
    o += "}\n";
  } else {
    // one 1,024-thread workgroup: each level's blocks four at a time (virtual 256-thread blocks), a
    // workgroup barrier after each level (the next level reads what this workgroup wrote)
    out.blocks = 1;
    out.threads = 1024;
    o += "extern \"C\" __global__ void __launch_bounds__(1024) pgm_pm(const pgm_pm_args a) {\n"
         "  const unsigned vb = threadIdx.x / 256u, lt = threadIdx.x % 256u;\n";
    int j = 0;
    for (int l = 0; l < n_levels; ++l) {
      const uint32_t b0 = level_off[l], b1 = level_off[l + 1];
      int j1 = j;
      while (j1 < n && jobs[j1].block0 < b1) ++j1;
      pgmi_appendf(o, "  for (unsigned b = %uu + vb; b < %uu; b += 4u) {\n", b0, b1);
      if (j1 > j) dispatch(j, j1, "    ");
      o += "  }\n  __syncthreads();\n";
      j = j1;
    }
    if (j != n) return false;  // jobs outside the level table: not a shape this form takes
    o += "}\n";
  }
  for (int q = 0; q < n; ++q) {
    const pgmi_cs_job &J = jobs[q];
    if (J.kind == 2) {
      out.ptrs.insert(out.ptrs.end(), J.ops, J.ops + J.n.n_ops);
      out.ptrs.push_back(J.C);
    } else if (J.kind == 1) {
      out.ptrs.insert(out.ptrs.end(), {J.A, (const double *)J.codes, J.C, (const double *)J.err});
    } else {
      out.ptrs.insert(out.ptrs.end(), {J.A, J.B, J.C});
    }
  }
  return true;
}

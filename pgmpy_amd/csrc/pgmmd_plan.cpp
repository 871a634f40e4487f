// pgmmd_plan.cpp — the host side of the mirror-descent fit of junction-tree potentials (include/pgmhip.h
// "Junction-tree potentials by mirror descent"): validation of the cliques, the tree and the marginals, the tree rooted
// at clique 0 with its depth levels, the separators with their strides on both sides, the owner of every marginal, the
// reduction jobs, projections and additions of every phase of a calibration with their item lists, the LDS layout,
// the tier and the argument checks of pgm_md_run.  No HIP call and no HIP include: ctypes drives all of it without a
// device.  The kernel and the launch are pgmmd.hip.
#include <algorithm>
#include <cmath>
#include <new>

#include "pgm_md.h"

namespace {

struct Scope {
  int32_t nv = 0;
  int32_t var[kMdMaxVars] = {}, card[kMdMaxVars] = {}, stride[kMdMaxVars] = {};  // C order: the last variable fastest
  int64_t size = 1;
  int32_t pos(int32_t v) const {
    for (int32_t k = 0; k < nv; ++k)
      if (var[k] == v) return k;
    return -1;
  }
};

int scope_read(const char *what, int32_t i, const int32_t *card, int32_t n_vars, int32_t nv, const int32_t *vars, Scope &s) {
  if (nv < 1 || nv > kMdMaxVars)
    return pgmi_failf(PGM_EINVAL, "md_plan_create: %s %d has %d variables (1 .. %d)", what, i, nv, kMdMaxVars);
  s = Scope();
  s.nv = nv;
  for (int32_t k = 0; k < nv; ++k) {
    if (vars[k] < 0 || vars[k] >= n_vars)
      return pgmi_failf(PGM_EINVAL, "md_plan_create: %s %d: variable %d is out of range (0 .. %d)", what, i, vars[k], n_vars - 1);
    for (int32_t m = 0; m < k; ++m)
      if (vars[m] == vars[k]) return pgmi_failf(PGM_EINVAL, "md_plan_create: %s %d lists variable %d twice", what, i, vars[k]);
    s.var[k] = vars[k], s.card[k] = card[vars[k]];
    if (s.size > (INT32_MAX / 2) / s.card[k])  // before the product: 254^8 is past int64, and the strides are int32
      return pgmi_failf(PGM_EINVAL, "md_plan_create: %s %d has more than 2^30 - 1 cells", what, i);
    s.size *= s.card[k];
  }
  for (int32_t k = nv - 1, st = 1; k >= 0; --k) s.stride[k] = st, st *= s.card[k];
  return PGM_OK;
}

// the reduction of `table` (at tab) onto `kept` (variables of the table, the output's C order), output at `out`
MdJob job_of(const Scope &table, int32_t tab, const Scope &kept, int32_t out) {
  MdJob j = {};
  j.tab = tab, j.out = out, j.n_out = (int32_t)kept.size, j.nk = kept.nv;
  for (int32_t k = 0; k < kept.nv; ++k)
    j.kc[k] = kept.card[k], j.ks[k] = kept.stride[k], j.kt[k] = table.stride[table.pos(kept.var[k])];
  Scope rest;
  rest.nv = 0;
  for (int32_t k = 0; k < table.nv; ++k)
    if (kept.pos(table.var[k]) < 0) rest.var[rest.nv] = table.var[k], rest.card[rest.nv] = table.card[k], ++rest.nv;
  int32_t st = 1;
  for (int32_t k = rest.nv - 1; k >= 0; --k) rest.stride[k] = st, st *= rest.card[k];
  j.n_res = st, j.nr = rest.nv;
  for (int32_t k = 0; k < rest.nv; ++k)
    j.rc[k] = rest.card[k], j.rs[k] = rest.stride[k], j.rt[k] = table.stride[table.pos(rest.var[k])];
  return j;
}

// a cell of `table` read as a cell of the array over `small` (variables of the table) at off
MdProj proj_of(const Scope &table, const Scope &small, int32_t off) {
  MdProj q = {};
  q.off = off, q.nv = small.nv;
  for (int32_t k = 0; k < small.nv; ++k)
    q.st[k] = table.stride[table.pos(small.var[k])], q.card[k] = small.card[k], q.ss[k] = small.stride[k];
  return q;
}

// a reduction phase over `jobs`: the cells of the jobs with a short residual, then the cells of the others
void reduce_phase(MdPlan &p, int32_t kind, const std::vector<int32_t> &jobs) {
  MdPhase ph = {};
  ph.kind = kind;
  for (int pass = 0; pass < 2; ++pass) {
    const int32_t first = (int32_t)p.items.size();
    for (int32_t j : jobs) {
      MdJob &J = p.jobs[(size_t)j];
      if ((J.n_res >= kMdWave) != (pass == 1)) continue;
      J.item0 = (int32_t)p.items.size();
      p.items.insert(p.items.end(), (size_t)J.n_out, j);
    }
    (pass ? ph.wave0 : ph.lane0) = first;
    (pass ? ph.wave_n : ph.lane_n) = (int32_t)p.items.size() - first;
  }
  p.phases.push_back(ph);
}

}  // namespace

int md_pick_tier(MdPlan &p, int32_t tier) {
  if (tier != PGM_MD_TIER_AUTO && tier != PGM_MD_TIER_LDS && tier != PGM_MD_TIER_GLOBAL)
    return pgmi_failf(PGM_EINVAL, "md_set_tier: tier %d (0 automatic, 1 LDS, 2 global)", tier);
  const int64_t lds = md_lds_bytes(PGM_MD_TIER_LDS, p.n_cells, p.n_sep, p.n_y);
  const int64_t glb = md_lds_bytes(PGM_MD_TIER_GLOBAL, p.n_cells, p.n_sep, p.n_y);
  if (tier == PGM_MD_TIER_LDS && lds > kMdLdsMax)
    return pgmi_failf(PGM_EINVAL, "md_set_tier: the state needs %lld bytes of LDS (%lld at most)", (long long)lds, (long long)kMdLdsMax);
  if (glb > kMdLdsMax)
    return pgmi_failf(PGM_EINVAL, "md_plan_create: the marginal vectors alone need %lld bytes of LDS (%lld at most)",
                      (long long)glb, (long long)kMdLdsMax);
  p.forced_tier = tier;
  p.tier = tier != PGM_MD_TIER_AUTO ? tier : lds <= kMdLdsMax ? PGM_MD_TIER_LDS : PGM_MD_TIER_GLOBAL;
  p.lds_bytes = p.tier == PGM_MD_TIER_LDS ? lds : glb;
  return PGM_OK;
}

int md_plan_build(const int32_t *card, int32_t n_vars, const int32_t *c_nvars, const int32_t *c_vars, int32_t n_cliques,
                  const int32_t *edges, int32_t n_edges, const int32_t *m_nvars, const int32_t *m_vars, int32_t n_marginals,
                  MdPlan &out) {
  if (n_vars < 1) return pgmi_failf(PGM_EINVAL, "md_plan_create: %d variables (1 at least)", n_vars);
  if (n_cliques < 1) return pgmi_failf(PGM_EINVAL, "md_plan_create: %d cliques (1 at least)", n_cliques);
  if (n_marginals < 1) return pgmi_failf(PGM_EINVAL, "md_plan_create: %d marginals (1 at least)", n_marginals);
  if (!card || !c_nvars || !c_vars || !m_nvars || !m_vars) return pgmi_failf(PGM_EINVAL, "md_plan_create: null card / cliques / marginals");
  if (n_edges != n_cliques - 1)
    return pgmi_failf(PGM_EINVAL, "md_plan_create: %d edges between %d cliques (a tree has %d)", n_edges, n_cliques, n_cliques - 1);
  if (n_edges && !edges) return pgmi_failf(PGM_EINVAL, "md_plan_create: null edges");
  for (int32_t v = 0; v < n_vars; ++v)
    if (card[v] < 1 || card[v] > kMdMaxCard)
      return pgmi_failf(PGM_EINVAL, "md_plan_create: variable %d has cardinality %d (1 .. %d)", v, card[v], kMdMaxCard);
  MdPlan p;
  p.n_vars = n_vars, p.n_cliques = n_cliques, p.n_edges = n_edges, p.n_marginals = n_marginals;

  std::vector<Scope> cl((size_t)n_cliques);
  for (int32_t c = 0; c < n_cliques; ++c) {
    if (const int st = scope_read("clique", c, card, n_vars, c_nvars[c], c_vars + (size_t)c * kMdMaxVars, cl[(size_t)c])) return st;
    p.clique_off.push_back((int32_t)p.n_cells);
    p.n_cells += cl[(size_t)c].size;
    if (2 * p.n_cells > INT32_MAX)
      return pgmi_failf(PGM_EINVAL, "md_plan_create: the tables up to clique %d have %lld cells (2^30 - 1 at most)", c, (long long)p.n_cells);
  }
  p.clique_off.push_back((int32_t)p.n_cells);

  // the tree rooted at clique 0: breadth first, the neighbours of a clique in the order of the edge list
  std::vector<std::vector<int32_t>> nbr((size_t)n_cliques);
  for (int32_t e = 0; e < n_edges; ++e) {
    const int32_t a = edges[2 * e], b = edges[2 * e + 1];
    if (a < 0 || a >= n_cliques || b < 0 || b >= n_cliques || a == b)
      return pgmi_failf(PGM_EINVAL, "md_plan_create: edge %d joins cliques %d and %d (two of 0 .. %d)", e, a, b, n_cliques - 1);
    nbr[(size_t)a].push_back(b), nbr[(size_t)b].push_back(a);
  }
  p.parent.assign((size_t)n_cliques, -1), p.level.assign((size_t)n_cliques, -1);
  std::vector<int32_t> order = {0};
  p.level[0] = 0;
  for (size_t i = 0; i < order.size(); ++i)
    for (int32_t k : nbr[(size_t)order[i]])
      if (p.level[(size_t)k] < 0) {
        p.level[(size_t)k] = p.level[(size_t)order[i]] + 1, p.parent[(size_t)k] = order[i];
        p.depth = std::max(p.depth, p.level[(size_t)k]);
        order.push_back(k);
      }
  if ((int32_t)order.size() != n_cliques)
    return pgmi_failf(PGM_EINVAL, "md_plan_create: the edges reach %d of the %d cliques from clique 0 (not a tree)", (int)order.size(), n_cliques);

  // the separator of a clique and its parent: the shared variables in the child's order
  std::vector<Scope> sep((size_t)n_cliques);
  for (int32_t c = 0; c < n_cliques; ++c) {
    p.sep_off.push_back((int32_t)p.n_sep);
    if (c == 0) continue;
    const Scope &C = cl[(size_t)c], &P = cl[(size_t)p.parent[(size_t)c]];
    Scope &S = sep[(size_t)c];
    S.nv = 0;
    for (int32_t k = 0; k < C.nv; ++k)
      if (P.pos(C.var[k]) >= 0) S.var[S.nv] = C.var[k], S.card[S.nv] = C.card[k], S.size *= C.card[k], ++S.nv;
    for (int32_t k = S.nv - 1, st = 1; k >= 0; --k) S.stride[k] = st, st *= S.card[k];
    p.n_sep += S.size;
  }
  p.sep_off.push_back((int32_t)p.n_sep);
  p.state_len = 2 * (p.n_cells + p.n_sep);
  if (p.state_len > INT32_MAX)
    return pgmi_failf(PGM_EINVAL, "md_plan_create: the state of an instance has %lld cells (2^31 - 1 at most)", (long long)p.state_len);

  // the marginals: each belongs to the first clique that holds its scope
  std::vector<Scope> mg((size_t)n_marginals);
  for (int32_t j = 0; j < n_marginals; ++j) {
    Scope &M = mg[(size_t)j];
    if (const int st = scope_read("marginal", j, card, n_vars, m_nvars[j], m_vars + (size_t)j * kMdMaxVars, M)) return st;
    int32_t own = -1;
    for (int32_t c = 0; c < n_cliques && own < 0; ++c) {
      bool all = true;
      for (int32_t k = 0; k < M.nv; ++k) all = all && cl[(size_t)c].pos(M.var[k]) >= 0;
      if (all) own = c;
    }
    if (own < 0) return pgmi_failf(PGM_EINVAL, "md_plan_create: no clique holds the scope of marginal %d", j);
    p.owner.push_back(own), p.y_off.push_back((int32_t)p.n_y);
    p.n_y += M.size;
  }
  p.y_off.push_back((int32_t)p.n_y);
  if (const int st = md_pick_tier(p, PGM_MD_TIER_AUTO)) return st;

  // jobs: up of clique c at c - 1, down of clique c at n_cliques - 1 + c - 1, marginal j at 2 (n_cliques - 1) + j
  for (int32_t c = 1; c < n_cliques; ++c) p.jobs.push_back(job_of(cl[(size_t)c], p.clique_off[(size_t)c], sep[(size_t)c], p.sep_off[(size_t)c]));
  for (int32_t c = 1; c < n_cliques; ++c) {
    const int32_t par = p.parent[(size_t)c];
    p.jobs.push_back(job_of(cl[(size_t)par], p.clique_off[(size_t)par], sep[(size_t)c], p.sep_off[(size_t)c]));
  }
  for (int32_t j = 0; j < n_marginals; ++j) {
    const int32_t c = p.owner[(size_t)j];
    p.jobs.push_back(job_of(cl[(size_t)c], p.clique_off[(size_t)c], mg[(size_t)j], p.y_off[(size_t)j]));
  }
  const int32_t up0 = -1, dn0 = n_cliques - 2, mg0 = 2 * (n_cliques - 1);  // job of clique c: up0 + c, dn0 + c

  // the gradient gather of every clique: its marginals in their order
  auto add_open = [&](int32_t c) { p.adds.push_back(MdAdd{p.clique_off[(size_t)c], (int32_t)cl[(size_t)c].size, (int32_t)p.projs.size(), 0}); };
  auto add_close = [&]() { p.adds.back().p1 = (int32_t)p.projs.size(); };
  for (int32_t c = 0; c < n_cliques; ++c) {
    add_open(c);
    for (int32_t j = 0; j < n_marginals; ++j)
      if (p.owner[(size_t)j] == c) p.projs.push_back(proj_of(cl[(size_t)c], mg[(size_t)j], p.y_off[(size_t)j]));
    add_close();
  }

  // the phases of a calibration: up from the deepest level, log Z at the root, down to the deepest level, the marginals
  std::vector<int32_t> list;
  for (int32_t L = p.depth; L >= 1; --L) {
    list.clear();
    for (int32_t c = 0; c < n_cliques; ++c)
      if (p.level[(size_t)c] == L) list.push_back(up0 + c);
    reduce_phase(p, kMdUp, list);
    MdPhase ph = {};
    ph.kind = kMdAddUp, ph.a0 = (int32_t)p.adds.size();
    for (int32_t par = 0; par < n_cliques; ++par) {
      if (p.level[(size_t)par] != L - 1) continue;
      add_open(par);
      for (int32_t c = 1; c < n_cliques; ++c)
        if (p.parent[(size_t)c] == par) p.projs.push_back(proj_of(cl[(size_t)par], sep[(size_t)c], p.sep_off[(size_t)c]));
      add_close();
      if (p.adds.back().p0 == p.adds.back().p1) p.adds.pop_back();  // a leaf of this level
    }
    ph.a1 = (int32_t)p.adds.size();
    p.phases.push_back(ph);
  }
  MdPhase logz = {};
  logz.kind = kMdLogZ;
  p.phases.push_back(logz);
  p.root_tab = p.clique_off[0], p.root_size = (int32_t)cl[0].size;
  for (int32_t L = 0; L < p.depth; ++L) {
    list.clear();
    for (int32_t c = 1; c < n_cliques; ++c)
      if (p.level[(size_t)c] == L + 1) list.push_back(dn0 + c);
    reduce_phase(p, kMdDown, list);
    MdPhase ph = {};
    ph.kind = kMdAddDown, ph.a0 = (int32_t)p.adds.size();
    for (int32_t c = 1; c < n_cliques; ++c) {
      if (p.level[(size_t)c] != L + 1) continue;
      add_open(c);
      p.projs.push_back(proj_of(cl[(size_t)c], sep[(size_t)c], p.sep_off[(size_t)c]));
      add_close();
    }
    ph.a1 = (int32_t)p.adds.size();
    p.phases.push_back(ph);
  }
  list.clear();
  for (int32_t j = 0; j < n_marginals; ++j) list.push_back(mg0 + j);
  reduce_phase(p, kMdMarg, list);
  out = std::move(p);
  return PGM_OK;
}

int md_run_check(const MdHandle *h, const double *targets, const double *totals, const double *theta_in, int64_t theta_rows,
                 int64_t n_rows, int32_t metric, int32_t iterations, double stepsize, int32_t step_mode, const double *scratch,
                 const double *theta_out, const double *mu_out, const double *values, const int32_t *trials, bool *launch) {
  *launch = false;
  if (!h) return pgmi_failf(PGM_EINVAL, "md_run: null plan");
  if (!targets || !totals || !theta_in) return pgmi_failf(PGM_EINVAL, "md_run: null targets / totals / theta_in");
  if (!theta_out || !mu_out || !values || !trials) return pgmi_failf(PGM_EINVAL, "md_run: null theta_out / mu_out / values / trials");
  if (n_rows < 0 || n_rows > INT32_MAX) return pgmi_failf(PGM_EINVAL, "md_run: %lld instances (0 .. 2^31 - 1)", (long long)n_rows);
  if (theta_rows != 1 && theta_rows != n_rows)
    return pgmi_failf(PGM_EINVAL, "md_run: theta_in has %lld rows (1 or %lld)", (long long)theta_rows, (long long)n_rows);
  if (metric != PGM_MD_L1 && metric != PGM_MD_L2) return pgmi_failf(PGM_EINVAL, "md_run: metric %d (1: L1, 2: L2)", metric);
  if (iterations < 0) return pgmi_failf(PGM_EINVAL, "md_run: %d iterations", iterations);
  if (step_mode != PGM_MD_STEP_FIXED && step_mode != PGM_MD_STEP_SEARCH && step_mode != PGM_MD_STEP_DEFAULT)
    return pgmi_failf(PGM_EINVAL, "md_run: step mode %d (0 fixed, 1 line search, 2 fixed at 1 / total^2)", step_mode);
  if (step_mode == PGM_MD_STEP_FIXED && !std::isfinite(stepsize)) return pgmi_failf(PGM_EINVAL, "md_run: step size %g (finite)", stepsize);
  if (h->p.tier == PGM_MD_TIER_GLOBAL && !scratch)
    return pgmi_failf(PGM_EINVAL, "md_run: the global tier needs a scratch slab of %lld fp64 per instance", (long long)h->p.state_len);
  const void *f64[] = {targets, totals, theta_in, scratch, theta_out, mu_out, values};
  for (const void *q : f64)
    if ((uintptr_t)q % 8) return pgmi_failf(PGM_EINVAL, "md_run: an fp64 pointer is not 8-byte aligned");
  if ((uintptr_t)trials % 4) return pgmi_failf(PGM_EINVAL, "md_run: trials is not 4-byte aligned");
  *launch = n_rows > 0;
  return PGM_OK;
}

extern "C" {

int pgm_md_plan_create(const int32_t *card, int32_t n_vars, const int32_t *clique_nvars, const int32_t *clique_vars,
                       int32_t n_cliques, const int32_t *edges, int32_t n_edges, const int32_t *marginal_nvars,
                       const int32_t *marginal_vars, int32_t n_marginals, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "md_plan_create: null plan");
  *plan = nullptr;
  MdHandle *h = new (std::nothrow) MdHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "md_plan_create: out of memory");
  int st;
  try {
    st = md_plan_build(card, n_vars, clique_nvars, clique_vars, n_cliques, edges, n_edges, marginal_nvars, marginal_vars, n_marginals, h->p);
  } catch (const std::bad_alloc &) {  // the item list holds one int32 per separator and marginal cell
    st = pgmi_failf(PGM_ENOMEM, "md_plan_create: out of memory");
  }
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_md_set_tier(void *plan, int32_t tier) {
  MdHandle *h = static_cast<MdHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "md_set_tier: null plan");
  return md_pick_tier(h->p, tier);
}

int pgm_md_plan_info(void *plan, pgm_md_info_t *info, int32_t *clique_off, int32_t *parent, int32_t *level, int32_t *sep_off,
                     int32_t *sep_strides, int32_t *owner, int32_t *y_off, int32_t *marginal_strides) {
  const MdHandle *h = static_cast<const MdHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "md_plan_info: null plan");
  const MdPlan &p = h->p;
  if (info) {
    info->n_vars = p.n_vars, info->n_cliques = p.n_cliques, info->n_edges = p.n_edges, info->n_marginals = p.n_marginals;
    info->depth = p.depth, info->tier = p.tier, info->block = kMdBlock, info->n_phases = (int32_t)p.phases.size();
    info->n_cells = p.n_cells, info->n_sep = p.n_sep, info->n_y = p.n_y, info->state_len = p.state_len;
    info->scratch_len = p.tier == PGM_MD_TIER_GLOBAL ? p.state_len : 0;
    info->lds_bytes = p.lds_bytes, info->lds_max = kMdLdsMax;
  }
  if (clique_off) std::copy(p.clique_off.begin(), p.clique_off.end(), clique_off);
  if (parent) std::copy(p.parent.begin(), p.parent.end(), parent);
  if (level) std::copy(p.level.begin(), p.level.end(), level);
  if (sep_off) std::copy(p.sep_off.begin(), p.sep_off.end(), sep_off);
  if (owner) std::copy(p.owner.begin(), p.owner.end(), owner);
  if (y_off) std::copy(p.y_off.begin(), p.y_off.end(), y_off);
  const int32_t nc = p.n_cliques;
  if (sep_strides) {  // [n_cliques][2][PGM_MD_MAX_VARS]: in the child's table, in the parent's; 0 past the separator
    std::fill(sep_strides, sep_strides + (size_t)nc * 2 * kMdMaxVars, 0);
    for (int32_t c = 1; c < nc; ++c) {
      const MdJob &U = p.jobs[(size_t)(c - 1)], &D = p.jobs[(size_t)(nc - 2 + c)];
      std::copy(U.kt, U.kt + U.nk, sep_strides + (size_t)c * 2 * kMdMaxVars);
      std::copy(D.kt, D.kt + D.nk, sep_strides + (size_t)c * 2 * kMdMaxVars + kMdMaxVars);
    }
  }
  if (marginal_strides) {  // [n_marginals][PGM_MD_MAX_VARS]: in the owner's table
    std::fill(marginal_strides, marginal_strides + (size_t)p.n_marginals * kMdMaxVars, 0);
    for (int32_t j = 0; j < p.n_marginals; ++j) {
      const MdJob &M = p.jobs[(size_t)(2 * (nc - 1) + j)];
      std::copy(M.kt, M.kt + M.nk, marginal_strides + (size_t)j * kMdMaxVars);
    }
  }
  return PGM_OK;
}
}

// pgmdbn_pf_plan.cpp — the host side of the dynamic-network particle filter (include/pgmhip.h "dynamic Bayesian
// networks: the particle filter"): validation of the slice nodes and the two family sets, the plan order of each
// set, the interface, the family descriptors the kernel reads, the LDS geometry and the argument checks of
// pgm_dbn_pf_run and pgm_dbn_pf_trace.  No HIP call and no HIP include: ctypes drives all of it without a
// device.  The kernels and the launches are pgmdbn_pf.hip.
#include <algorithm>
#include <new>

#include "pgm_dbn_pf.h"

static bool pf_pow2_in_range(int32_t N) {
  return N >= PGM_DBN_PF_MIN_PARTICLES && N <= PGM_DBN_PF_MAX_PARTICLES && (N & (N - 1)) == 0;
}

int pf_plan_build(const int32_t *card, const uint8_t *queried, int32_t n, const pgm_fit_family *fam0, int32_t n_fam0,
                  const pgm_fit_family *fam1, int32_t n_fam1, PfPlan &out) {
  if (n < 1 || n > kPfMaxNodes) return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %d slice nodes (1 .. %d)", n, kPfMaxNodes);
  if (!card) return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: null card");
  if (!fam0 || !fam1) return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: null families");
  if (n_fam0 < 0 || n_fam1 < 0) return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %d / %d families", n_fam0, n_fam1);
  for (int32_t v = 0; v < n; ++v)
    if (card[v] < 1 || card[v] > kPfMaxCard)
      return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: node %d has cardinality %d (1 .. %d)", v, card[v], kPfMaxCard);

  // the families: columns, cardinalities, one per node and set (the rules of pgm_dbn_plan_create)
  const pgm_fit_family *fams[2] = {fam0, fam1};
  const int32_t n_fams[2] = {n_fam0, n_fam1};
  const char *names[2] = {"slice-0", "transition"};
  std::vector<int32_t> fam_of[2];
  std::vector<int64_t> size[2];
  PfPlan p;
  p.n = n;
  for (int k = 0; k < 2; ++k) {
    const char *what = names[k];
    const int32_t lo = k ? n : 0, hi = k ? 2 * n : n;
    fam_of[k].assign((size_t)n, -1);
    for (int32_t f = 0; f < n_fams[k]; ++f) {
      const pgm_fit_family &F = fams[k][f];
      if (F.n_vars < 1 || F.n_vars > PGM_MAX_DIMS)
        return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %s family %d has %d variables (1 .. %d)", what, f, F.n_vars,
                          PGM_MAX_DIMS);
      if (F.col[0] < lo || F.col[0] >= hi)
        return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %s family %d: node column %d is out of range (%d .. %d)", what, f,
                          F.col[0], lo, hi - 1);
      int64_t sz = 1;
      for (int32_t j = 0; j < F.n_vars; ++j) {
        const int32_t c = F.col[j];
        if (c < 0 || c >= hi)
          return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %s family %d: column %d is out of range (0 .. %d)", what, f, c,
                            hi - 1);
        for (int32_t m = 0; m < j; ++m)
          if (F.col[m] == c)
            return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %s family %d lists column %d twice", what, f, c);
        if (F.card[j] != card[c % n])
          return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %s family %d gives column %d cardinality %d, node %d has %d", what,
                            f, c, F.card[j], c % n, card[c % n]);
        sz *= F.card[j];
        if (sz > INT32_MAX)
          return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %s family %d has 2^31 table entries or more", what, f);
      }
      const int32_t v = F.col[0] - lo;
      if (fam_of[k][(size_t)v] >= 0)
        return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: node %d has two %s families (%d and %d)", v, what,
                          fam_of[k][(size_t)v], f);
      fam_of[k][(size_t)v] = f;
      p.off[k].push_back(p.total[k]);
      size[k].push_back(sz);
      p.total[k] += sz;
      if (p.total[k] > INT32_MAX)
        return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: the %s tables have 2^31 entries or more", what);
    }
    for (int32_t v = 0; v < n; ++v)
      if (fam_of[k][(size_t)v] < 0) return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: node %d has no %s family", v, what);
  }

  // the interface: nodes with a child in the next slice, in node order
  std::vector<int32_t> iface_at((size_t)n, -1), iface;
  for (int32_t f = 0; f < n_fam1; ++f)
    for (int32_t j = 1; j < fam1[f].n_vars; ++j)
      if (fam1[f].col[j] < n) iface_at[(size_t)fam1[f].col[j]] = 0;
  for (int32_t v = 0; v < n; ++v)
    if (iface_at[(size_t)v] == 0) {
      iface_at[(size_t)v] = (int32_t)iface.size();
      iface.push_back(v);
    }
  p.n_iface = (int32_t)iface.size();

  // the plan order of a set: Kahn over the set's intra-slice edges, the lowest ready node first
  for (int k = 0; k < 2; ++k) {
    const int32_t base = k ? n : 0;
    std::vector<uint8_t> done((size_t)n, 0);
    for (int32_t step = 0; step < n; ++step) {
      int32_t pick = -1;
      for (int32_t v = 0; v < n && pick < 0; ++v) {
        if (done[(size_t)v]) continue;
        const pgm_fit_family &F = fams[k][(size_t)fam_of[k][(size_t)v]];
        bool ready = true;
        for (int32_t j = 1; j < F.n_vars; ++j)
          if (F.col[j] >= base && F.col[j] < base + n && !done[(size_t)(F.col[j] - base)]) ready = false;
        if (ready) pick = v;
      }
      if (pick < 0) return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: the %s families have a cycle within the slice", names[k]);
      done[(size_t)pick] = 1;
      p.order[k].push_back(pick);
    }
  }

  // the descriptors, in plan order
  for (int k = 0; k < 2; ++k) {
    int64_t cols = 0;
    for (int32_t v : p.order[k]) {
      const size_t given = (size_t)fam_of[k][(size_t)v];
      const pgm_fit_family &F = fams[k][given];
      PfFam D = {};
      D.node = v, D.card = F.card[0], D.n_par = F.n_vars - 1;
      D.ncol = (int32_t)(size[k][given] / F.card[0]);
      D.off = (int32_t)p.off[k][given];
      int32_t stride = D.ncol;
      for (int32_t j = 1; j < F.n_vars; ++j) {
        stride /= F.card[j];  // C order: the last parent fastest
        const int32_t c = F.col[j];
        D.src[j - 1] = (k == 1 && c < n) ? n + iface_at[(size_t)c] : c % n;
        D.stride[j - 1] = stride;
      }
      p.fams.push_back(D);
      p.col_off.push_back(cols);
      cols += D.ncol;
    }
    p.col_off.push_back(cols);
  }

  std::vector<int32_t> qnode, qoff;
  for (int32_t v = 0; v < n; ++v)
    if (queried && queried[v]) {
      qnode.push_back(v), qoff.push_back(p.bins);
      p.bins += card[v];
    }
  p.n_qnodes = (int32_t)qnode.size();
  auto put = [&](const std::vector<int32_t> &v) {
    const int32_t at = (int32_t)p.tab.size();
    p.tab.insert(p.tab.end(), v.begin(), v.end());
    return at;
  };
  p.o_card = put(std::vector<int32_t>(card, card + n));
  p.o_iface = put(iface);
  p.o_qnode = put(qnode);
  p.o_qoff = put(qoff);
  if (pf_max_particles(p) == 0)
    return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: %lld bytes of LDS for %d particles, %lld at most",
                      (long long)pf_lds_bytes(n, p.n_iface, p.bins, PGM_DBN_PF_MIN_PARTICLES), PGM_DBN_PF_MIN_PARTICLES,
                      (long long)kPfLdsMax);
  out = std::move(p);
  return PGM_OK;
}

static int pf_particles_check(const char *who, const PfPlan &p, int32_t N, bool fit) {
  if (!pf_pow2_in_range(N))
    return pgmi_failf(PGM_EINVAL, "%s: %d particles per sequence (a power of two, %d .. %d)", who, N, PGM_DBN_PF_MIN_PARTICLES,
                      PGM_DBN_PF_MAX_PARTICLES);
  if (fit && pf_lds_bytes(p.n, p.n_iface, p.bins, N) > kPfLdsMax)
    return pgmi_failf(PGM_EINVAL, "%s: %d particles per sequence need %lld bytes of LDS (%lld at most): the largest that fits is %d",
                      who, N, (long long)pf_lds_bytes(p.n, p.n_iface, p.bins, N), (long long)kPfLdsMax, pf_max_particles(p));
  return PGM_OK;
}

int pf_run_check(const PfHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                 int32_t n_slices, const double *values0, const double *values1, int32_t n_particles, int64_t first_row,
                 const double *filter, const double *loglik, const double *ess, const uint16_t *ancestors, const uint8_t *traj,
                 bool *launch) {
  *launch = false;
  if (!h) return pgmi_failf(PGM_EINVAL, "dbn_pf_run: null plan");
  const PfPlan &p = h->p;
  if (!codes || !values0 || !values1) return pgmi_failf(PGM_EINVAL, "dbn_pf_run: null codes / values");
  if (n_slices < 1 || n_slices > kPfMaxSlices)
    return pgmi_failf(PGM_EINVAL, "dbn_pf_run: %d slices (1 .. %d)", n_slices, kPfMaxSlices);
  if ((int64_t)n_cols != (int64_t)n_slices * p.n)
    return pgmi_failf(PGM_EINVAL, "dbn_pf_run: %d code columns, %d slices of %d nodes need %lld", n_cols, n_slices, p.n,
                      (long long)n_slices * p.n);
  if (ld < 0 || row0 < 0 || n_rows < 0 || n_rows > ld || row0 > ld - n_rows)
    return pgmi_failf(PGM_EINVAL, "dbn_pf_run: rows [%lld, %lld + %lld) are outside ld %lld", (long long)row0, (long long)row0,
                      (long long)n_rows, (long long)ld);
  const int st = pf_particles_check("dbn_pf_run", p, n_particles, true);
  if (st != PGM_OK) return st;
  if (first_row < 0) return pgmi_failf(PGM_EINVAL, "dbn_pf_run: first_row %lld is negative", (long long)first_row);
  const void *f64[] = {values0, values1, filter, loglik, ess};
  for (const void *q : f64)
    if ((uintptr_t)q % 8) return pgmi_failf(PGM_EINVAL, "dbn_pf_run: an fp64 pointer is not 8-byte aligned");
  if ((uintptr_t)ancestors % 2) return pgmi_failf(PGM_EINVAL, "dbn_pf_run: ancestors is not 2-byte aligned");
  if (traj && !ancestors) return pgmi_failf(PGM_EINVAL, "dbn_pf_run: traj without ancestors");
  if (n_rows > INT32_MAX) return pgmi_failf(PGM_EINVAL, "dbn_pf_run: %lld sequences in one call (2^31 - 1 at most)", (long long)n_rows);
  *launch = n_rows > 0;
  return PGM_OK;
}

int pf_trace_check(const PfHandle *h, const uint16_t *ancestors, const uint8_t *traj, int64_t n_rows, int32_t n_slices,
                   int32_t n_particles, const uint8_t *out, int64_t ld_out, int64_t row0_out, bool *launch) {
  *launch = false;
  if (!h) return pgmi_failf(PGM_EINVAL, "dbn_pf_trace: null plan");
  if (!ancestors || !traj || !out) return pgmi_failf(PGM_EINVAL, "dbn_pf_trace: null ancestors / traj / out");
  if ((uintptr_t)ancestors % 2) return pgmi_failf(PGM_EINVAL, "dbn_pf_trace: ancestors is not 2-byte aligned");
  if (n_slices < 1 || n_slices > kPfMaxSlices)
    return pgmi_failf(PGM_EINVAL, "dbn_pf_trace: %d slices (1 .. %d)", n_slices, kPfMaxSlices);
  const int st = pf_particles_check("dbn_pf_trace", h->p, n_particles, false);
  if (st != PGM_OK) return st;
  // one work-item per final particle, 256 to a workgroup: the grid holds 2^31 - 1 workgroups
  if (n_rows < 0 || n_rows > INT32_MAX / 16)
    return pgmi_failf(PGM_EINVAL, "dbn_pf_trace: %lld sequences (0 .. %d)", (long long)n_rows, INT32_MAX / 16);
  const int64_t need = n_rows * n_particles;
  if (ld_out < 0 || row0_out < 0 || need > ld_out || row0_out > ld_out - need)
    return pgmi_failf(PGM_EINVAL, "dbn_pf_trace: rows [%lld, %lld + %lld) are outside ld_out %lld", (long long)row0_out,
                      (long long)row0_out, (long long)need, (long long)ld_out);
  *launch = n_rows > 0 && h->p.n_qnodes > 0;
  return PGM_OK;
}

extern "C" {

int pgm_dbn_pf_plan_create(const int32_t *card, const uint8_t *queried, int32_t n, const pgm_fit_family *families0,
                           int32_t n_families0, const pgm_fit_family *families1, int32_t n_families1, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_create: null plan");
  *plan = nullptr;
  PfHandle *h = new (std::nothrow) PfHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "dbn_pf_plan_create: out of memory");
  const int st = pf_plan_build(card, queried, n, families0, n_families0, families1, n_families1, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_dbn_pf_plan_info(void *plan, int32_t n_particles, pgm_dbn_pf_info_t *info, int32_t *order0, int32_t *order1,
                         int64_t *off0, int64_t *off1) {
  const PfHandle *h = static_cast<const PfHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "dbn_pf_plan_info: null plan");
  const PfPlan &p = h->p;
  const int st = pf_particles_check("dbn_pf_plan_info", p, n_particles, false);
  if (st != PGM_OK) return st;
  if (info) {
    info->n = p.n;
    info->n_interface = p.n_iface;
    info->n_query_nodes = p.n_qnodes;
    info->n_query = p.bins;
    info->block = std::min<int32_t>(n_particles, kPfMaxBlock);
    info->max_particles = pf_max_particles(p);
    info->lds_bytes = pf_lds_bytes(p.n, p.n_iface, p.bins, n_particles);
    info->values0 = p.total[0];
    info->values1 = p.total[1];
  }
  if (order0) std::copy(p.order[0].begin(), p.order[0].end(), order0);
  if (order1) std::copy(p.order[1].begin(), p.order[1].end(), order1);
  if (off0) std::copy(p.off[0].begin(), p.off[0].end(), off0);
  if (off1) std::copy(p.off[1].begin(), p.off[1].end(), off1);
  return PGM_OK;
}
}

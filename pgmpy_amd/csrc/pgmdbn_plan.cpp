// pgmdbn_plan.cpp — the host side of the dynamic-network filter (include/pgmhip.h "dynamic Bayesian
// networks"): validation of the slice nodes and the two family sets, the offset tables the kernel reads, the
// launch geometry and the argument checks of pgm_dbn_run, pgm_dbn_viterbi and pgm_dbn_estep.  No HIP call and no HIP include:
// ctypes drives all of it without a device.  The kernels and the launches are pgmdbn.hip.
#include <algorithm>
#include <new>

#include "pgm_dbn.h"

static int32_t tab_put(std::vector<int32_t> &tab, const std::vector<int32_t> &v) {
  const int32_t at = (int32_t)tab.size();
  tab.insert(tab.end(), v.begin(), v.end());
  return at;
}

int dbn_plan_build(const int32_t *card, const uint8_t *clamped, const uint8_t *queried, int32_t n, const pgm_fit_family *fam0,
                   int32_t n_fam0, const pgm_fit_family *fam1, int32_t n_fam1, DbnPlan &out) {
  if (n < 1 || n > kDbnMaxNodes) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %d slice nodes (1 .. %d)", n, kDbnMaxNodes);
  if (!card || !clamped) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: null card / clamped");
  if (!fam0 || !fam1) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: null families");
  if (n_fam0 < 0 || n_fam1 < 0) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %d / %d families", n_fam0, n_fam1);
  for (int32_t v = 0; v < n; ++v)
    if (card[v] < 1 || card[v] > 255)
      return pgmi_failf(PGM_EINVAL, "dbn_plan_create: node %d has cardinality %d (1 .. 255)", v, card[v]);

  // the joint of the free nodes, the last fastest
  std::vector<int32_t> xstride((size_t)n, 0), free_nodes;
  int64_t J = 1;
  for (int32_t v = n - 1; v >= 0; --v) {
    if (clamped[v]) continue;
    xstride[(size_t)v] = (int32_t)J;
    J *= card[v];
    if (J > kDbnMaxConfigs)
      return pgmi_failf(PGM_EINVAL, "dbn_plan_create: the free nodes have more than %d joint states", kDbnMaxConfigs);
  }
  for (int32_t v = 0; v < n; ++v)
    if (!clamped[v]) free_nodes.push_back(v);

  // the families: columns, cardinalities, one per node and set
  const pgm_fit_family *fams[2] = {fam0, fam1};
  const int32_t n_fams[2] = {n_fam0, n_fam1};
  const char *names[2] = {"slice-0", "transition"};
  std::vector<int32_t> fam_of[2];
  DbnPlan p;
  for (int k = 0; k < 2; ++k) {
    const char *what = names[k];
    const int32_t lo = k ? n : 0, hi = k ? 2 * n : n;
    fam_of[k].assign((size_t)n, -1);
    for (int32_t f = 0; f < n_fams[k]; ++f) {
      const pgm_fit_family &F = fams[k][f];
      if (F.n_vars < 1 || F.n_vars > PGM_MAX_DIMS)
        return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %s family %d has %d variables (1 .. %d)", what, f, F.n_vars, PGM_MAX_DIMS);
      if (F.col[0] < lo || F.col[0] >= hi)
        return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %s family %d: node column %d is out of range (%d .. %d)", what, f, F.col[0],
                          lo, hi - 1);
      int64_t size = 1;
      for (int32_t j = 0; j < F.n_vars; ++j) {
        const int32_t c = F.col[j];
        if (c < 0 || c >= hi)
          return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %s family %d: column %d is out of range (0 .. %d)", what, f, c, hi - 1);
        for (int32_t m = 0; m < j; ++m)
          if (F.col[m] == c) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %s family %d lists column %d twice", what, f, c);
        if (F.card[j] != card[c % n])
          return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %s family %d gives column %d cardinality %d, node %d has %d", what, f, c,
                            F.card[j], c % n, card[c % n]);
        if (k && c < n && fam_of[0][(size_t)c] < 0)
          return pgmi_failf(PGM_EINVAL, "dbn_plan_create: transition family %d: its slice-t parent, column %d, has no slice-0 family",
                            f, c);
        size *= F.card[j];
        if (size > INT32_MAX) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %s family %d has 2^31 table entries or more", what, f);
      }
      const int32_t v = F.col[0] - lo;
      if (fam_of[k][(size_t)v] >= 0)
        return pgmi_failf(PGM_EINVAL, "dbn_plan_create: node %d has two %s families (%d and %d)", v, what, fam_of[k][(size_t)v], f);
      fam_of[k][(size_t)v] = f;
      p.off[k].push_back(p.total[k]);
      p.size[k].push_back(size);
      p.total[k] += size;
      if (p.total[k] > INT32_MAX) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: the %s tables have 2^31 entries or more", what);
    }
  }
  for (int k = 0; k < 2; ++k)
    for (int32_t v = 0; v < n; ++v)
      if (fam_of[k][(size_t)v] < 0) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: node %d has no %s family", v, names[k]);

  // the interface: free nodes that are a slice-t parent of a transition family; its joint, the last fastest
  std::vector<uint8_t> is_iface((size_t)n, 0);
  for (int32_t f = 0; f < n; ++f)
    for (int32_t j = 1; j < fam1[f].n_vars; ++j)
      if (fam1[f].col[j] < n && !clamped[fam1[f].col[j]]) is_iface[(size_t)fam1[f].col[j]] = 1;
  std::vector<int32_t> istride((size_t)n, 0);
  int64_t S = 1;
  for (int32_t v = n - 1; v >= 0; --v)
    if (is_iface[(size_t)v]) {
      istride[(size_t)v] = (int32_t)S;
      S *= card[v];
    }
  const int32_t Ji = (int32_t)J, Si = (int32_t)S, R = Ji / Si;
  auto digit = [&](int32_t x, int32_t v) { return x / xstride[(size_t)v] % card[v]; };
  std::vector<int32_t> ix((size_t)Ji), xperm((size_t)Ji), fill((size_t)Si, 0);
  for (int32_t x = 0; x < Ji; ++x) {
    int32_t i = 0;
    for (int32_t v : free_nodes)
      if (is_iface[(size_t)v]) i += digit(x, v) * istride[(size_t)v];
    ix[(size_t)x] = i;
    xperm[(size_t)i * R + fill[(size_t)i]++] = x;
  }

  DbnLayout &L = p.L;
  L.n = n, L.J = Ji, L.S = Si, L.R = R, L.n_free = (int32_t)free_nodes.size();
  int32_t P = 1;
  while (P < Ji && P < kDbnBlock) P *= 2;
  L.P = P;
  L.spw = kDbnBlock / P;
  while (L.spw > 1 && dbn_lds_bytes(L.spw, n, Ji, Si) > kDbnLdsMax) --L.spw;
  p.lds_bytes = dbn_lds_bytes(L.spw, n, Ji, Si);
  if (p.lds_bytes > kDbnLdsMax) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: %lld bytes of LDS per sequence", (long long)p.lds_bytes);

  std::vector<int32_t> &tab = p.tab;
  L.o_card = tab_put(tab, std::vector<int32_t>(card, card + n));
  L.o_clamp = tab_put(tab, std::vector<int32_t>(clamped, clamped + n));
  L.o_xstride = tab_put(tab, xstride);
  L.o_free = tab_put(tab, free_nodes);
  L.o_ix = tab_put(tab, ix);
  L.o_xperm = tab_put(tab, xperm);

  std::vector<int32_t> cur, prev, ioff;
  for (int k = 0; k < 2; ++k) {
    std::vector<int32_t> voff((size_t)n), xoff((size_t)n * Ji, 0), ctoff, ctidx, ctstr;
    // the kernel's family f is node f's, wherever the caller listed it: the factors of a product are
    // multiplied in node order, so the bits of a result do not depend on the order the families came in
    for (int32_t f = 0; f < n; ++f) {
      const size_t given = (size_t)fam_of[k][(size_t)f];
      const pgm_fit_family &F = fams[k][given];
      voff[(size_t)f] = (int32_t)p.off[k][given];
      ctoff.push_back((int32_t)ctidx.size());
      std::vector<int32_t> io;
      int32_t stride = (int32_t)p.size[k][given];
      for (int32_t j = 0; j < F.n_vars; ++j) {
        stride /= F.card[j];  // C order: the last variable fastest
        const int32_t c = F.col[j], v = c % n;
        // the window of codes a slice keeps: [0, n) the slice before, [n, 2n) the slice itself
        const bool before = k == 1 && c < n;
        if (clamped[v]) {
          ctidx.push_back(before ? v : n + v);
          ctstr.push_back(stride);
        } else if (before) {
          if (io.empty()) io.assign((size_t)Si, 0);
          for (int32_t i = 0; i < Si; ++i) io[(size_t)i] += i / istride[(size_t)v] % card[v] * stride;
        } else {
          for (int32_t x = 0; x < Ji; ++x) xoff[(size_t)f * Ji + x] += digit(x, v) * stride;
        }
      }
      if (k == 1) {
        if (io.empty()) {
          cur.push_back(f);
        } else {
          prev.push_back(f);
          ioff.insert(ioff.end(), io.begin(), io.end());
        }
      }
    }
    ctoff.push_back((int32_t)ctidx.size());
    L.o_voff[k] = tab_put(tab, voff);
    L.o_xoff[k] = tab_put(tab, xoff);
    L.o_ctoff[k] = tab_put(tab, ctoff);
    L.o_ctidx[k] = tab_put(tab, ctidx);
    L.o_ctstr[k] = tab_put(tab, ctstr);
  }
  L.n_cur = (int32_t)cur.size(), L.n_prev = (int32_t)prev.size();
  L.o_cur = tab_put(tab, cur);
  L.o_prev = tab_put(tab, prev);
  L.o_ioff = tab_put(tab, ioff);

  std::vector<int32_t> qnode, qstate;
  for (int32_t v = 0; v < n; ++v)
    if (queried && queried[v])
      for (int32_t s = 0; s < card[v]; ++s) qnode.push_back(v), qstate.push_back(s);
  L.Q = (int32_t)qnode.size();
  L.o_qnode = tab_put(tab, qnode);
  L.o_qstate = tab_put(tab, qstate);
  out = std::move(p);
  return PGM_OK;
}

int dbn_run_check(const DbnHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                  int32_t n_slices, const double *values0, const double *values1, const double *filter, const double *smooth,
                  const double *loglik, const double *scratch, int64_t scratch_bytes, bool *launch) {
  *launch = false;
  if (!h) return pgmi_failf(PGM_EINVAL, "dbn_run: null plan");
  const DbnLayout &L = h->p.L;
  if (!codes || !values0 || !values1) return pgmi_failf(PGM_EINVAL, "dbn_run: null codes / values");
  if (n_slices < 1 || n_slices > kDbnMaxSlices)
    return pgmi_failf(PGM_EINVAL, "dbn_run: %d slices (1 .. %d)", n_slices, kDbnMaxSlices);
  if ((int64_t)n_cols != (int64_t)n_slices * L.n)
    return pgmi_failf(PGM_EINVAL, "dbn_run: %d code columns, %d slices of %d nodes need %lld", n_cols, n_slices, L.n,
                      (long long)n_slices * L.n);
  if (ld < 0 || row0 < 0 || n_rows < 0 || n_rows > ld || row0 > ld - n_rows)
    return pgmi_failf(PGM_EINVAL, "dbn_run: rows [%lld, %lld + %lld) are outside ld %lld", (long long)row0, (long long)row0,
                      (long long)n_rows, (long long)ld);
  const void *f64[] = {values0, values1, filter, smooth, loglik, scratch};
  for (const void *q : f64)
    if ((uintptr_t)q % 8) return pgmi_failf(PGM_EINVAL, "dbn_run: an fp64 pointer is not 8-byte aligned");
  if (smooth) {
    if (scratch_bytes < 0 || (scratch_bytes > 0 && !scratch)) return pgmi_failf(PGM_EINVAL, "dbn_run: null scratch");
    // n_rows <= ld and the factors below are small: no overflow before the comparison
    const double need = (double)n_rows * n_slices * (L.S + 1) * 8.0;
    if (need > (double)scratch_bytes)
      return pgmi_failf(PGM_EINVAL, "dbn_run: smooth needs %.0f bytes of scratch (n_rows x slices x (S + 1) doubles), %lld given",
                        need, (long long)scratch_bytes);
  }
  *launch = n_rows > 0;
  return PGM_OK;
}

int dbn_viterbi_check(const DbnHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                      int32_t n_slices, const double *values0, const double *values1, const uint8_t *path, int64_t ld_out,
                      int64_t row0_out, const double *logmap, const void *scratch, int64_t scratch_bytes, bool *launch) {
  *launch = false;
  if (!h) return pgmi_failf(PGM_EINVAL, "dbn_viterbi: null plan");
  const DbnLayout &L = h->p.L;
  if (!codes || !values0 || !values1) return pgmi_failf(PGM_EINVAL, "dbn_viterbi: null codes / values");
  if (!path) return pgmi_failf(PGM_EINVAL, "dbn_viterbi: null path");
  if (n_slices < 1 || n_slices > kDbnMaxSlices)
    return pgmi_failf(PGM_EINVAL, "dbn_viterbi: %d slices (1 .. %d)", n_slices, kDbnMaxSlices);
  if ((int64_t)n_cols != (int64_t)n_slices * L.n)
    return pgmi_failf(PGM_EINVAL, "dbn_viterbi: %d code columns, %d slices of %d nodes need %lld", n_cols, n_slices, L.n,
                      (long long)n_slices * L.n);
  if (ld < 0 || row0 < 0 || n_rows < 0 || n_rows > ld || row0 > ld - n_rows)
    return pgmi_failf(PGM_EINVAL, "dbn_viterbi: rows [%lld, %lld + %lld) are outside ld %lld", (long long)row0, (long long)row0,
                      (long long)n_rows, (long long)ld);
  if (ld_out < 0 || row0_out < 0 || n_rows > ld_out || row0_out > ld_out - n_rows)
    return pgmi_failf(PGM_EINVAL, "dbn_viterbi: path rows [%lld, %lld + %lld) are outside ld_out %lld", (long long)row0_out,
                      (long long)row0_out, (long long)n_rows, (long long)ld_out);
  const void *f64[] = {values0, values1, logmap};
  for (const void *q : f64)
    if ((uintptr_t)q % 8) return pgmi_failf(PGM_EINVAL, "dbn_viterbi: an fp64 pointer is not 8-byte aligned");
  if ((uintptr_t)scratch % 2) return pgmi_failf(PGM_EINVAL, "dbn_viterbi: the scratch is not 2-byte aligned");
  // n_rows <= ld and the factors are small: no overflow before the comparison
  const double need = dbn_viterbi_scratch(n_rows, n_slices, L.J);
  if (scratch_bytes < 0 || need > (double)scratch_bytes || (need > 0 && !scratch))
    return pgmi_failf(PGM_EINVAL,
                      "dbn_viterbi: the backpointers need %.0f bytes of scratch (n_rows x (slices - 1) x J uint16), %lld given", need,
                      (long long)scratch_bytes);
  *launch = n_rows > 0;
  return PGM_OK;
}

// The tile whenever it fits: no cap on its size.  Measured (profiles/dbn_em_bench.json, 100,000 sequences x 101
// slices): the tile took 12.4 ms where the direct path took 1,708 ms (HMM, 328 entries), and 28.9 ms where it took
// 11.1 s (six chains, 420 entries, 1,000 sequences); a tile near the LDS limit has not been measured.
DbnEstepGeom dbn_estep_geom(const DbnPlan &p, uint32_t flags) {
  DbnEstepGeom g;
  g.tile_at = (p.lds_bytes + 7) / 8;
  g.tile_bytes = 8 * (p.total[0] + p.total[1]);
  g.fits = g.tile_at * 8 + g.tile_bytes <= kDbnLdsMax;
  g.tile = g.fits && !(flags & PGM_DBN_ESTEP_DIRECT);
  g.lds_bytes = g.tile ? g.tile_at * 8 + g.tile_bytes : p.lds_bytes;
  if (g.tile) {
    g.blocks_per_cu = (int32_t)std::min<int64_t>(kDbnWavesPerCu, kDbnLdsMax / g.lds_bytes);
    g.max_blocks = (int64_t)kDbnCus * g.blocks_per_cu;
  }
  return g;
}

int dbn_estep_check(const DbnHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                    int32_t n_slices, const double *values0, const double *values1, const double *tables0, const double *tables1,
                    const double *loglik, const double *scratch, int64_t scratch_bytes, uint32_t flags, bool *launch) {
  *launch = false;
  if (!tables0 || !tables1) return pgmi_failf(PGM_EINVAL, "dbn_estep: null tables");
  if (flags & ~PGM_DBN_ESTEP_DIRECT) return pgmi_failf(PGM_EINVAL, "dbn_estep: unknown flag bits 0x%x", flags & ~PGM_DBN_ESTEP_DIRECT);
  // the tables stand where a smoother's outputs do: 8-byte aligned, and the scratch rule of a smoother holds
  return dbn_run_check(h, codes, n_cols, ld, row0, n_rows, n_slices, values0, values1, tables0, tables1, loglik, scratch,
                       scratch_bytes, launch);
}

extern "C" {

int pgm_dbn_estep_info(void *plan, uint32_t flags, pgm_dbn_estep_info_t *info) {
  const DbnHandle *h = static_cast<const DbnHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "dbn_estep_info: null plan");
  if (flags & ~PGM_DBN_ESTEP_DIRECT)
    return pgmi_failf(PGM_EINVAL, "dbn_estep_info: unknown flag bits 0x%x", flags & ~PGM_DBN_ESTEP_DIRECT);
  if (info) {
    const DbnEstepGeom g = dbn_estep_geom(h->p, flags);
    info->path = g.tile ? PGM_DBN_ESTEP_TILE : (int32_t)PGM_DBN_ESTEP_DIRECT;
    info->tile_fits = g.fits ? 1 : 0;
    info->blocks_per_cu = g.blocks_per_cu;
    info->reserved = 0;
    info->lds_bytes = g.lds_bytes;
    info->tile_bytes = g.tile_bytes;
    info->max_blocks = g.max_blocks;
  }
  return PGM_OK;
}

int pgm_dbn_plan_create(const int32_t *card, const uint8_t *clamped, const uint8_t *queried, int32_t n,
                        const pgm_fit_family *families0, int32_t n_families0, const pgm_fit_family *families1,
                        int32_t n_families1, void **plan) {
  if (!plan) return pgmi_failf(PGM_EINVAL, "dbn_plan_create: null plan");
  *plan = nullptr;
  DbnHandle *h = new (std::nothrow) DbnHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "dbn_plan_create: out of memory");
  const int st = dbn_plan_build(card, clamped, queried, n, families0, n_families0, families1, n_families1, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *plan = h;
  return PGM_OK;
}

int pgm_dbn_info(void *plan, pgm_dbn_info_t *info, int64_t *off0, int64_t *off1) {
  const DbnHandle *h = static_cast<const DbnHandle *>(plan);
  if (!h) return pgmi_failf(PGM_EINVAL, "dbn_info: null plan");
  const DbnPlan &p = h->p;
  if (info) {
    info->n = p.L.n;
    info->n_free = p.L.n_free;
    info->n_configs = p.L.J;
    info->n_interface = p.L.S;
    info->n_prev_families = p.L.n_prev;
    info->n_cur_families = p.L.n_cur;
    info->seq_per_wave = p.L.spw;
    info->block = kDbnBlock;
    info->n_query = p.L.Q;
    info->reserved = 0;
    info->lds_bytes = p.lds_bytes;
    info->values0 = p.total[0];
    info->values1 = p.total[1];
    info->scratch_per_slice = (int64_t)p.L.S + 1;
  }
  if (off0) std::copy(p.off[0].begin(), p.off[0].end(), off0);
  if (off1) std::copy(p.off[1].begin(), p.off[1].end(), off1);
  return PGM_OK;
}
}

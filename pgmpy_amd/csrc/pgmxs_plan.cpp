// pgmxs_plan.cpp — the host side of the exact structure search (include/pgmhip.h "Exact structure search"): the
// tiling of the two lattice kernels, the zeta launches, the popcount-ordered lists the sink kernel walks, the launch
// counts, and the checks of a family list.  No HIP call and no HIP include: ctypes drives all of it without a device.
// The kernels and the launches are pgmxs.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pgm_xs.h"

static inline int xs_popc(uint32_t x) { return __builtin_popcount(x); }

// the values 0 .. 2^bits - 1 by (popcount, value); off[q]: where popcount q starts, off[bits + 1]: the end
template <class T, class Off>
static void xs_layers(int bits, std::vector<T> &list, Off *off) {
  list.clear();
  for (int q = 0; q <= bits; ++q) {
    off[q] = (int32_t)list.size();
    for (uint32_t x = 0; x < (1u << bits); ++x)
      if (xs_popc(x) == q) list.push_back((T)x);
  }
  off[bits + 1] = (int32_t)list.size();
}

int xs_plan_build(int32_t n, int32_t L, int32_t h, XsPlan &out) {
  if (n < 1 || n > PGM_XS_MAX_NODES)
    return pgmi_failf(PGM_EINVAL, "xs: %d nodes (1 to %d)", n, PGM_XS_MAX_NODES);
  if (L < 1 || L > kXsMaxTile || h < 1 || h > L)
    return pgmi_failf(PGM_EINVAL, "xs: tiling L = %d, h = %d (1 <= h <= L <= %d)", L, h, kXsMaxTile);
  XsPlan p;
  p.n = n, p.W = n - 1, p.L = L, p.h = h;
  p.Lz = std::min(L, p.W), p.Ls = std::min(L, n);
  p.q_cells = (int64_t)n << p.W, p.r_cells = (int64_t)1 << n;
  p.post_rows = std::min(n, std::max(1, kXsPostCells >> p.W));
  if (p.W > 0) p.trips.push_back(XsTrip{p.Lz, p.Lz, 0, 0, p.Lz});
  for (int32_t b0 = p.Lz; b0 < p.W; b0 += h) {
    const int32_t hh = std::min(h, p.W - b0);
    p.trips.push_back(XsTrip{p.Lz - hh, b0, hh, p.Lz - hh, p.Lz});
  }
  p.hi_off.assign((size_t)(n - p.Ls) + 2, 0);
  xs_layers(n - p.Ls, p.hi_list, p.hi_off.data());
  xs_layers(p.Ls, p.lo_list, p.lo_off);
  out = std::move(p);
  return PGM_OK;
}

int xs_run_check(const char *who, const XsHandle *h, const int32_t *fam_node, const uint32_t *fam_mask,
                 const double *fam_score, int64_t n_fam, bool out, std::vector<uint32_t> &cell,
                 std::vector<uint32_t> &mask, std::vector<double> &score) {
  if (!h) return pgmi_failf(PGM_EINVAL, "%s: null handle", who);
  if (!out) return pgmi_failf(PGM_EINVAL, "%s: null result", who);
  if (n_fam < 0 || (n_fam > 0 && (!fam_node || !fam_mask || !fam_score)))
    return pgmi_failf(PGM_EINVAL, "%s: null family arrays / a negative count", who);
  const XsPlan &p = h->p;
  if (n_fam > p.q_cells) return pgmi_failf(PGM_EINVAL, "%s: %lld families, more than there are (node, parent set) pairs", who, (long long)n_fam);
  const uint32_t all = (1u << p.n) - 1;
  std::vector<uint32_t> seen((size_t)n_fam);
  cell.clear(), mask.clear(), score.clear();
  for (int64_t f = 0; f < n_fam; ++f) {
    const int32_t v = fam_node[f];
    const uint32_t P = fam_mask[f];
    const double s = fam_score[f];
    if (v < 0 || v >= p.n) return pgmi_failf(PGM_EINVAL, "%s: family %lld: node %d of %d", who, (long long)f, v, p.n);
    if (P & ~all) return pgmi_failf(PGM_EINVAL, "%s: family %lld: parent mask 0x%x has a bit at or above %d", who, (long long)f, P, p.n);
    if (P >> v & 1) return pgmi_failf(PGM_EINVAL, "%s: family %lld: node %d is among its own parents", who, (long long)f, v);
    if (std::isnan(s) || (std::isinf(s) && s > 0))
      return pgmi_failf(PGM_EINVAL, "%s: family %lld: score %g (finite or -inf)", who, (long long)f, s);
    const uint32_t T = (P & ((1u << v) - 1)) | ((P >> (v + 1)) << v);
    const uint32_t c = ((uint32_t)v << p.W) + T;
    seen[(size_t)f] = c;
    if (std::isinf(s)) continue;  // as good as absent: the cell keeps -inf and no winner
    cell.push_back(c), mask.push_back(P), score.push_back(s);
  }
  std::sort(seen.begin(), seen.end());
  const auto dup = std::adjacent_find(seen.begin(), seen.end());
  if (dup != seen.end()) {
    const uint32_t v = *dup >> p.W, T = *dup & ((1u << p.W) - 1);
    return pgmi_failf(PGM_EINVAL, "%s: node %u is given the parent mask 0x%x twice", who, v,
                      (T & ((1u << v) - 1)) | ((T >> v) << (v + 1)));
  }
  return PGM_OK;
}

void xs_by_node(const XsPlan &p, std::vector<uint32_t> &cell, std::vector<uint32_t> &mask, std::vector<double> &score,
                uint32_t *off) {
  std::vector<uint32_t> at(cell.size());
  for (size_t i = 0; i < at.size(); ++i) at[i] = (uint32_t)i;
  std::sort(at.begin(), at.end(), [&](uint32_t x, uint32_t y) { return cell[x] < cell[y]; });  // no two cells are equal
  std::vector<uint32_t> c(at.size()), m(at.size());
  std::vector<double> s(at.size());
  for (size_t i = 0; i < at.size(); ++i) c[i] = cell[at[i]], m[i] = mask[at[i]], s[i] = score[at[i]];
  cell.swap(c), mask.swap(m), score.swap(s);
  for (int32_t v = 0; v <= p.n; ++v)
    off[v] = (uint32_t)(std::lower_bound(cell.begin(), cell.end(), (uint32_t)v << p.W) - cell.begin());
}

extern "C" {

int pgm_xs_create(int32_t n, void **handle) {
  return plan_create<XsHandle>("xs_create", handle,
                               [&](XsPlan &p) { return xs_plan_build(n, kXsMaxTile, kXsDefaultHigh, p); });
}

int pgm_xs_info(void *handle, pgm_xs_info_t *info) {
  if (!handle || !info) return pgmi_fail(PGM_EINVAL, "xs_info: null handle / info");
  const XsPlan &p = static_cast<const XsHandle *>(handle)->p;
  memset(info, 0, sizeof *info);
  info->n = p.n, info->tile_log2 = p.L, info->high_bits = p.h, info->block = kXsBlock;
  info->zeta_tile_log2 = p.Lz, info->sink_tile_log2 = p.Ls;
  info->zeta_low_passes = p.Lz, info->zeta_high_trips = p.trips.empty() ? 0 : (int32_t)p.trips.size() - 1;
  info->zeta_launches = (int32_t)p.trips.size(), info->sink_launches = p.n - p.Ls + 1;
  info->q_bytes = 8 * p.q_cells, info->a_bytes = 4 * p.q_cells, info->r_bytes = 8 * p.r_cells, info->k_bytes = 4 * p.r_cells;
  info->zeta_lds = p.W ? xs_zeta_lds(p) : 0, info->sink_lds = xs_sink_lds(p);
  return PGM_OK;
}

int pgm_xs_phase_ms(void *handle, double *ms) {
  if (!handle || !ms) return pgmi_fail(PGM_EINVAL, "xs_phase_ms: null handle / ms");
  const XsHandle *h = static_cast<const XsHandle *>(handle);
  if (!h->timed) return pgmi_fail(PGM_EINVAL, "xs_phase_ms: the handle has no completed run");
  std::copy(h->phase_ms, h->phase_ms + h->timed, ms);
  return PGM_OK;
}
}

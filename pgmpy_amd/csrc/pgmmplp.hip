// pgmmplp.hip — MAP by max-product linear programming on a Markov network, on the device (gfx950): k_mplp runs a
// whole batch of instances, one workgroup each, through every iteration of the message updates, the decode, the
// primal and dual values and the convergence test in one launch, with the state in LDS throughout; and the C-ABI
// (pgm_mplp_plan_destroy, pgm_mplp_run).  The contract is include/pgmhip.h "MAP by max-product linear
// programming"; the host side (validation, intersection sets, levels, item lists, LDS layout, argument checks,
// pgm_mplp_plan_info) is pgmmplp_plan.cpp.  fp64 and integers only; additions, subtractions, comparisons and one
// multiplication by 1 / k: nothing a compiler could contract.
#include "pgm_hip_common.h"
#include "pgm_mplp.h"

struct MplpArgs {
  const int32_t *node_off;
  const MplpCluster *clusters;
  const MplpSet *sets;
  const int32_t *lev_set, *lev_cell;
  const uint32_t *set_items, *cell_items;
  int32_t n_nodes, n_clusters, n_levels, n_iter;
  int32_t n_unary, n_theta, n_tab, n_stage;
  int64_t state_len;
  double dual_thr, gap_thr;
  const double *unaries, *theta, *state_in;
  uint8_t *codes;
  double *values;
  int32_t *iters;
  double *state_out;
};

// The first-index argmax of every node objective into cur, then the two sums of an iteration: dual = the maxima
// of all objectives, primal = the original terms at cur.  Work-item l adds nodes l, l + 256, ... and then clusters
// l, l + 256, ... in that order; a wave adds its 64 partial sums in a butterfly (every lane ends with the same
// bits: each stage adds the same two values on both sides), and the four wave totals are added in wave order.
// Fixed by kMplpBlock alone.  Every work-item returns the same two values.
__device__ __forceinline__ void mplp_totals(const MplpArgs &a, const double *st, const double *th, const double *un,
                                            uint8_t *cur, double *pad, double &dual, double &primal) {
  const int32_t tid = (int32_t)threadIdx.x;
  double d = 0.0, p = 0.0;
  for (int32_t v = tid; v < a.n_nodes; v += kMplpBlock) {
    const int32_t o = a.node_off[v], n = a.node_off[v + 1] - o;
    double m = st[o];
    int32_t arg = 0;
    for (int32_t s = 1; s < n; ++s) {
      const double x = st[o + s];
      if (x > m) m = x, arg = s;
    }
    cur[v] = (uint8_t)arg;
    d += m;
    p += un[o + arg];
  }
  __syncthreads();
  for (int32_t c = tid; c < a.n_clusters; c += kMplpBlock) {
    const MplpCluster C = a.clusters[c];
    double m = st[C.off_obj];
    for (int32_t i = 1; i < C.size; ++i) {
      const double x = st[C.off_obj + i];
      if (x > m) m = x;
    }
    d += m;
    int32_t at = 0;
#pragma unroll
    for (int j = 0; j < kMplpMaxVars; ++j)
      if (j < C.nv) at += (int32_t)cur[C.var[j]] * C.cstride[j];
    p += th[C.off_theta + at];
  }
  for (int x = 32; x > 0; x >>= 1) {
    d += __shfl_xor(d, x);
    p += __shfl_xor(p, x);
  }
  if ((tid & 63) == 0) pad[tid >> 6] = d, pad[4 + (tid >> 6)] = p;
  __syncthreads();
  dual = ((pad[0] + pad[1]) + pad[2]) + pad[3];
  primal = ((pad[4] + pad[5]) + pad[6]) + pad[7];
  __syncthreads();  // the pad is written again by the next call
}

// Workgroup b runs instance b.  Dynamic LDS as mplp_lds_bytes lays it out.  THETA_LDS: the cluster terms are
// copied to LDS once; otherwise they are read through the caches, which every instance of the launch shares.
template <bool THETA_LDS>
__global__ __launch_bounds__(kMplpBlock) void k_mplp(MplpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t tid = (int32_t)threadIdx.x;
  double *st = reinterpret_cast<double *>(smem);  // [n_tab]: node objectives, cluster objectives, messages
  double *stage = st + a.n_tab;                   // [n_stage]: phi of the level's sets
  double *th_lds = stage + a.n_stage;
  double *pad = th_lds + (THETA_LDS ? a.n_theta : 0);
  uint8_t *cur = reinterpret_cast<uint8_t *>(pad + kMplpPadBytes / 8);
  uint8_t *bestc = cur + (a.n_nodes + 7) / 8 * 8;
  const double *th = THETA_LDS ? th_lds : a.theta;
  const int64_t b = blockIdx.x;
  const double *un = a.unaries + b * a.n_unary;

  double best = -INFINITY, dual_lp = 0.0;
  if (a.state_in) {
    const double *si = a.state_in + b * a.state_len;
    for (int32_t i = tid; i < a.n_tab; i += kMplpBlock) st[i] = si[i];
    for (int32_t v = tid; v < a.n_nodes; v += kMplpBlock) bestc[v] = (uint8_t)(int32_t)si[a.n_tab + 2 + v];
    best = si[a.n_tab], dual_lp = si[a.n_tab + 1];
  } else {
    for (int32_t i = tid; i < a.n_unary; i += kMplpBlock) st[i] = un[i];
    for (int32_t i = tid; i < a.n_theta; i += kMplpBlock) st[a.n_unary + i] = a.theta[i];
    for (int32_t i = a.n_unary + a.n_theta + tid; i < a.n_tab; i += kMplpBlock) st[i] = 0.0;
    for (int32_t v = tid; v < a.n_nodes; v += kMplpBlock) bestc[v] = 0;
  }
  if constexpr (THETA_LDS)
    for (int32_t i = tid; i < a.n_theta; i += kMplpBlock) th_lds[i] = a.theta[i];
  __syncthreads();
  if (!a.state_in) {  // the dual value of the terms as given
    double ignored;
    mplp_totals(a, st, th, un, cur, pad, dual_lp, ignored);
  }

  double dual_gap = (double)NAN, int_gap = (double)NAN;
  int32_t used = 0;
  for (int32_t it = 0; it < a.n_iter; ++it) {
    for (int32_t lev = 0; lev < a.n_levels; ++lev) {
      const int32_t s0 = a.lev_set[lev], s1 = a.lev_set[lev + 1];
      // 1. phi of every cell of every set of the level's clusters: the maximum over the cluster's other variables
      //    of S = obj[c] + obj[s_0] + obj[s_1] + obj[s_2], added in that order, times 1 / k
      for (int32_t i = s0 + tid; i < s1; i += kMplpBlock) {
        const uint32_t item = a.set_items[i];
        const int32_t cell = (int32_t)(item & 0xffffu);
        const MplpSet S = a.sets[item >> 16];
        const MplpCluster C = a.clusters[S.cluster];
        int32_t at_c = C.off_obj, at0 = C.sobj[0], at1 = C.sobj[1], at2 = C.sobj[2];
        int32_t n0 = 1, n1 = 1, c0 = 0, c1 = 0, p00 = 0, p01 = 0, p10 = 0, p11 = 0, p20 = 0, p21 = 0, n_free = 0;
#pragma unroll
        for (int j = 0; j < kMplpMaxVars; ++j) {
          if (j >= C.nv) continue;
          if (S.str[j]) {  // a variable of the set: fixed by the cell
            const int32_t x = cell / S.str[j] % C.card[j];
            at_c += x * C.cstride[j], at0 += x * C.sstr[j], at1 += x * C.sstr[3 + j], at2 += x * C.sstr[6 + j];
          } else if (n_free++ == 0) {
            n0 = C.card[j], c0 = C.cstride[j], p00 = C.sstr[j], p10 = C.sstr[3 + j], p20 = C.sstr[6 + j];
          } else {
            n1 = C.card[j], c1 = C.cstride[j], p01 = C.sstr[j], p11 = C.sstr[3 + j], p21 = C.sstr[6 + j];
          }
        }
        double m = -INFINITY;
        for (int32_t x0 = 0; x0 < n0; ++x0)
          for (int32_t x1 = 0; x1 < n1; ++x1) {
            double v = st[at_c + x0 * c0 + x1 * c1];
            v += st[at0 + x0 * p00 + x1 * p01];
            if (C.k > 1) v += st[at1 + x0 * p10 + x1 * p11];
            if (C.k > 2) v += st[at2 + x0 * p20 + x1 * p21];
            m = v > m ? v : m;
          }
        stage[S.off_stage + cell] = m * (1.0 / (double)C.k);
      }
      __syncthreads();
      // 2. the new messages and the sets' objectives (a set belongs to one cluster of the level)
      for (int32_t i = s0 + tid; i < s1; i += kMplpBlock) {
        const uint32_t item = a.set_items[i];
        const int32_t cell = (int32_t)(item & 0xffffu);
        const MplpSet S = a.sets[item >> 16];
        const double phi = stage[S.off_stage + cell];
        st[S.off_msg + cell] = phi - (st[S.off_obj + cell] - st[S.off_msg + cell]);
        st[S.off_obj + cell] = phi;
      }
      __syncthreads();
      // 3. the clusters' objectives: theta less the new messages, in set order
      for (int32_t i = a.lev_cell[lev] + tid; i < a.lev_cell[lev + 1]; i += kMplpBlock) {
        const uint32_t item = a.cell_items[i];
        const int32_t cell = (int32_t)(item & 0xffffu);
        const MplpCluster C = a.clusters[item >> 16];
        int32_t at0 = C.smsg[0], at1 = C.smsg[1], at2 = C.smsg[2];
#pragma unroll
        for (int j = 0; j < kMplpMaxVars; ++j) {
          if (j >= C.nv) continue;
          const int32_t x = cell / C.cstride[j] % C.card[j];
          at0 += x * C.sstr[j], at1 += x * C.sstr[3 + j], at2 += x * C.sstr[6 + j];
        }
        double v = th[C.off_theta + cell];
        v -= st[at0];
        if (C.k > 1) v -= st[at1];
        if (C.k > 2) v -= st[at2];
        st[C.off_obj + cell] = v;
      }
      __syncthreads();
    }

    // the decode, the two values, the convergence test: the same on every work-item
    double new_dual, primal;
    mplp_totals(a, st, th, un, cur, pad, new_dual, primal);
    if (best < primal) {
      best = primal;
      for (int32_t v = tid; v < a.n_nodes; v += kMplpBlock) bestc[v] = cur[v];  // the cells this work-item decoded
    }
    dual_gap = fabs(dual_lp - new_dual);
    int_gap = fabs(dual_lp - best);
    const bool conv = (a.dual_thr != 0.0 && dual_gap < a.dual_thr) || (a.gap_thr != 0.0 && int_gap < a.gap_thr);
    if (!conv) dual_lp = new_dual;
    used = it + 1;
    if (conv && it >= kMplpMinStop) break;
  }

  for (int32_t v = tid; v < a.n_nodes; v += kMplpBlock) a.codes[b * a.n_nodes + v] = bestc[v];
  if (a.state_out) {
    double *so = a.state_out + b * a.state_len;
    for (int32_t i = tid; i < a.n_tab; i += kMplpBlock) so[i] = st[i];
    for (int32_t v = tid; v < a.n_nodes; v += kMplpBlock) so[a.n_tab + 2 + v] = (double)bestc[v];
    if (tid == 0) so[a.n_tab] = best, so[a.n_tab + 1] = dual_lp;
  }
  if (tid == 0) {
    double *val = a.values + b * PGM_MPLP_VALUES;
    val[0] = best, val[1] = dual_lp, val[2] = dual_gap, val[3] = int_gap;
    a.iters[b] = used;
  }
}

// ---------------------------------------------------------------------------- the handle's device side
static int mplp_use(MplpHandle *h) {
  const MplpPlan &p = h->p;
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_node_off, p.node_off),   pgmdev::upload(h->d_clusters, p.clusters),
                               pgmdev::upload(h->d_sets, p.sets),           pgmdev::upload(h->d_lev_set, p.lev_set),
                               pgmdev::upload(h->d_lev_cell, p.lev_cell),   pgmdev::upload(h->d_set_items, p.set_items),
                               pgmdev::upload(h->d_cell_items, p.cell_items)};
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_mplp_plan_destroy(void *plan) { return pgm_plan_destroy<MplpHandle>(plan); }

int pgm_mplp_run(void *plan, const double *unaries, const double *theta, int64_t n_rows, int32_t n_iter,
                 double dual_threshold, double gap_threshold, const double *state_in, uint8_t *codes, double *values,
                 int32_t *iters, double *state_out, void *stream) {
  MplpHandle *h = static_cast<MplpHandle *>(plan);
  bool launch = false;
  const int st = mplp_run_check(h, unaries, theta, n_rows, n_iter, dual_threshold, gap_threshold, state_in, codes, values,
                                iters, state_out, &launch);
  if (st != PGM_OK || !launch) return st;
  const MplpPlan &p = h->p;
  const int up = mplp_use(h);
  if (up != PGM_OK) return up;
  const void *kernel = p.theta_in_lds ? reinterpret_cast<const void *>(&k_mplp<true>) : reinterpret_cast<const void *>(&k_mplp<false>);
  // above 64 KiB of dynamic LDS a kernel has to be told so before the launch
  if (p.lds_bytes > 65536) HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  MplpArgs a = {};
  a.node_off = h->d_node_off, a.clusters = h->d_clusters, a.sets = h->d_sets;
  a.lev_set = h->d_lev_set, a.lev_cell = h->d_lev_cell, a.set_items = h->d_set_items, a.cell_items = h->d_cell_items;
  a.n_nodes = p.n_nodes, a.n_clusters = p.n_clusters, a.n_levels = p.n_levels, a.n_iter = n_iter;
  a.n_unary = (int32_t)p.n_unary, a.n_theta = (int32_t)p.n_theta, a.n_tab = (int32_t)p.n_tab, a.n_stage = (int32_t)p.n_stage;
  a.state_len = p.state_len;
  a.dual_thr = dual_threshold, a.gap_thr = gap_threshold;
  a.unaries = unaries, a.theta = theta, a.state_in = state_in;
  a.codes = codes, a.values = values, a.iters = iters, a.state_out = state_out;
  const dim3 grid((unsigned)n_rows), wg(kMplpBlock);
  if (p.theta_in_lds) hipLaunchKernelGGL(k_mplp<true>, grid, wg, (size_t)p.lds_bytes, S(stream), a);
  else hipLaunchKernelGGL(k_mplp<false>, grid, wg, (size_t)p.lds_bytes, S(stream), a);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

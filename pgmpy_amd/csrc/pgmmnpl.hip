// pgmmnpl.hip — the log pseudo-likelihood of a Markov network and its gradient in the log-potentials, from count
// tables, on the device (gfx950): k_mn_pl (one workgroup per node: the conditionals of every blanket configuration,
// the residual table in LDS, the node's value, the node's share of the gradient of every incident factor),
// k_mn_pl_gather (the shares added per entry, the ridge term, the value) and the C-ABI (pgm_mnpl_plan_destroy,
// pgm_mnpl_eval).  The contract is include/pgmhip.h "Pseudo-likelihood of a Markov network"; the host side
// (validation, blanket families, digits, part slots, LDS sizing, argument checks, pgm_mnpl_plan_info) is
// pgmmnpl_plan.cpp.  fp64 and integers only; no matrix instruction (gathers, exp and log: nothing to multiply), no
// atomic, no sum whose order depends on the launch.
#include "pgm_hip_common.h"
#include "pgm_mnpl.h"

struct MnplArgs {
  const int32_t *inc_off;
  const GibbsInc *inc;
  const GibbsOther *others;
  const MnplNode *nodes;
  const MnplInc *minc;
  const MnplDigit *odig, *free;
  const int64_t *counts;
  const double *theta;
  double *parts, *node_val;
};

// Node i on its workgroup.  r: the residual table [card][n_cfg]; ths: the LDS copy of the incident tables (TH_LDS).
template <bool TH_LDS>
__device__ __forceinline__ void mn_pl_node(const MnplArgs &a, int32_t i, const MnplNode &nd, double *r, double *ths,
                                           double *pad) {
  const int32_t tid = (int32_t)threadIdx.x;
  const int32_t e0 = a.inc_off[i], e1 = a.inc_off[i + 1], K = nd.card, Q = nd.n_cfg;
  if constexpr (TH_LDS) {
    for (int32_t e = e0; e < e1; ++e) {
      const double *src = a.theta + a.inc[e].off;
      double *dst = ths + a.minc[e].lds_off;
      for (int32_t k = tid, n = a.minc[e].size; k < n; k += kMnplBlock) dst[k] = src[k];
    }
    __syncthreads();
  }

  // Phase A: a work-item owns the configurations c = tid, tid + 256, ..; cell (s, c) of r is its own until the barrier
  const int64_t *cnt = a.counts + nd.count_off;
  double part = 0.0;
  for (int32_t c = tid; c < Q; c += kMnplBlock) {
    int64_t N = 0;
    for (int32_t s = 0; s < K; ++s) N += cnt[(int64_t)s * Q + c];
    if (N == 0) {  // an empty configuration: no residual, no term, no exp
      for (int32_t s = 0; s < K; ++s) r[s * Q + c] = 0.0;
      continue;
    }
    // the logits, factor by factor in ascending order, accumulated in the cells
    for (int32_t e = e0; e < e1; ++e) {
      const GibbsInc I = a.inc[e];
      int64_t base = TH_LDS ? (int64_t)a.minc[e].lds_off : I.off;
      for (int32_t o = I.other_begin; o < I.other_end; ++o) {
        const MnplDigit d = a.odig[o];
        base += (int64_t)((c / d.div) % d.card) * a.others[o].stride;
      }
      const double *t = (TH_LDS ? ths : a.theta) + base;
      if (e == e0)
        for (int32_t s = 0; s < K; ++s) r[s * Q + c] = t[(int64_t)s * I.stride];
      else
        for (int32_t s = 0; s < K; ++s) r[s * Q + c] += t[(int64_t)s * I.stride];
    }
    double top = r[c];
    for (int32_t s = 1; s < K; ++s) top = r[s * Q + c] > top ? r[s * Q + c] : top;
    double z = 0.0;
    for (int32_t s = 0; s < K; ++s) z += exp(r[s * Q + c] - top);
    const double lse = top + log(z), total = (double)N;
    for (int32_t s = 0; s < K; ++s) {
      const double l = r[s * Q + c] - lse, n = (double)cnt[(int64_t)s * Q + c];
      part += n * l;
      r[s * Q + c] = n - total * exp(l);
    }
  }
  // the node's value: a butterfly over the wave (the same two values meet on both sides of every stage), then the
  // four wave totals in wave order.  Its barrier is also the one between the phases.
  for (int x = 32; x > 0; x >>= 1) part += __shfl_xor(part, x);
  if ((tid & 63) == 0) pad[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) a.node_val[i] = ((pad[0] + pad[1]) + pad[2]) + pad[3];

  // Phase B: entry t = (s, x) of incident factor e is the sum of r[s, c] over the configurations that agree with x
  // on the factor's other columns; the free columns' digits run in blanket order, so c ascends with k
  for (int32_t e = e0; e < e1; ++e) {
    const GibbsInc I = a.inc[e];
    const MnplInc M = a.minc[e];
    for (int32_t t = tid; t < M.size; t += kMnplBlock) {
      const int32_t s = (t / I.stride) % K;
      int32_t fixed = 0, n_free = Q;
      for (int32_t o = I.other_begin; o < I.other_end; ++o) {
        const MnplDigit d = a.odig[o];
        fixed += ((t / a.others[o].stride) % d.card) * d.div;
        n_free /= d.card;
      }
      const double *row = r + s * Q + fixed;
      double acc = 0.0;
      for (int32_t k = 0; k < n_free; ++k) {
        int32_t c = 0, rest = k;
        for (int32_t j = M.free_end - 1; j >= M.free_begin; --j) {
          const MnplDigit d = a.free[j];
          c += (rest % d.card) * d.div;
          rest /= d.card;
        }
        acc += row[c];
      }
      a.parts[M.part_off + t] = acc;
    }
  }
}

// Workgroup b is node b.  Dynamic LDS: the launch's is the largest node's; a node uses its own share of it.
__global__ __launch_bounds__(kMnplBlock) void k_mn_pl(MnplArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t i = (int32_t)blockIdx.x;
  const MnplNode nd = a.nodes[i];
  double *r = reinterpret_cast<double *>(smem);
  double *ths = r + (int64_t)nd.card * nd.n_cfg;
  if (nd.theta_lds) mn_pl_node<true>(a, i, nd, r, ths, ths + nd.n_theta);
  else mn_pl_node<false>(a, i, nd, r, ths, ths);
}

// grad[e] = the entry's parts in member order - l2 theta[e]; work-item 0 of the launch adds the value in node order,
// then the ridge term in entry order.
__global__ __launch_bounds__(kMnplGatherBlock) void k_mn_pl_gather(const int64_t *fac_off, const int64_t *part_off,
                                                                  int32_t n_factors, int32_t n_nodes, int64_t n_theta,
                                                                  const double *parts, const double *node_val,
                                                                  const double *theta, double l2, double *value,
                                                                  double *grad, double *node_values) {
  const int64_t e = (int64_t)blockIdx.x * kMnplGatherBlock + threadIdx.x;
  if (grad && e < n_theta) {
    int32_t lo = 0, hi = n_factors;  // the factor of entry e: fac_off[lo] <= e < fac_off[lo + 1]
    while (hi - lo > 1) {
      const int32_t mid = (lo + hi) >> 1;
      if (fac_off[mid] <= e) lo = mid;
      else hi = mid;
    }
    const int64_t size = fac_off[lo + 1] - fac_off[lo], p0 = part_off[lo] + (e - fac_off[lo]), p1 = part_off[lo + 1];
    double acc = parts[p0];
    for (int64_t q = p0 + size; q < p1; q += size) acc += parts[q];
    grad[e] = acc - l2 * theta[e];
  }
  if (node_values && e < n_nodes) node_values[e] = node_val[e];
  if (e == 0) {
    double v = 0.0;
    for (int32_t i = 0; i < n_nodes; ++i) v += node_val[i];
    if (l2 != 0.0)
      for (int64_t k = 0; k < n_theta; ++k) v -= 0.5 * l2 * (theta[k] * theta[k]);
    *value = v;
  }
}

// ---------------------------------------------------------------------------- the handle's device side
static int mnpl_use(MnplHandle *h) {
  const MnplPlan &p = h->p;
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_inc_off, p.g.inc_off), pgmdev::upload(h->d_inc, p.g.inc),
                               pgmdev::upload(h->d_others, p.g.others),   pgmdev::upload(h->d_nodes, p.nodes),
                               pgmdev::upload(h->d_minc, p.minc),         pgmdev::upload(h->d_odig, p.odig),
                               pgmdev::upload(h->d_free, p.free),         pgmdev::upload(h->d_fac_off, p.fac_off),
                               pgmdev::upload(h->d_part_off, p.part_off), pgmdev::scratch(h->d_parts, (size_t)p.n_parts),
                               pgmdev::scratch(h->d_node_val, (size_t)p.g.n_cols)};
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_mnpl_plan_destroy(void *plan) { return pgm_plan_destroy<MnplHandle>(plan); }

int pgm_mnpl_eval(void *plan, const int64_t *counts, const double *theta, double l2, double *value, double *grad,
                  double *node_values, void *stream) {
  MnplHandle *h = static_cast<MnplHandle *>(plan);
  const int st = mnpl_eval_check(h, counts, theta, l2, value, grad, node_values);
  if (st != PGM_OK) return st;
  const MnplPlan &p = h->p;
  const int up = mnpl_use(h);
  if (up != PGM_OK) return up;
  // above 64 KiB of dynamic LDS a kernel has to be told so before the launch
  if (p.lds_bytes > 65536)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mn_pl), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)p.lds_bytes));
  MnplArgs a = {};
  a.inc_off = h->d_inc_off, a.inc = h->d_inc, a.others = h->d_others, a.nodes = h->d_nodes, a.minc = h->d_minc;
  a.odig = h->d_odig, a.free = h->d_free, a.counts = counts, a.theta = theta;
  a.parts = h->d_parts, a.node_val = h->d_node_val;
  hipLaunchKernelGGL(k_mn_pl, dim3((unsigned)p.g.n_cols), dim3(kMnplBlock), (size_t)p.lds_bytes, S(stream), a);
  HIP_TRY(hipGetLastError());
  const int64_t items = p.n_theta > p.g.n_cols ? p.n_theta : (int64_t)p.g.n_cols;
  const unsigned blocks = (unsigned)((items + kMnplGatherBlock - 1) / kMnplGatherBlock);
  hipLaunchKernelGGL(k_mn_pl_gather, dim3(blocks), dim3(kMnplGatherBlock), 0, S(stream), h->d_fac_off, h->d_part_off,
                     (int32_t)p.g.fit.fams.size(), p.g.n_cols, p.n_theta, h->d_parts, h->d_node_val, theta, l2, value,
                     grad, node_values);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

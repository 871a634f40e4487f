// pgmlbp.hip — marginals by sum-product loopy belief propagation on a Markov network, on the device (gfx950): k_lbp
// runs a whole batch of instances, one workgroup each, through every iteration of the flooding schedule, the
// convergence test, the node and factor beliefs and the Bethe value in one launch, with the node terms, the messages
// and (when they fit) the unique factor tables in LDS throughout; and the C-ABI (pgm_lbp_plan_destroy, pgm_lbp_run).
// The contract is include/pgmhip.h "Marginals by loopy belief propagation"; the host side (validation, pairs,
// incidence lists, table deduplication, LDS layout, argument checks, pgm_lbp_plan_info) is pgmlbp_plan.cpp.  fp64 in
// the linear domain and integers only; no matrix instruction (a matrix-vector product per instance), no float atomic,
// no reduction whose order depends on the launch.
#include "pgm_hip_common.h"
#include "pgm_lbp.h"

struct LbpArgs {
  const int32_t *node_off, *node_csr, *nbr_moff, *item_pair, *lead;
  const LbpPair *pairs;
  const LbpTable *tables;
  int32_t n_nodes, n_factors, n_tables, n_iter;
  int32_t n_unary, n_msg, n_theta_lds;
  int64_t n_theta;
  double tol, damping;
  const double *unaries, *theta, *state_in;
  double *marginals, *values;
  int32_t *iters;
  double *factor_beliefs, *state_out;
};

// Phase 1, the cavities: cell (pair (f, u), state x) = phi_u(x) times the messages into u from its other pairs, in
// the order of the node's incidence list.  An explicit product: a zero stays a zero, nothing is divided out.
__device__ __forceinline__ void lbp_cavities(const LbpArgs &a, const double *un, const double *cur, double *cav) {
  for (int32_t i = (int32_t)threadIdx.x; i < a.n_msg; i += kLbpBlock) {
    const LbpPair &P = a.pairs[a.item_pair[i]];
    const int32_t moff = P.moff, x = i - moff;
    double c = un[P.uoff + x];
    for (int32_t q = P.csr0, q1 = P.csr1; q < q1; ++q) {
      const int32_t m = a.nbr_moff[q];
      if (m != moff) c *= cur[m + x];
    }
    cav[i] = c;
  }
}

// The wave's 64 values of `sum` added in a butterfly (every lane ends with the same bits: each stage adds the same two
// values on both sides) and the four wave totals added in wave order; `top` is the maximum over the workgroup.  Fixed
// by kLbpBlock alone.  Two barriers: the pad may be written again right after the call.
__device__ __forceinline__ void lbp_reduce(double *pad, double &sum, double &top) {
  for (int x = 32; x > 0; x >>= 1) {
    sum += __shfl_xor(sum, x);
    const double o = __shfl_xor(top, x);
    top = o > top ? o : top;
  }
  const int32_t tid = (int32_t)threadIdx.x;
  if ((tid & 63) == 0) pad[tid >> 6] = sum, pad[4 + (tid >> 6)] = top;
  __syncthreads();
  sum = ((pad[0] + pad[1]) + pad[2]) + pad[3];
  top = pad[4];
  for (int w = 5; w < 8; ++w) top = pad[w] > top ? pad[w] : top;
  __syncthreads();
}

// Workgroup b runs instance b.  Dynamic LDS as lbp_lds_bytes lays it out.  THETA_LDS: the unique tables are copied to
// LDS once; otherwise the tables are read through the caches, which every instance of the launch shares.
template <bool THETA_LDS>
__global__ __launch_bounds__(kLbpBlock) void k_lbp(LbpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t tid = (int32_t)threadIdx.x;
  double *un = reinterpret_cast<double *>(smem);  // [n_unary]: the node terms
  double *cur = un + a.n_unary;                   // [n_msg]: the messages factor -> variable, each summing to 1
  double *cav = cur + a.n_msg;                    // [n_msg]: the cavities variable -> factor
  double *raw = cav + a.n_msg;                    // [n_msg]: the unnormalised new messages
  double *th_lds = raw + a.n_msg;
  double *pad = th_lds + (THETA_LDS ? a.n_theta_lds : 0);
  const double *th = THETA_LDS ? th_lds : a.theta;
  const int64_t b = blockIdx.x;

  for (int32_t i = tid; i < a.n_unary; i += kLbpBlock) un[i] = a.unaries[b * a.n_unary + i];
  if (a.state_in)
    for (int32_t i = tid; i < a.n_msg; i += kLbpBlock) cur[i] = a.state_in[b * a.n_msg + i];
  else
    for (int32_t i = tid; i < a.n_msg; i += kLbpBlock) cur[i] = 1.0 / (double)a.pairs[a.item_pair[i]].card;
  if constexpr (THETA_LDS)
    for (int32_t t = 0; t < a.n_tables; ++t) {
      const LbpTable T = a.tables[t];
      for (int32_t i = tid; i < T.size; i += kLbpBlock) th_lds[T.dst + i] = a.theta[T.src + i];
    }
  __syncthreads();

  const double keep = 1.0 - a.damping;
  double residual = (double)NAN, bad = 0.0;
  int32_t used = 0;
  for (int32_t it = 0; it < a.n_iter; ++it) {
    lbp_cavities(a, un, cur, cav);
    __syncthreads();
    // 2. the messages: cell (pair (f, v), state x) = the sum over the joint states of the factor's other variables,
    //    in ascending flat order, of psi_f times their cavities
    for (int32_t i = tid; i < a.n_msg; i += kLbpBlock) {
      const LbpPair &P = a.pairs[a.item_pair[i]];
      const int32_t nv = P.nv, n0 = P.n0, n1 = P.n1, s0 = P.s0, s1 = P.s1, c0 = P.c0, c1 = P.c1;
      const int32_t base = P.off_th + (i - P.moff) * P.sv;
      double acc = 0.0;
      for (int32_t x0 = 0; x0 < n0; ++x0) {
        const double k0 = nv > 1 ? cav[c0 + x0] : 1.0;
        for (int32_t x1 = 0; x1 < n1; ++x1) {
          double t = th[base + x0 * s0 + x1 * s1] * k0;
          if (nv > 2) t *= cav[c1 + x1];
          acc += t;
        }
      }
      raw[i] = acc;
    }
    __syncthreads();
    // 3. normalise, damp, residual; a message that sums to 0 is a contradiction
    double r = 0.0, sum = 0.0;
    for (int32_t i = tid; i < a.n_msg; i += kLbpBlock) {
      const LbpPair &P = a.pairs[a.item_pair[i]];
      const int32_t moff = P.moff, n = P.card;
      double z = 0.0;
      for (int32_t k = 0; k < n; ++k) z += raw[moff + k];
      if (!(z > 0.0)) {
        bad = 1.0;
        continue;
      }
      const double old = cur[i], now = keep * (raw[i] / z) + a.damping * old;
      cur[i] = now;
      const double d = fabs(now - old);
      r = d > r ? d : r;
    }
    double top = bad > 0.0 ? (double)INFINITY : r;  // one maximum carries both: a contradiction is an infinite residual
    lbp_reduce(pad, sum, top);
    used = it + 1, residual = top;
    if (top == (double)INFINITY) bad = 1.0;
    if (bad > 0.0 || top < a.tol) break;  // the same on every work-item
  }

  if (a.state_out)
    for (int32_t i = tid; i < a.n_msg; i += kLbpBlock) a.state_out[b * a.n_msg + i] = cur[i];
  lbp_cavities(a, un, cur, cav);  // from the final messages
  __syncthreads();

  // the node beliefs and their share of the Bethe value: sum of b (log phi - (1 - deg) log b), 0 log 0 = 0
  double part = 0.0;
  double *marg = a.marginals + b * a.n_unary;
  for (int32_t v = tid; v < a.n_nodes; v += kLbpBlock) {
    const int32_t o = a.node_off[v], n = a.node_off[v + 1] - o, q0 = a.node_csr[v], q1 = a.node_csr[v + 1];
    double z = 0.0;
    for (int32_t x = 0; x < n; ++x) {
      double c = un[o + x];
      for (int32_t q = q0; q < q1; ++q) c *= cur[a.nbr_moff[q] + x];
      marg[o + x] = c;
      z += c;
    }
    if (!(z > 0.0)) {
      bad = 1.0;
      continue;
    }
    const double w = (double)(1 - (q1 - q0));
    double t = 0.0;
    for (int32_t x = 0; x < n; ++x) {
      const double p = marg[o + x] / z;  // this work-item's own write
      marg[o + x] = p;
      if (p > 0.0) t += p * (log(un[o + x]) - w * log(p));
    }
    part += t;
  }
  __syncthreads();  // the messages are read no more: cur takes the factors' second partial sum

  // the factor beliefs u = psi times the cavities of its variables, unnormalised: one work-item per state of the
  // factor's first variable adds A = sum u and D = - sum u log(the cavities' product) over the other variables, then
  // one work-item per factor adds those in ascending order: its share is sum b log(psi / b) = D / A + log A
  for (int32_t i = tid; i < a.n_msg; i += kLbpBlock) {
    const LbpPair &P = a.pairs[a.item_pair[i]];
    if (P.pos != 0) continue;
    const int32_t nv = P.nv, n0 = P.n0, n1 = P.n1, s0 = P.s0, s1 = P.s1, c0 = P.c0, c1 = P.c1;
    const int32_t base = P.off_th + (i - P.moff) * P.sv;
    const double k = cav[i];
    double A = 0.0, D = 0.0;
    for (int32_t x0 = 0; x0 < n0; ++x0) {
      const double k0 = nv > 1 ? k * cav[c0 + x0] : k;
      for (int32_t x1 = 0; x1 < n1; ++x1) {
        const double kk = nv > 2 ? k0 * cav[c1 + x1] : k0, u = th[base + x0 * s0 + x1 * s1] * kk;
        if (u > 0.0) A += u, D -= u * log(kk);
      }
    }
    raw[i] = A, cur[i] = D;
  }
  __syncthreads();
  for (int32_t f = tid; f < a.n_factors; f += kLbpBlock) {
    const LbpPair &P = a.pairs[a.lead[f]];
    const int32_t moff = P.moff, n = P.card;
    double A = 0.0, D = 0.0;
    for (int32_t k = 0; k < n; ++k) A += raw[moff + k], D += cur[moff + k];
    raw[moff] = A;  // only this work-item read it; the factor's normaliser from here on
    if (A > 0.0) part += D / A + log(A);
    else bad = 1.0;
  }
  lbp_reduce(pad, part, bad);

  if (bad > 0.0) {  // the same on every work-item: this row is a contradiction
    for (int32_t i = tid; i < a.n_unary; i += kLbpBlock) marg[i] = (double)NAN;
    if (a.factor_beliefs)
      for (int64_t i = tid; i < a.n_theta; i += kLbpBlock) a.factor_beliefs[b * a.n_theta + i] = (double)NAN;
  } else if (a.factor_beliefs) {
    double *fb = a.factor_beliefs + b * a.n_theta;
    for (int32_t i = tid; i < a.n_msg; i += kLbpBlock) {
      const LbpPair &P = a.pairs[a.item_pair[i]];
      if (P.pos != 0) continue;
      const int32_t nv = P.nv, n0 = P.n0, n1 = P.n1, s0 = P.s0, s1 = P.s1, c0 = P.c0, c1 = P.c1;
      const int32_t row = (i - P.moff) * P.sv, base = P.off_th + row, out = P.off_out + row;
      const double k = cav[i], z = raw[P.moff];
      for (int32_t x0 = 0; x0 < n0; ++x0) {
        const double k0 = nv > 1 ? k * cav[c0 + x0] : k;
        for (int32_t x1 = 0; x1 < n1; ++x1) {
          const double kk = nv > 2 ? k0 * cav[c1 + x1] : k0;
          fb[out + x0 * s0 + x1 * s1] = th[base + x0 * s0 + x1 * s1] * kk / z;
        }
      }
    }
  }
  if (tid == 0) {
    double *val = a.values + b * PGM_LBP_VALUES;
    val[0] = bad > 0.0 ? (double)NAN : part, val[1] = bad > 0.0 ? (double)NAN : residual;
    a.iters[b] = bad > 0.0 ? -1 : used;
  }
}

// ---------------------------------------------------------------------------- the handle's device side
static int lbp_use(LbpHandle *h) {
  const LbpPlan &p = h->p;
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_node_off, p.node_off),   pgmdev::upload(h->d_node_csr, p.node_csr),
                               pgmdev::upload(h->d_nbr_moff, p.nbr_moff),   pgmdev::upload(h->d_item_pair, p.item_pair),
                               pgmdev::upload(h->d_lead, p.lead),           pgmdev::upload(h->d_pairs, p.pairs),
                               pgmdev::upload(h->d_tables, p.tables)};
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_lbp_plan_destroy(void *plan) { return pgm_plan_destroy<LbpHandle>(plan); }

int pgm_lbp_run(void *plan, const double *unaries, const double *theta, int64_t n_rows, int32_t n_iter, double tol,
                double damping, const double *state_in, double *marginals, double *values, int32_t *iters,
                double *factor_beliefs, double *state_out, void *stream) {
  LbpHandle *h = static_cast<LbpHandle *>(plan);
  bool launch = false;
  const int st = lbp_run_check(h, unaries, theta, n_rows, n_iter, tol, damping, state_in, marginals, values, iters,
                               factor_beliefs, state_out, &launch);
  if (st != PGM_OK || !launch) return st;
  const LbpPlan &p = h->p;
  const int up = lbp_use(h);
  if (up != PGM_OK) return up;
  const void *kernel = p.theta_in_lds ? reinterpret_cast<const void *>(&k_lbp<true>) : reinterpret_cast<const void *>(&k_lbp<false>);
  // above 64 KiB of dynamic LDS a kernel has to be told so before the launch
  if (p.lds_bytes > 65536) HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  LbpArgs a = {};
  a.node_off = h->d_node_off, a.node_csr = h->d_node_csr, a.nbr_moff = h->d_nbr_moff, a.item_pair = h->d_item_pair;
  a.lead = h->d_lead, a.pairs = h->d_pairs, a.tables = h->d_tables;
  a.n_nodes = p.n_nodes, a.n_factors = p.n_factors, a.n_tables = p.n_tables_unique, a.n_iter = n_iter;
  a.n_unary = (int32_t)p.n_unary, a.n_msg = (int32_t)p.n_msg, a.n_theta_lds = (int32_t)p.n_theta_unique, a.n_theta = p.n_theta;
  a.tol = tol, a.damping = damping;
  a.unaries = unaries, a.theta = theta, a.state_in = state_in;
  a.marginals = marginals, a.values = values, a.iters = iters, a.factor_beliefs = factor_beliefs, a.state_out = state_out;
  const dim3 grid((unsigned)n_rows), wg(kLbpBlock);
  if (p.theta_in_lds) hipLaunchKernelGGL(k_lbp<true>, grid, wg, (size_t)p.lds_bytes, S(stream), a);
  else hipLaunchKernelGGL(k_lbp<false>, grid, wg, (size_t)p.lds_bytes, S(stream), a);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

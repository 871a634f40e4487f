// pgmmd.hip — junction-tree potentials fitted to measured marginals by entropic mirror descent, on the device
// (gfx950): k_md runs a whole batch of instances, one workgroup each, through every iteration, every line-search
// trial and the log-space calibration of every trial in one launch, with the potentials, the trial log-beliefs, the
// messages and the per-marginal vectors in LDS throughout (or the tables in the instance's slice of a global slab
// when they do not fit); and the C-ABI (pgm_md_plan_destroy, pgm_md_run).  The contract is include/pgmhip.h
// "Junction-tree potentials by mirror descent"; the host side (validation, rooted tree, jobs, projections, item
// lists, tier, argument checks, pgm_md_plan_info) is pgmmd_plan.cpp.  fp64 and integers only; no matrix instruction
// (a log-sum-exp is no multiply-add), no atomic, no reduction whose order depends on the launch.
#include "pgm_hip_common.h"
#include "pgm_md.h"

struct MdArgs {
  const MdJob *jobs;
  const MdProj *projs;
  const MdAdd *adds;
  const MdPhase *phases;
  const int32_t *items;
  int32_t n_cliques, n_phases, n_cells, n_sep, n_y, root_tab, root_size;
  int32_t metric, iterations, line_search, fixed_step;  // fixed_step: alpha = stepsize, else 1 / total^2
  int64_t theta_stride, state_len;
  double stepsize;
  const double *targets, *totals, *theta_in;
  double *scratch, *theta_out, *mu_out, *values;
  int32_t *trials;
};

// the state of an instance: tables and messages (LDS or the global slice), the per-marginal vectors and the pad (LDS)
struct MdState {
  double *om, *bel, *up, *dn;  // omega and the trial log-beliefs [n_cells]; the messages child -> parent and back [n_sep]
  double *y, *g, *nu2, *m2;    // targets, gradient at omega, the marginals at omega and of the trial [n_y]
  double *pad;
};

// The wave's 64 values added in a butterfly (every lane ends with the same bits), the four wave totals added in wave
// order; fixed by kMdBlock alone.  Two barriers: the pad may be written again right after the call.
__device__ __forceinline__ void md_sum2(double *pad, double &s0, double &s1) {
  for (int x = 32; x > 0; x >>= 1) s0 += __shfl_xor(s0, x), s1 += __shfl_xor(s1, x);
  const int32_t tid = (int32_t)threadIdx.x;
  if ((tid & 63) == 0) pad[tid >> 6] = s0, pad[4 + (tid >> 6)] = s1;
  __syncthreads();
  s0 = ((pad[0] + pad[1]) + pad[2]) + pad[3];
  s1 = ((pad[4] + pad[5]) + pad[6]) + pad[7];
  __syncthreads();
}
__device__ __forceinline__ double md_wave_max(double v) {
  for (int x = 32; x > 0; x >>= 1) {
    const double o = __shfl_xor(v, x);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ double md_max(double *pad, double v) {
  v = md_wave_max(v);
  const int32_t tid = (int32_t)threadIdx.x;
  if ((tid & 63) == 0) pad[tid >> 6] = v;
  __syncthreads();
  v = pad[0];
  for (int w = 1; w < 4; ++w) v = pad[w] > v ? pad[w] : v;
  __syncthreads();
  return v;
}

// the sum over the projections [p0, p1) of table cell x, in their order
__device__ __forceinline__ double md_proj_sum(const MdArgs &a, int32_t x, int32_t p0, int32_t p1, const double *src) {
  double s = 0.0;
  for (int32_t q = p0; q < p1; ++q) {
    const MdProj &P = a.projs[q];
    int32_t idx = P.off;
    for (int32_t k = 0; k < P.nv; ++k) idx += ((x / P.st[k]) % P.card[k]) * P.ss[k];
    s += src[idx];
  }
  return s;
}

// dst = omega - alpha dL on every table: dL(x) is gathered from the gradient vectors of the clique's marginals
__device__ __forceinline__ void md_step(const MdArgs &a, const MdState &s, double *dst, double alpha) {
  for (int32_t c = 0; c < a.n_cliques; ++c) {
    const MdAdd A = a.adds[c];
    for (int32_t x = (int32_t)threadIdx.x; x < A.size; x += kMdBlock)
      dst[A.tab + x] = s.om[A.tab + x] - alpha * md_proj_sum(a, x, A.p0, A.p1, s.g);
  }
}

__device__ __forceinline__ int32_t md_cell(const int32_t *card, const int32_t *from, const int32_t *to, int32_t n, int32_t i) {
  int32_t off = 0;
  for (int32_t k = 0; k < n; ++k) off += ((i / from[k]) % card[k]) * to[k];
  return off;
}

// The reductions of a phase.  An item is one output cell of one job: log sum exp of the trial log-beliefs over the
// cells of the job's table that share the output cell, maximum first, then the sum of exp(v - maximum) in ascending
// order of the residual (one work-item), or lane l adding the cells l, l + 64, .. and a butterfly over the wave.
__device__ __forceinline__ void md_reduce(const MdArgs &a, const MdState &s, const MdPhase &ph, double shift) {
  const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63;
  // the lane items by work-item, then the wave items by wave: one loop, `wide` says which
  for (int pass = 0; pass < 2; ++pass) {
    const bool wide = pass == 1;
    const int32_t first = wide ? ph.wave0 : ph.lane0, count = wide ? ph.wave_n : ph.lane_n;
    for (int32_t i = wide ? tid >> 6 : tid; i < count; i += wide ? kMdBlock / 64 : kMdBlock) {
      const int32_t j = a.items[first + i];
      const MdJob &J = a.jobs[j];
      const int32_t cell = first + i - J.item0;
      const double *tab = s.bel + J.tab + md_cell(J.kc, J.ks, J.kt, J.nk, cell);
      const int32_t r0 = wide ? lane : 0, dr = wide ? 64 : 1;
      double top = -(double)INFINITY, sum = 0.0;
      for (int32_t r = r0; r < J.n_res; r += dr) {
        const double v = tab[md_cell(J.rc, J.rs, J.rt, J.nr, r)];
        top = v > top ? v : top;
      }
      if (wide) top = md_wave_max(top);
      for (int32_t r = r0; r < J.n_res; r += dr) {
        const double v = tab[md_cell(J.rc, J.rs, J.rt, J.nr, r)];
        sum += top == -(double)INFINITY ? 0.0 : exp(v - top);
      }
      if (wide)
        for (int x = 32; x > 0; x >>= 1) sum += __shfl_xor(sum, x);
      const double lse = top == -(double)INFINITY ? top : top + log(sum);
      if (wide && lane != 0) continue;
      const int32_t o = J.out + cell;
      if (ph.kind == kMdUp) s.up[o] = lse;
      else if (ph.kind == kMdDown) s.dn[o] = lse - s.up[o];
      else s.m2[o] = exp(lse + shift);
    }
  }
}

// every table cell of the phase's cliques takes the messages that reached the clique in this phase
__device__ __forceinline__ void md_add(const MdArgs &a, const MdState &s, const MdPhase &ph, const double *msg) {
  for (int32_t q = ph.a0; q < ph.a1; ++q) {
    const MdAdd A = a.adds[q];
    for (int32_t x = (int32_t)threadIdx.x; x < A.size; x += kMdBlock) s.bel[A.tab + x] += md_proj_sum(a, x, A.p0, A.p1, msg);
  }
}

// One calibration of theta = omega - alpha dL in log space: the trial log-beliefs of every clique, log Z at the root,
// the trial's marginals m2, its loss and the Armijo dot product dL . (nu - mu) = sum g (nu2 - m2).  The same values on
// every work-item.  Ends behind a barrier.
__device__ __forceinline__ void md_calibrate(const MdArgs &a, const MdState &s, double alpha, double logn, double &logz,
                                             double &loss, double &dot) {
  const int32_t tid = (int32_t)threadIdx.x;
  md_step(a, s, s.bel, alpha);
  __syncthreads();
  for (int32_t p = 0; p < a.n_phases; ++p) {
    const MdPhase ph = a.phases[p];
    if (ph.kind == kMdAddUp) md_add(a, s, ph, s.up);
    else if (ph.kind == kMdAddDown) md_add(a, s, ph, s.dn);
    else if (ph.kind == kMdLogZ) {
      const double *root = s.bel + a.root_tab;
      double top = -(double)INFINITY, sum = 0.0, none = 0.0;
      for (int32_t x = tid; x < a.root_size; x += kMdBlock) top = root[x] > top ? root[x] : top;
      top = md_max(s.pad, top);
      for (int32_t x = tid; x < a.root_size; x += kMdBlock) sum += top == -(double)INFINITY ? 0.0 : exp(root[x] - top);
      md_sum2(s.pad, sum, none);
      logz = top == -(double)INFINITY ? top : top + log(sum);
    } else md_reduce(a, s, ph, logn - logz);
    __syncthreads();
  }
  loss = 0.0, dot = 0.0;
  for (int32_t j = tid; j < a.n_y; j += kMdBlock) {
    const double d = s.m2[j] - s.y[j];
    loss += a.metric == PGM_MD_L2 ? 0.5 * d * d : fabs(d);
    dot += s.g[j] * (s.nu2[j] - s.m2[j]);
  }
  md_sum2(s.pad, loss, dot);
}

// the trial becomes the point: omega = omega - alpha dL (with the gradient the trial was made from), then the
// gradient and the marginals of the new point
__device__ __forceinline__ void md_accept(const MdArgs &a, const MdState &s, double alpha) {
  md_step(a, s, s.om, alpha);
  __syncthreads();
  for (int32_t j = (int32_t)threadIdx.x; j < a.n_y; j += kMdBlock) {
    const double d = s.m2[j] - s.y[j];
    s.g[j] = a.metric == PGM_MD_L2 ? d : d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d;  // the sign of 0 is 0 (of NaN, NaN)
    s.nu2[j] = s.m2[j];
  }
  __syncthreads();
}

// Workgroup b runs instance b.  Dynamic LDS as md_lds_bytes lays it out.  TABLES_LDS: the tables and messages are in
// LDS; otherwise in slice b of the scratch slab, which only this workgroup touches.
template <bool TABLES_LDS>
__global__ __launch_bounds__(kMdBlock) void k_md(MdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int32_t tid = (int32_t)threadIdx.x;
  const int64_t b = blockIdx.x;
  double *lds = reinterpret_cast<double *>(smem);
  MdState s;
  s.om = TABLES_LDS ? lds : a.scratch + b * a.state_len;
  s.bel = s.om + a.n_cells, s.up = s.bel + a.n_cells, s.dn = s.up + a.n_sep;
  s.y = TABLES_LDS ? s.dn + a.n_sep : lds;
  s.g = s.y + a.n_y, s.nu2 = s.g + a.n_y, s.m2 = s.nu2 + a.n_y, s.pad = s.m2 + a.n_y;

  const double *th = a.theta_in + b * a.theta_stride;
  for (int32_t i = tid; i < a.n_cells; i += kMdBlock) s.om[i] = th[i];
  for (int32_t j = tid; j < a.n_y; j += kMdBlock) s.y[j] = a.targets[b * a.n_y + j], s.g[j] = 0.0, s.nu2[j] = 0.0;
  __syncthreads();

  const double total = a.totals[b], logn = log(total);
  double alpha = a.fixed_step ? a.stepsize : 1.0 / (total * total);
  double logz = 0.0, curr = 0.0, dot = 0.0;
  md_calibrate(a, s, 0.0, logn, logz, curr, dot);  // the start: theta = omega
  md_accept(a, s, 0.0);
  int32_t n_trials = 0, n_rejected = 0;
  for (int32_t it = 0; it < a.iterations; ++it) {
    if (a.line_search) alpha *= 2.0;
    double used = alpha, now = curr;
    for (int32_t t = 0; t < kMdTrials; ++t) {
      used = alpha;
      md_calibrate(a, s, used, logn, logz, now, dot);
      ++n_trials;
      if (!a.line_search || curr - now >= 0.5 * used * dot) break;  // the same on every work-item
      alpha *= 0.5, ++n_rejected;
    }
    md_accept(a, s, used);  // after kMdTrials rejections the last trial is kept all the same
    curr = now;
  }

  for (int32_t i = tid; i < a.n_cells; i += kMdBlock) {
    a.theta_out[b * a.n_cells + i] = s.om[i];
    a.mu_out[b * a.n_cells + i] = exp(s.bel[i] + logn - logz);
  }
  if (tid == 0) {
    a.values[b * PGM_MD_VALUES] = curr, a.values[b * PGM_MD_VALUES + 1] = alpha;
    a.trials[b * 2] = n_trials, a.trials[b * 2 + 1] = n_rejected;
  }
}

// ---------------------------------------------------------------------------- the handle's device side
static int md_use(MdHandle *h) {
  const MdPlan &p = h->p;
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_jobs, p.jobs), pgmdev::upload(h->d_projs, p.projs), pgmdev::upload(h->d_adds, p.adds),
                               pgmdev::upload(h->d_phases, p.phases), pgmdev::upload(h->d_items, p.items)};
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_md_plan_destroy(void *plan) { return pgm_plan_destroy<MdHandle>(plan); }

int pgm_md_run(void *plan, const double *targets, const double *totals, const double *theta_in, int64_t theta_rows,
               int64_t n_rows, int32_t metric, int32_t iterations, double stepsize, int32_t step_mode, double *scratch,
               double *theta_out, double *mu_out, double *values, int32_t *trials, void *stream) {
  MdHandle *h = static_cast<MdHandle *>(plan);
  bool launch = false;
  const int st = md_run_check(h, targets, totals, theta_in, theta_rows, n_rows, metric, iterations, stepsize, step_mode,
                              scratch, theta_out, mu_out, values, trials, &launch);
  if (st != PGM_OK || !launch) return st;
  const MdPlan &p = h->p;
  const int up = md_use(h);
  if (up != PGM_OK) return up;
  const bool lds = p.tier == PGM_MD_TIER_LDS;
  const void *kernel = lds ? reinterpret_cast<const void *>(&k_md<true>) : reinterpret_cast<const void *>(&k_md<false>);
  // above 64 KiB of dynamic LDS a kernel has to be told so before the launch
  if (p.lds_bytes > 65536) HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  MdArgs a = {};
  a.jobs = h->d_jobs, a.projs = h->d_projs, a.adds = h->d_adds, a.phases = h->d_phases, a.items = h->d_items;
  a.n_cliques = p.n_cliques, a.n_phases = (int32_t)p.phases.size(), a.n_cells = (int32_t)p.n_cells, a.n_sep = (int32_t)p.n_sep;
  a.n_y = (int32_t)p.n_y, a.root_tab = p.root_tab, a.root_size = p.root_size;
  a.metric = metric, a.iterations = iterations, a.line_search = step_mode == PGM_MD_STEP_SEARCH;
  a.fixed_step = step_mode == PGM_MD_STEP_FIXED;
  a.theta_stride = theta_rows == 1 ? 0 : p.n_cells, a.state_len = p.state_len, a.stepsize = stepsize;
  a.targets = targets, a.totals = totals, a.theta_in = theta_in;
  a.scratch = scratch, a.theta_out = theta_out, a.mu_out = mu_out, a.values = values, a.trials = trials;
  const dim3 grid((unsigned)n_rows), wg(kMdBlock);
  if (lds) hipLaunchKernelGGL(k_md<true>, grid, wg, (size_t)p.lds_bytes, S(stream), a);
  else hipLaunchKernelGGL(k_md<false>, grid, wg, (size_t)p.lds_bytes, S(stream), a);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

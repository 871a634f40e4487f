// pgmlogp.hip — the per-row log-probability of complete rows under a Bayesian network on the device
// (gfx950): the kernels behind pgmpy_amd.metrics.BayesianModelProbability / log_likelihood_score and their
// C-ABI (pgm_fit_log_values, pgm_fit_logprob).  Replaces the reference's per-node np.unique(axis=0) and
// Python loop over the rows (metrics/bn_inference.py:23-126).  The entry points live on the fit plan: the
// host side (argument checks, pgm_fit_logprob_info) is pgmfit_plan.cpp, the handle's device side is
// pgmfit.hip's fit_use.
#include <cmath>

#include "pgm_fit.h"
#include "pgm_hip_common.h"

// ---------------------------------------------------------------------------- log tables
// One work-item per entry of the flat layout.  values and logv may be the same buffer (each entry is read
// and written by its own work-item), so neither is __restrict__.  log(0) = -inf; a negative or NaN value
// raises *err.
__global__ __launch_bounds__(kLogpBlock) void k_fit_log_values(const double *values, double *logv, int64_t n,
                                                               int32_t *__restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * kLogpBlock + threadIdx.x;
  if (i >= n) return;
  const double v = values[i];
  if (!(v >= 0.0)) atomicOr(err, 1);
  logv[i] = log(v);
}

// ---------------------------------------------------------------------------- per-row sums
// code loads issued two families ahead: a node and three parents; the variables past them are loaded
// where they are used
static constexpr int kLogpPrefetch = 4;
static_assert(kLogpPrefetch <= PGM_MAX_DIMS, "prefetch slots index FitFam::col");

// N rows of one lane through every family in plan order (N = 4: the 4 codes of a column are one aligned
// dword; N = 1: one byte), pgm_sample_forward's walk as a reduction.  `at` is the first row's index in the
// buffer (row0 + r).  out[j] is row j's sum, added family by family from +0.0 (the same sequence of fp64
// additions for either N), or NaN for a skipped row; returns the mask of skipped rows and sets bad when a
// code was neither a state nor PGM_EV_MISSING.  A skipped row loads nothing more from logv: no index is
// made from a code >= its cardinality.  n_fam >= 1 (a plan has at least one family).
template <int N>
__device__ __forceinline__ uint32_t logp_walk(const FitFam *__restrict__ fams, int32_t n_fam,
                                              const double *__restrict__ logv, const uint8_t *__restrict__ codes,
                                              int64_t ld, int64_t at, double (&out)[N], bool &bad) {
  static_assert(N == 1 || N == 4, "a byte or a dword of codes");
  double acc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) acc[j] = 0.0;
  uint32_t skip = 0;  // bit j: row j holds a code that is no state
  auto load = [&](int32_t col) -> uint32_t {
    const uint8_t *p = codes + (int64_t)col * ld + at;
    if constexpr (N == 4) return *reinterpret_cast<const uint32_t *>(p);
    else return *p;
  };
  // Three families are in flight per lane: the codes of family f + 2 are being loaded (its first
  // kLogpPrefetch variables, always that many loads without a branch: a slot past n_vars reloads the node's
  // column and is not used), the table entries of family f + 1 are being gathered, and family f's are
  // added.  So a family costs the longest of the three round trips, not their sum, and its code loads are
  // in flight together.  Past the last family the stages repeat it (clamped index): the same codes and
  // entries again, not added.
  auto prefetch = [&](const FitFam &G, uint32_t (&qq)[kLogpPrefetch]) {
#pragma unroll
    for (int k = 0; k < kLogpPrefetch; ++k) qq[k] = load(k < G.n_vars ? G.col[k] : G.col[0]);
  };
  // family F's entry of every row from its codes qq; 0.0 for a row that is skipped by now (never added to
  // a value that is kept: the row ends as NaN)
  auto gather = [&](const FitFam &F, const uint32_t (&qq)[kLogpPrefetch], double (&g)[N]) {
    const int32_t nv = F.n_vars;
    int32_t idx[N];
#pragma unroll
    for (int j = 0; j < N; ++j) idx[j] = 0;
    auto take = [&](uint32_t qv, int32_t v) {
      const uint32_t card = (uint32_t)F.card[v];
      const int32_t stride = F.stride[v];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const uint32_t c = (qv >> (8 * j)) & 255u;
        if (c >= card) {  // missing, or not a state
          bad |= c != PGM_EV_MISSING;
          skip |= 1u << j;
        } else {
          idx[j] += (int32_t)c * stride;
        }
      }
    };
#pragma unroll
    for (int k = 0; k < kLogpPrefetch; ++k)
      if (k < nv) take(qq[k], k);
    for (int32_t v = kLogpPrefetch; v < nv; ++v) take(load(F.col[v]), v);
    const double *t = logv + F.off;
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = (skip >> j & 1u) ? 0.0 : t[idx[j]];
  };
  const int32_t last = n_fam - 1;
  uint32_t q[kLogpPrefetch], nq[kLogpPrefetch];
  double g[N], ng[N];
  prefetch(fams[0], q);
  prefetch(fams[1 < last ? 1 : last], nq);
  gather(fams[0], q, g);
#pragma unroll
  for (int k = 0; k < kLogpPrefetch; ++k) q[k] = nq[k];
  for (int32_t f = 0; f < n_fam; ++f) {
    // q: the codes of family min(f + 1, last); g: the entries of family f
    prefetch(fams[f + 2 < last ? f + 2 : last], nq);  // workgroup-uniform descriptors: scalar loads
    gather(fams[f + 1 < last ? f + 1 : last], q, ng);
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] += g[j];
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = ng[j];
#pragma unroll
    for (int k = 0; k < kLogpPrefetch; ++k) q[k] = nq[k];
  }
#pragma unroll
  for (int j = 0; j < N; ++j) out[j] = (skip >> j & 1u) ? (double)NAN : acc[j];
  return skip;
}

// One launch sums every family of n_rows rows: workgroup b takes rows [b, b + 1) * kLogpRowsPerBlock.
// V4 (codes, ld and row0 multiples of 4: codes_vec4): lane t owns the 4 consecutive rows 4 t .. 4 t + 3 of
// the workgroup and loads their 4 codes of a column as one aligned dword, so a wave reads 256 contiguous
// bytes per column; the rows of the tail that do not fill a dword take the one-row path.  Else lane t
// takes the rows t, t + 256, t + 512, t + 768.  The log tables are gathered through the cache (DESIGN.md:
// no LDS staging).
// Either way row i of the workgroup leaves its value (+0.0 if skipped or past the window) in s_row[i], and
// the workgroup's partial is added from s_row in an order that depends on nothing else: work-item t adds
// s_row[t], s_row[t + 256], s_row[t + 512], s_row[t + 768] in that order, then the fixed tree.
template <bool V4>
__global__ __launch_bounds__(kLogpBlock) void k_fit_logprob(const FitFam *__restrict__ fams, int32_t n_fam,
                                                            const double *__restrict__ logv,
                                                            const uint8_t *__restrict__ codes, int64_t ld,
                                                            int64_t row0, int64_t n_rows, double *__restrict__ logp,
                                                            double *__restrict__ part, int32_t *__restrict__ part_skip,
                                                            int32_t *__restrict__ err) {
  __shared__ double s_row[kLogpRowsPerBlock];
  __shared__ double s_sum[kLogpBlock];
  __shared__ int32_t s_skipped;
  const int32_t tid = (int32_t)threadIdx.x;
  const int64_t r_begin = (int64_t)blockIdx.x * kLogpRowsPerBlock;
  const int64_t r_end = r_begin + kLogpRowsPerBlock < n_rows ? r_begin + kLogpRowsPerBlock : n_rows;
  if (tid == 0) s_skipped = 0;
  for (int32_t i = tid; i < kLogpRowsPerBlock; i += kLogpBlock) s_row[i] = 0.0;
  __syncthreads();
  constexpr int RPL = V4 ? 4 : 1;  // rows per lane and step
  bool bad = false;
  int32_t skipped = 0;
  for (int64_t r = r_begin + (int64_t)tid * RPL; r < r_end; r += kLogpBlock * RPL) {
    if (V4 && r + 4 <= r_end) {
      double v[4];
      const uint32_t skip = logp_walk<4>(fams, n_fam, logv, codes, ld, row0 + r, v, bad);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (logp) logp[row0 + r + j] = v[j];
        if (skip >> j & 1u) ++skipped;
        else s_row[(int32_t)(r - r_begin) + j] = v[j];
      }
      continue;
    }
    const int64_t r_stop = r + RPL < r_end ? r + RPL : r_end;
    for (int64_t rr = r; rr < r_stop; ++rr) {
      double v[1];
      const uint32_t skip = logp_walk<1>(fams, n_fam, logv, codes, ld, row0 + rr, v, bad);
      if (logp) logp[row0 + rr] = v[0];
      if (skip) ++skipped;
      else s_row[(int32_t)(rr - r_begin)] = v[0];
    }
  }
  if (bad) atomicOr(err, 1);
  if (skipped) atomicAdd(&s_skipped, skipped);  // an integer: exact in any order
  __syncthreads();
  double sum = s_row[tid];
  for (int32_t k = 1; k < kLogpRowsPerBlock / kLogpBlock; ++k) sum += s_row[tid + k * kLogpBlock];
  s_sum[tid] = sum;
  __syncthreads();
  for (int32_t w = kLogpBlock / 2; w > 0; w >>= 1) {
    if (tid < w) s_sum[tid] += s_sum[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    part[blockIdx.x] = s_sum[0];
    part_skip[blockIdx.x] = s_skipped;
  }
}

// One workgroup adds the block partials: work-item t takes partials t, t + 256, ... in index order, then
// the same fixed tree (k_fit_score_sum's shape).
__global__ __launch_bounds__(kLogpBlock) void k_fit_logprob_sum(const double *__restrict__ part,
                                                                const int32_t *__restrict__ part_skip, int32_t n,
                                                                double *__restrict__ total,
                                                                int64_t *__restrict__ n_skipped) {
  __shared__ double s_sum[kLogpBlock];
  __shared__ int64_t s_skip[kLogpBlock];
  const int32_t tid = (int32_t)threadIdx.x;
  double sum = 0.0;
  int64_t skip = 0;
  for (int32_t i = tid; i < n; i += kLogpBlock) {
    sum += part[i];
    skip += part_skip[i];
  }
  s_sum[tid] = sum;
  s_skip[tid] = skip;
  __syncthreads();
  for (int32_t w = kLogpBlock / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_sum[tid] += s_sum[tid + w];
      s_skip[tid] += s_skip[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (total) *total = s_sum[0];
    if (n_skipped) *n_skipped = s_skip[0];
  }
}

extern "C" {

int pgm_fit_log_values(void *plan, const double *values, double *logv, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  int64_t blocks = 0;
  const int st = fit_log_values_check(h, values, logv, &blocks);
  if (st != PGM_OK) return st;
  int up = fit_use(h);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  hipLaunchKernelGGL(k_fit_log_values, dim3((unsigned)blocks), dim3(kLogpBlock), 0, S(stream), values, logv,
                     h->p.total_bins, h->dev.flag());
  // PGM_EINVAL is this call's status: the flag is read back after the launch (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad) return pgmi_fail(PGM_EINVAL, "fit_log_values: a value is negative or NaN");
  return PGM_OK;
}

int pgm_fit_logprob(void *plan, const double *logv, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                    int64_t n_rows, double *logp, double *total, int64_t *n_skipped, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  int64_t blocks = 0;
  const int st = fit_logprob_check(h, logv, codes, n_cols, ld, row0, n_rows, logp, total, n_skipped, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) {  // no rows: no launch
    if (total) HIP_TRY(hipMemsetAsync(total, 0, sizeof *total, S(stream)));
    if (n_skipped) HIP_TRY(hipMemsetAsync(n_skipped, 0, sizeof *n_skipped, S(stream)));
    return PGM_OK;
  }
  int up = fit_use(h, kFitLogp);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  const int32_t nf = (int32_t)h->p.fams.size();
  const dim3 grid((unsigned)blocks), wg(kLogpBlock);
  if (codes_vec4(codes, ld, row0))
    hipLaunchKernelGGL(k_fit_logprob<true>, grid, wg, 0, S(stream), h->d_fams, nf, logv, codes, ld, row0, n_rows, logp,
                       h->d_logp_part, h->d_logp_skip, h->dev.flag());
  else
    hipLaunchKernelGGL(k_fit_logprob<false>, grid, wg, 0, S(stream), h->d_fams, nf, logv, codes, ld, row0, n_rows, logp,
                       h->d_logp_part, h->d_logp_skip, h->dev.flag());
  HIP_TRY(hipGetLastError());
  if (total || n_skipped)
    hipLaunchKernelGGL(k_fit_logprob_sum, dim3(1), wg, 0, S(stream), h->d_logp_part, h->d_logp_skip, (int32_t)blocks, total,
                       n_skipped);
  // PGM_EINDEX is this call's status, as in pgm_fit_count (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad) return pgmi_fail(PGM_EINDEX, "fit_logprob: a state code is >= its variable's cardinality");
  return PGM_OK;
}
}

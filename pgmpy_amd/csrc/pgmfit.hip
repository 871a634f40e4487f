// pgmfit.hip — parameter learning on the device (gfx950): the family-count kernel and the CPD finishing
// kernel behind DiscreteBayesianNetwork.fit / fit_update, and their C-ABI (pgm_fit_plan_destroy,
// pgm_fit_count, pgm_fit_finish).  Replaces the reference's per-node pandas groupby
// (estimators/base.py:67-176) and the per-CPD normalisation (MLE.py:183-212, BayesianEstimator.py:252-264).
// The host side (validation, table layout, family groups, argument checks) is pgmfit_plan.cpp.
#include <mutex>
#include <type_traits>

#include "pgm_fit.h"
#include "pgm_hip_common.h"

// ---------------------------------------------------------------------------- counting
// One launch counts every family: workgroup b takes row chunk b / n_groups for family group
// b % n_groups.  Tile groups privatise their run of bins in LDS (LDS atomics per row), then add only the
// non-zero bins to the global tables: one global atomic per workgroup and bin, not one per row.  A global
// group (one family larger than the tile) adds straight into its global table.  A row whose code is
// PGM_EV_MISSING in any column of a family is skipped for that family only (the reference's groupby /
// value_counts drop NaN per family); a code >= the cardinality sets *err and is skipped too, so no
// index leaves the family's table.
// W = false: each row counts 1 (uint32 LDS bins, int64 tables: exact, order-independent).
// W = true:  each row counts weights[row0 + row] (fp64 LDS bins and tables: the order of addition varies).
// V4 = true (codes, ld and row0 all multiples of 4: fit_count_vec4): a lane takes 4 consecutive rows and
// loads their 4 codes of a column as one dword, so a family costs a quarter of the dependent load round
// trips; the rows of a chunk's tail that do not fill a dword take the one-row path.
template <bool W, bool V4>
__global__ __launch_bounds__(kFitBlock) void k_fit_count(const FitFam *__restrict__ fams,
                                                         const FitGroup *__restrict__ groups, uint32_t n_groups,
                                                         const uint8_t *__restrict__ codes, int64_t ld, int64_t row0,
                                                         int64_t n_rows, const double *__restrict__ weights,
                                                         void *__restrict__ tables, int32_t *__restrict__ err) {
  using Bin = typename std::conditional<W, double, uint32_t>::type;
  using Out = typename std::conditional<W, double, unsigned long long>::type;
  extern __shared__ unsigned char fit_lds[];
  Bin *lds = reinterpret_cast<Bin *>(fit_lds);
  const uint32_t tid = threadIdx.x;
  const FitGroup g = groups[blockIdx.x % n_groups];
  const int64_t r_begin = (int64_t)(blockIdx.x / n_groups) * kFitRowsPerBlock;
  const int64_t r_end = r_begin + kFitRowsPerBlock < n_rows ? r_begin + kFitRowsPerBlock : n_rows;
  Out *out = static_cast<Out *>(tables) + g.off;
  if (!g.global) {
    for (int32_t i = (int32_t)tid; i < g.bins; i += kFitBlock) lds[i] = Bin(0);
    __syncthreads();
  }
  bool bad = false;
  for (int32_t f = g.fam_begin; f < g.fam_end; ++f) {
    const FitFam &F = fams[f];
    const int32_t base = (int32_t)(F.off - g.off);  // 0 for a global group
    const int32_t nv = F.n_vars;
    auto add = [&](int32_t idx, int64_t r) {
      if (g.global) {
        if constexpr (W) atomicAdd(&out[idx], weights[row0 + r]);
        else atomicAdd(&out[idx], 1ull);
      } else {
        if constexpr (W) atomicAdd(&lds[base + idx], weights[row0 + r]);
        else atomicAdd(&lds[base + idx], 1u);
      }
    };
    constexpr int RPL = V4 ? 4 : 1;  // rows per lane and step
    for (int64_t r = r_begin + (int64_t)tid * RPL; r < r_end; r += kFitBlock * RPL) {
      if (V4 && r + 4 <= r_end) {
        int32_t idx[4] = {0, 0, 0, 0};
        uint32_t skip = 0;  // bit j: row r + j is not counted for this family
        for (int32_t v = 0; v < nv; ++v) {
          const uint32_t q = *reinterpret_cast<const uint32_t *>(codes + (int64_t)F.col[v] * ld + row0 + r);
          const uint32_t card = (uint32_t)F.card[v];
          const int32_t stride = F.stride[v];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t c = (q >> (8 * j)) & 255u;
            if (c >= card) {  // missing, or not a state
              bad |= c != PGM_EV_MISSING;
              skip |= 1u << j;
            } else {
              idx[j] += (int32_t)c * stride;
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!(skip >> j & 1u)) add(idx[j], r + j);
        continue;
      }
      const int64_t r_stop = r + RPL < r_end ? r + RPL : r_end;
      for (int64_t rr = r; rr < r_stop; ++rr) {
        int32_t idx = 0;
        bool skip = false;
        for (int32_t v = 0; v < nv; ++v) {
          const uint32_t c = codes[(int64_t)F.col[v] * ld + row0 + rr];
          if (c >= (uint32_t)F.card[v]) {  // missing, or not a state
            bad |= c != PGM_EV_MISSING;
            skip = true;
            break;
          }
          idx += (int32_t)c * F.stride[v];
        }
        if (!skip) add(idx, rr);
      }
    }
  }
  if (bad) atomicOr(err, 1);
  if (!g.global) {
    __syncthreads();
    for (int32_t i = (int32_t)tid; i < g.bins; i += kFitBlock) {
      const Bin v = lds[i];
      if (v != Bin(0)) atomicAdd(&out[i], (Out)v);
    }
  }
}

// ---------------------------------------------------------------------------- finishing
// One launch turns the count buffer into every CPD's values: one work-item per CPD column (a parent
// configuration of one family; the family is found by bisection over col_off).  v = count (+ pseudo);
// MLE: a column whose v are all zero becomes ones (MLE.py:187); then v / sum with the sum taken in state
// order (values / values.sum(axis=0), CPD.py normalize).  Bayes keeps 0/0 = NaN.
template <bool W>
__global__ __launch_bounds__(256) void k_fit_finish(const FitFam *__restrict__ fams,
                                                    const int64_t *__restrict__ col_off, int32_t n_fam,
                                                    const void *__restrict__ counts,
                                                    const double *__restrict__ pseudo, int32_t bayes,
                                                    double *__restrict__ values) {
  using Cnt = typename std::conditional<W, double, int64_t>::type;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= col_off[n_fam]) return;
  int32_t lo = 0, hi = n_fam;  // col_off[lo] <= c < col_off[hi]
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (col_off[mid] <= c) lo = mid;
    else hi = mid;
  }
  const FitFam &F = fams[lo];
  const int32_t card = F.card[0];
  const int64_t ncol = F.size / card;
  const int64_t at = F.off + (c - col_off[lo]);
  const Cnt *cnt = static_cast<const Cnt *>(counts);
  double sum = 0.0;
  bool all_zero = true;
  for (int32_t s = 0; s < card; ++s) {
    double v = (double)cnt[at + s * ncol];
    if (pseudo) v += pseudo[at + s * ncol];
    all_zero &= v == 0.0;
    sum += v;
  }
  const bool fill = !bayes && all_zero;
  if (fill) sum = (double)card;
  for (int32_t s = 0; s < card; ++s) {
    double v = (double)cnt[at + s * ncol];
    if (pseudo) v += pseudo[at + s * ncol];
    values[at + s * ncol] = (fill ? 1.0 : v) / sum;
  }
}

// ---------------------------------------------------------------------------- the handle's device side
static std::mutex g_fit_mu;

static void fit_free_device(FitHandle *h) {
  for (void **p : {&h->d_fams, &h->d_groups, &h->d_col_off, &h->d_err}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  h->device = -1;
}

// the descriptors on the current device (uploaded on first use; again when the device changes)
static int fit_upload(FitHandle *h) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_fit_mu);
  if (h->device == dev) return PGM_OK;
  fit_free_device(h);
  const FitPlan &p = h->p;
  const size_t nf = p.fams.size() * sizeof(FitFam), ng = p.groups.size() * sizeof(FitGroup);
  const size_t nc = p.col_off.size() * sizeof(int64_t);
  HIP_TRY(hipMalloc(&h->d_fams, nf));
  HIP_TRY(hipMalloc(&h->d_groups, ng));
  HIP_TRY(hipMalloc(&h->d_col_off, nc));
  HIP_TRY(hipMalloc(&h->d_err, sizeof(int32_t)));
  HIP_TRY(hipMemcpy(h->d_fams, p.fams.data(), nf, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_groups, p.groups.data(), ng, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_col_off, p.col_off.data(), nc, hipMemcpyHostToDevice));
  h->device = dev;
  return PGM_OK;
}

extern "C" {

int pgm_fit_plan_destroy(void *plan) {
  if (!plan) return PGM_OK;
  FitHandle *h = static_cast<FitHandle *>(plan);
  {
    std::lock_guard<std::mutex> lk(g_fit_mu);
    fit_free_device(h);
  }
  delete h;
  return PGM_OK;
}

int pgm_fit_count(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                  const double *weights, void *tables, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  int64_t blocks = 0;
  const int st = fit_count_check(h, codes, n_cols, ld, row0, n_rows, tables, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  const int up = fit_upload(h);
  if (up != PGM_OK) return up;
  int32_t *err = static_cast<int32_t *>(h->d_err);
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), S(stream)));
  const FitFam *fams = static_cast<const FitFam *>(h->d_fams);
  const FitGroup *groups = static_cast<const FitGroup *>(h->d_groups);
  const uint32_t ng = (uint32_t)h->p.groups.size();
  const dim3 grid((unsigned)blocks), wg(kFitBlock);
  const size_t lds = kFitTileBins * (weights ? sizeof(double) : sizeof(uint32_t));
  const bool v4 = fit_count_vec4(codes, ld, row0);
#define FIT_LAUNCH(W, V4)                                                                                        \
  hipLaunchKernelGGL((k_fit_count<W, V4>), grid, wg, lds, S(stream), fams, groups, ng, codes, ld, row0, n_rows, \
                     weights, tables, err)
  if (weights) {
    if (v4) FIT_LAUNCH(true, true);
    else FIT_LAUNCH(true, false);
  } else {
    if (v4) FIT_LAUNCH(false, true);
    else FIT_LAUNCH(false, false);
  }
#undef FIT_LAUNCH
  HIP_TRY(hipGetLastError());
  // PGM_EINDEX is this call's status: the flag is read back after the launch (synchronises the stream)
  int32_t bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, err, sizeof bad, hipMemcpyDeviceToHost, S(stream)));
  HIP_TRY(hipStreamSynchronize(S(stream)));
  if (bad) return pgmi_fail(PGM_EINDEX, "fit_count: a state code is >= its variable's cardinality");
  return PGM_OK;
}

int pgm_fit_finish(void *plan, const void *counts, const double *pseudo, int32_t mode, double *values, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  const int st = fit_finish_check(h, counts, mode, values);
  if (st != PGM_OK) return st;
  const int up = fit_upload(h);
  if (up != PGM_OK) return up;
  const int64_t cols = h->p.col_off.back();
  const int64_t blocks = (cols + 255) / 256;
  if (blocks > INT32_MAX) return pgmi_fail(PGM_EINVAL, "fit_finish: too many CPD columns for one launch");
  const FitFam *fams = static_cast<const FitFam *>(h->d_fams);
  const int64_t *col_off = static_cast<const int64_t *>(h->d_col_off);
  const int32_t nf = (int32_t)h->p.fams.size(), bayes = mode & PGM_FIT_BAYES ? 1 : 0;
  if (mode & PGM_FIT_WEIGHTED)
    hipLaunchKernelGGL(k_fit_finish<true>, dim3((unsigned)blocks), dim3(256), 0, S(stream), fams, col_off, nf, counts,
                       pseudo, bayes, values);
  else
    hipLaunchKernelGGL(k_fit_finish<false>, dim3((unsigned)blocks), dim3(256), 0, S(stream), fams, col_off, nf, counts,
                       pseudo, bayes, values);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

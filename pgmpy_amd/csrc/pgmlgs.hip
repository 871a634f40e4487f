// pgmlgs.hip — Gaussian structure learning on the moment matrix pgm_lg_gram leaves on the device
// (include/pgmhip.h "Gaussian structure learning"): thousands of small independent fp64 factorisations per
// launch.  A job is a conditioning set K and 1 .. 3 targets T, all indices into the (d + 1) x (d + 1) matrix;
// its result is a function of the Schur complement T|K.  Two kernels, chosen by a job's own |K|:
//   k_lgs_lane<K, T>  one job per lane, |K| <= PGM_LGS_LANE_MAX: the packed lower triangle of the (K + T)^2
//                     block lives in registers (every index is a compile-time constant);
//   k_lgs_wave        one wave per job, any |K| <= PGM_LGS_MAX_COND: the lower triangle in LDS, one lane per row.
// Both run the same steps in an order fixed by the job's own columns, with plain stores and no atomics, so a
// job's outputs carry the same bits whatever else is in the batch.  The host side is pgmlgs_plan.cpp.
#include "pgm_hip_common.h"
#include "pgm_ibeta.h"
#include "pgm_lgs.h"

struct LgsArgs {
  const int32_t *job_off, *job_cols, *order;
  const double *G, *shift;
  int32_t d, mode;  // mode: PGM_LGS_LL / BIC / AIC of a score launch (one target), unused by pcorr
  double *out0, *out1;
  int32_t *rank;
};

// ---------------------------------------------------------------------------- what both paths share
// Entry (u, v) of the moment matrix of a job: the shifted G as it stands, or with cu / cv the shifts (0 for the
// ones column) the raw moments M_uv = G_uv + c_u G_v1 + c_v G_u1 + n c_u c_v.  cu = cv = 0 adds exact zeros.
__device__ __forceinline__ double lgs_entry(double g, double cu, double cv, double gu1, double gv1, double n) {
  return ((g + cu * gv1) + cv * gu1) + (n * cu) * cv;
}

// coef and p-value from the Schur complement of (X, Y[, ones]) and the centred variances sxx, syy of the two
// targets before conditioning.  NaN: a non-finite entry, n <= 2, or a target without residual variance: one
// that is constant to rounding (sd below 64 u |shift|) or whose own pivot would be dropped (residual at or below
// RCOND of its variance).
template <int T>
__device__ __forceinline__ void lgs_pcorr_finish(double rxx, double ryx, double ryy, double r1x, double r1y, double n, double sxx,
                                                 double syy, double cx, double cy, bool bad, double *coef, double *pvalue) {
  double cxx = rxx, cyx = ryx, cyy = ryy;
  if (T == 3) {
    cxx = rxx - r1x * r1x / n;
    cyx = ryx - r1y * r1x / n;
    cyy = ryy - r1y * r1y / n;
  }
  const double tiny = 64.0 * 1.1102230246251565e-16;
  const bool live = !bad && n > 2.0 && sxx > n * (tiny * cx) * (tiny * cx) && syy > n * (tiny * cy) * (tiny * cy) &&
                    cxx > kLgsRcond * sxx && cyy > kLgsRcond * syy;
  double r = cyx / (sqrt(cxx) * sqrt(cyy));
  r = fmin(1.0, fmax(-1.0, r));
  *coef = live ? r : NAN;
  *pvalue = live ? pgm_pearson_p(r, n) : NAN;
}

// statsmodels' concentrated Gaussian log-likelihood and its penalties; rss <= 0: +inf as the closed form gives
__device__ __forceinline__ double lgs_score_finish(double rss, double n, int32_t df, int32_t mode, bool bad) {
  if (bad || !(n > 0.0)) return NAN;
  if (!(rss > 0.0)) return INFINITY;
  const double llf = -0.5 * n * (log(6.283185307179586477 * rss / n) + 1.0);
  if (mode == PGM_LGS_BIC) return llf - 0.5 * (double)(df + 2) * log(n);
  if (mode == PGM_LGS_AIC) return llf - (double)(df + 2);
  return llf;
}

// ---------------------------------------------------------------------------- the lane path
template <int K, int T>
__global__ __launch_bounds__(kLgsBlock) void k_lgs_lane(const LgsArgs a, int32_t first, int32_t count) {
  constexpr int M = K + T;
  const int32_t i0 = (int32_t)(blockIdx.x * kLgsBlock + threadIdx.x);
  if (i0 >= count) return;
  const int32_t job = a.order[first + i0];
  const int32_t *cols = a.job_cols + a.job_off[job];
  const int32_t d = a.d, d1 = d + 1;
  const double n = a.G[(int64_t)d * d1 + d];
  int32_t col[M];
  double c[M], g1[M];
  bool has_ones = false;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    col[i] = cols[i];
    if (i < K) has_ones |= col[i] == d;
  }
  const bool raw = K > 0 && !has_ones;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    c[i] = raw && col[i] != d ? a.shift[col[i]] : 0.0;
    g1[i] = a.G[(int64_t)col[i] * d1 + d];
  }
  double A[M * (M + 1) / 2];
  bool bad = false;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const double g = a.G[(int64_t)col[i] * d1 + col[j]];
      bad |= !isfinite(g);
      A[i * (i + 1) / 2 + j] = lgs_entry(g, c[i], c[j], g1[i], g1[j], n);
    }
  // the targets' centred variances before conditioning (pcorr)
  double s0 = 0.0, s1 = 0.0, c0 = 0.0, c1 = 0.0;
  if constexpr (T >= 2) {
    const double gx = a.G[(int64_t)col[K] * d1 + col[K]], gy = a.G[(int64_t)col[K + 1] * d1 + col[K + 1]];
    s0 = gx - g1[K] * g1[K] / n;
    s1 = gy - g1[K + 1] * g1[K + 1] / n;
    c0 = col[K] != d ? a.shift[col[K]] : 0.0;
    c1 = col[K + 1] != d ? a.shift[col[K + 1]] : 0.0;
  }
  // K to unit diagonal; a column with no positive diagonal is dropped here
  double s[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const double dg = A[i * (i + 1) / 2 + i];
    s[i] = i < K ? (dg > 0.0 ? 1.0 / sqrt(dg) : 0.0) : 1.0;
  }
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] *= s[i] * s[j];
  // Cholesky without pivoting in its outer-product form; a pivot at or below RCOND drops its column
  int32_t rank = 0, df = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double p = A[j * (j + 1) / 2 + j];
    const bool keep = p > kLgsRcond;
    const double inv = keep ? 1.0 / p : 0.0;
    rank += keep ? 1 : 0;
    df += keep && col[j] != d ? 1 : 0;
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      const double l = A[i * (i + 1) / 2 + j] * inv;
#pragma unroll
      for (int b = j + 1; b <= i; ++b) A[i * (i + 1) / 2 + b] -= l * A[b * (b + 1) / 2 + j];
    }
  }
#define LGS_R(i, j) A[(K + (i)) * (K + (i) + 1) / 2 + K + (j)]
  if constexpr (T == 1) {
    const double rss = LGS_R(0, 0);
    a.out0[job] = lgs_score_finish(rss, n, df, a.mode, bad);
    a.out1[job] = bad ? NAN : rss;
  } else {
    double coef, pv;
    lgs_pcorr_finish<T>(LGS_R(0, 0), LGS_R(1, 0), LGS_R(1, 1), T == 3 ? LGS_R(T - 1, 0) : 0.0, T == 3 ? LGS_R(T - 1, 1) : 0.0, n,
                        s0, s1, c0, c1, bad, &coef, &pv);
    a.out0[job] = coef;
    a.out1[job] = pv;
  }
#undef LGS_R
  a.rank[job] = rank;
}

// ---------------------------------------------------------------------------- the wave path
// LDS (doubles): A[m][ldm] lower triangle, ldm = m | 1 (an odd row length keeps the row-per-lane accesses of a
// column on distinct banks), then c[m], g1[m], s[m].  At |K| = 64 with three targets: 67 * 67 + 201 doubles =
// 37,520 bytes, four workgroups per CU.
__global__ __launch_bounds__(kLgsBlock) void k_lgs_wave(const LgsArgs a, int32_t first, int32_t k, int32_t t) {
  extern __shared__ double lds[];
  const int32_t m = k + t, ldm = m | 1, lane = (int32_t)threadIdx.x;
  double *A = lds, *c = lds + (size_t)m * ldm, *g1 = c + m, *s = g1 + m;
  const int32_t job = a.order[first + (int32_t)blockIdx.x];
  const int32_t *cols = a.job_cols + a.job_off[job];
  const int32_t d = a.d, d1 = d + 1;
  const double n = a.G[(int64_t)d * d1 + d];
  bool mine = false;
  for (int32_t i = lane; i < k; i += kLgsBlock) mine |= cols[i] == d;
  const bool raw = k > 0 && !__any(mine);
  for (int32_t i = lane; i < m; i += kLgsBlock) {
    const int32_t ci = cols[i];
    c[i] = raw && ci != d ? a.shift[ci] : 0.0;
    g1[i] = a.G[(int64_t)ci * d1 + d];
  }
  __syncthreads();
  bool bad = false;
  for (int32_t i = lane; i < m; i += kLgsBlock) {
    const int32_t ci = cols[i];
    const double cu = c[i], gu1 = g1[i];
    double dg = 0.0;
    for (int32_t j = 0; j <= i; ++j) {
      const double g = a.G[(int64_t)ci * d1 + cols[j]];
      bad |= !isfinite(g);
      dg = lgs_entry(g, cu, c[j], gu1, g1[j], n);
      A[(size_t)i * ldm + j] = dg;
    }
    s[i] = i < k ? (dg > 0.0 ? 1.0 / sqrt(dg) : 0.0) : 1.0;
  }
  bad = __any(bad);
  __syncthreads();
  for (int32_t i = lane; i < m; i += kLgsBlock) {
    const double si = s[i];
    for (int32_t j = 0; j <= i; ++j) A[(size_t)i * ldm + j] *= si * s[j];
  }
  __syncthreads();
  int32_t rank = 0, df = 0;
  for (int32_t j = 0; j < k; ++j) {
    const double p = A[(size_t)j * ldm + j];  // the same word for every lane: the branch is uniform
    if (p > kLgsRcond) {
      const double inv = 1.0 / p;
      rank += 1;
      df += cols[j] != d ? 1 : 0;
      for (int32_t i = j + 1 + lane; i < m; i += kLgsBlock) {
        const double l = A[(size_t)i * ldm + j] * inv;
        for (int32_t b = j + 1; b <= i; ++b) A[(size_t)i * ldm + b] -= l * A[(size_t)b * ldm + j];
      }
    }
    __syncthreads();
  }
  if (lane != 0) return;
#define LGS_R(i, j) A[(size_t)(k + (i)) * ldm + k + (j)]
  if (t == 1) {
    const double rss = LGS_R(0, 0);
    a.out0[job] = lgs_score_finish(rss, n, df, a.mode, bad);
    a.out1[job] = bad ? NAN : rss;
  } else {
    const int32_t cx = cols[k], cy = cols[k + 1];
    const double gx = a.G[(int64_t)cx * d1 + cx], gy = a.G[(int64_t)cy * d1 + cy];
    const double s0 = gx - g1[k] * g1[k] / n, s1 = gy - g1[k + 1] * g1[k + 1] / n;
    const double c0 = cx != d ? a.shift[cx] : 0.0, c1 = cy != d ? a.shift[cy] : 0.0;
    double coef, pv;
    if (t == 3)
      lgs_pcorr_finish<3>(LGS_R(0, 0), LGS_R(1, 0), LGS_R(1, 1), LGS_R(2, 0), LGS_R(2, 1), n, s0, s1, c0, c1, bad, &coef, &pv);
    else
      lgs_pcorr_finish<2>(LGS_R(0, 0), LGS_R(1, 0), LGS_R(1, 1), 0.0, 0.0, n, s0, s1, c0, c1, bad, &coef, &pv);
    a.out0[job] = coef;
    a.out1[job] = pv;
  }
#undef LGS_R
  a.rank[job] = rank;
}

// ---------------------------------------------------------------------------- launches
typedef void (*LgsLaneKernel)(const LgsArgs, int32_t, int32_t);

template <int K>
static LgsLaneKernel lgs_lane_kernel_t(int32_t t) {
  return t == 1 ? k_lgs_lane<K, 1> : t == 2 ? k_lgs_lane<K, 2> : k_lgs_lane<K, 3>;
}

static LgsLaneKernel lgs_lane_kernel(int32_t k, int32_t t) {
  static_assert(kLgsLaneMax == 7, "one case per lane-path size");
  switch (k) {
    case 0: return lgs_lane_kernel_t<0>(t);
    case 1: return lgs_lane_kernel_t<1>(t);
    case 2: return lgs_lane_kernel_t<2>(t);
    case 3: return lgs_lane_kernel_t<3>(t);
    case 4: return lgs_lane_kernel_t<4>(t);
    case 5: return lgs_lane_kernel_t<5>(t);
    case 6: return lgs_lane_kernel_t<6>(t);
    default: return lgs_lane_kernel_t<7>(t);
  }
}

static int lgs_launch(LgsHandle *h, LgsArgs a, void *stream) {
  using pgmdev::upload;
  const LgsPlan &p = h->p;
  const pgmdev::Slot base[] = {upload(h->d_job_off, p.job_off), upload(h->d_job_cols, p.job_cols), upload(h->d_order, p.order)};
  const int up = h->dev.use(kHipDevOps, base);
  if (up != PGM_OK) return up;
  a.job_off = h->d_job_off;
  a.job_cols = h->d_job_cols;
  a.order = h->d_order;
  for (const LgsBucket &b : p.buckets) {
    if (b.k <= kLgsLaneMax) {
      hipLaunchKernelGGL(lgs_lane_kernel(b.k, b.t), dim3((unsigned)((b.count + kLgsBlock - 1) / kLgsBlock)), dim3(kLgsBlock), 0,
                         S(stream), a, b.first, b.count);
    } else {
      hipLaunchKernelGGL(k_lgs_wave, dim3((unsigned)b.count), dim3(kLgsBlock), 8 * lgs_wave_lds_doubles(b.k, b.t), S(stream), a,
                         b.first, b.k, b.t);
    }
    HIP_TRY(hipGetLastError());
  }
  return PGM_OK;
}

extern "C" {

int pgm_lgs_jobs_destroy(void *handle) { return pgm_plan_destroy<LgsHandle>(handle); }

int pgm_lgs_pcorr(void *handle, const double *G, const double *shift, int32_t d, int32_t intercept, double *coef, double *pvalue,
                  int32_t *rank, void *stream) {
  LgsHandle *h = static_cast<LgsHandle *>(handle);
  bool launch = false;
  const int st = lgs_pcorr_check(h, G, shift, d, intercept, coef, pvalue, rank, &launch);
  if (st != PGM_OK || !launch) return st;
  LgsArgs a = {};
  a.G = G, a.shift = shift, a.d = d, a.mode = 0, a.out0 = coef, a.out1 = pvalue, a.rank = rank;
  return lgs_launch(h, a, stream);
}

int pgm_lgs_score(void *handle, const double *G, const double *shift, int32_t d, int32_t kind, double *score, double *rss,
                  int32_t *rank, void *stream) {
  LgsHandle *h = static_cast<LgsHandle *>(handle);
  bool launch = false;
  const int st = lgs_score_check(h, G, shift, d, kind, score, rss, rank, &launch);
  if (st != PGM_OK || !launch) return st;
  LgsArgs a = {};
  a.G = G, a.shift = shift, a.d = d, a.mode = kind, a.out0 = score, a.out1 = rss, a.rank = rank;
  return lgs_launch(h, a, stream);
}
}

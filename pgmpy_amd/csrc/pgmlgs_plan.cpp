// pgmlgs_plan.cpp — the host side of the Gaussian structure learning calls (include/pgmhip.h "Gaussian
// structure learning"): validation of a job batch, its buckets by (|K|, targets), and the argument checks
// of pgm_lgs_pcorr / pgm_lgs_score.  No HIP call and no HIP include: ctypes drives all of it without a
// device.  The kernels and launches are pgmlgs.hip.
#include <algorithm>
#include <new>

#include "pgm_ibeta.h"
#include "pgm_lgs.h"

int lgs_plan_build(const int32_t *job_off, const int32_t *job_cols, const int32_t *n_targets, int32_t n_jobs, int32_t d,
                   LgsPlan &out) {
  if (n_jobs < 0) return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: %d jobs", n_jobs);
  if (d < 0 || d == INT32_MAX) return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: d %d", d);
  if (!job_off) return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: null job_off");
  if (n_jobs > 0 && (!job_cols || !n_targets)) return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: null job_cols / n_targets");
  if (job_off[0] != 0) return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: job_off[0] is %d", job_off[0]);
  LgsPlan p;
  p.n_jobs = n_jobs;
  p.d = d;
  p.has_ones.assign((size_t)n_jobs, 0);
  p.last_is_ones.assign((size_t)n_jobs, 0);
  std::vector<int32_t> key((size_t)n_jobs);  // k * 4 + t
  std::vector<int32_t> sorted;
  for (int32_t j = 0; j < n_jobs; ++j) {
    const int32_t t = n_targets[j];
    const int64_t len = (int64_t)job_off[j + 1] - job_off[j];
    if (t < 1 || t > kLgsMaxTargets)
      return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: job %d has %d targets (1 .. %d)", j, t, kLgsMaxTargets);
    if (len < t) return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: job %d has %lld columns for %d targets", j, (long long)len, t);
    const int64_t k = len - t;
    if (k > kLgsMaxCond)
      return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: job %d has %lld conditioning columns (at most %d)", j, (long long)k,
                        kLgsMaxCond);
    const int32_t *c = job_cols + job_off[j];
    for (int64_t i = 0; i < len; ++i)
      if (c[i] < 0 || c[i] > d)
        return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: job %d names column %d (0 .. %d)", j, c[i], d);
    // a column twice in K is an exactly collinear pair nobody asked for; a target in K has residual 0
    sorted.assign(c, c + len);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t i = 1; i < len; ++i)
      if (sorted[(size_t)i] == sorted[(size_t)i - 1]) {
        const bool in_k = std::find(c, c + k, sorted[(size_t)i]) != c + k;
        const bool in_t = std::find(c + k, c + len, sorted[(size_t)i]) != c + len;
        return pgmi_failf(PGM_EINVAL, in_k && in_t ? "lgs_jobs_create: job %d: target column %d is also a conditioning column"
                                                    : "lgs_jobs_create: job %d lists column %d twice",
                          j, sorted[(size_t)i]);
      }
    p.has_ones[(size_t)j] = std::find(c, c + k, d) != c + k ? 1 : 0;
    p.last_is_ones[(size_t)j] = c[len - 1] == d ? 1 : 0;
    p.max_cond = std::max(p.max_cond, (int32_t)k);
    key[(size_t)j] = (int32_t)k * 4 + t;
    (k <= kLgsLaneMax ? p.n_lane_jobs : p.n_wave_jobs) += 1;
  }
  p.job_off.assign(job_off, job_off + n_jobs + 1);
  p.job_cols.assign(job_cols, job_cols + (n_jobs ? job_off[n_jobs] : 0));
  // the buckets: ascending (k, t), the jobs of one in their own order
  p.order.resize((size_t)n_jobs);
  for (int32_t j = 0; j < n_jobs; ++j) p.order[(size_t)j] = j;
  std::stable_sort(p.order.begin(), p.order.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
  for (int32_t i = 0; i < n_jobs; ++i) {
    const int32_t kt = key[(size_t)p.order[(size_t)i]];
    if (p.buckets.empty() || p.buckets.back().k * 4 + p.buckets.back().t != kt) p.buckets.push_back(LgsBucket{kt / 4, kt % 4, i, 0});
    p.buckets.back().count += 1;
  }
  out = std::move(p);
  return PGM_OK;
}

static int lgs_common_check(const char *what, const LgsHandle *h, const double *G, const double *shift, int32_t d,
                            const void *o0, const void *o1, const void *o2, bool *launch) {
  *launch = false;
  if (!h) return pgmi_failf(PGM_EINVAL, "%s: null handle", what);
  if (d != h->p.d) return pgmi_failf(PGM_EINVAL, "%s: d %d, the handle was made for d %d", what, d, h->p.d);
  if (h->p.n_jobs == 0) return PGM_OK;
  if (!G || !shift) return pgmi_failf(PGM_EINVAL, "%s: null G / shift", what);
  if (!o0 || !o1 || !o2) return pgmi_failf(PGM_EINVAL, "%s: null output", what);
  *launch = true;
  return PGM_OK;
}

int lgs_pcorr_check(const LgsHandle *h, const double *G, const double *shift, int32_t d, int32_t intercept, const double *coef,
                    const double *pvalue, const int32_t *rank, bool *launch) {
  const int st = lgs_common_check("lgs_pcorr", h, G, shift, d, coef, pvalue, rank, launch);
  if (st != PGM_OK) return st;
  if (intercept != 0 && intercept != 1) return pgmi_failf(PGM_EINVAL, "lgs_pcorr: intercept %d", intercept);
  const LgsPlan &p = h->p;
  for (const LgsBucket &b : p.buckets)
    if (b.t != (intercept ? 2 : 3))
      return pgmi_failf(PGM_EINVAL, "lgs_pcorr: job %d has %d targets, intercept %d needs %d", p.order[(size_t)b.first], b.t,
                        intercept, intercept ? 2 : 3);
  // K and the targets are disjoint, so a job whose last target is the ones column has none in K
  for (int32_t j = 0; j < p.n_jobs; ++j) {
    const bool ones_k = p.has_ones[(size_t)j] != 0, ones_t = p.last_is_ones[(size_t)j] != 0;
    if (!(intercept ? ones_k : ones_t))
      return pgmi_failf(PGM_EINVAL,
                        intercept ? "lgs_pcorr: job %d: with an intercept a job is K (the ones column in it) and the targets X, Y"
                                  : "lgs_pcorr: job %d: without an intercept a job is K and the targets X, Y, ones column",
                        j);
  }
  return PGM_OK;
}

int lgs_score_check(const LgsHandle *h, const double *G, const double *shift, int32_t d, int32_t kind, const double *score,
                    const double *rss, const int32_t *rank, bool *launch) {
  const int st = lgs_common_check("lgs_score", h, G, shift, d, score, rss, rank, launch);
  if (st != PGM_OK) return st;
  if (kind != PGM_LGS_LL && kind != PGM_LGS_BIC && kind != PGM_LGS_AIC) return pgmi_failf(PGM_EINVAL, "lgs_score: kind %d", kind);
  const LgsPlan &p = h->p;
  for (const LgsBucket &b : p.buckets)
    if (b.t != 1) return pgmi_failf(PGM_EINVAL, "lgs_score: job %d has %d targets, a family has one", p.order[(size_t)b.first], b.t);
  for (int32_t j = 0; j < p.n_jobs; ++j)
    if (!p.has_ones[(size_t)j]) return pgmi_failf(PGM_EINVAL, "lgs_score: job %d: K must hold the ones column %d (the intercept)", j, d);
  return PGM_OK;
}

extern "C" {

int pgm_lgs_jobs_create(const int32_t *job_off, const int32_t *job_cols, const int32_t *n_targets, int32_t n_jobs, int32_t d,
                        void **handle) {
  if (!handle) return pgmi_failf(PGM_EINVAL, "lgs_jobs_create: null handle");
  *handle = nullptr;
  LgsHandle *h = new (std::nothrow) LgsHandle();
  if (!h) return pgmi_failf(PGM_ENOMEM, "lgs_jobs_create: out of memory");
  const int st = lgs_plan_build(job_off, job_cols, n_targets, n_jobs, d, h->p);
  if (st != PGM_OK) {
    delete h;
    return st;
  }
  *handle = h;
  return PGM_OK;
}

int pgm_lgs_jobs_info(void *handle, pgm_lgs_info_t *info, int32_t *buckets, int32_t *order) {
  const LgsHandle *h = static_cast<const LgsHandle *>(handle);
  if (!h) return pgmi_failf(PGM_EINVAL, "lgs_jobs_info: null handle");
  const LgsPlan &p = h->p;
  if (info) {
    info->n_jobs = p.n_jobs;
    info->d = p.d;
    info->n_buckets = (int32_t)p.buckets.size();
    info->max_cond = p.max_cond;
    info->n_lane_jobs = p.n_lane_jobs;
    info->n_wave_jobs = p.n_wave_jobs;
    info->wave_lds_bytes = p.n_wave_jobs ? (int64_t)(8 * lgs_wave_lds_doubles(p.max_cond, p.buckets.back().t)) : 0;
  }
  if (buckets)
    for (size_t b = 0; b < p.buckets.size(); ++b) {
      buckets[4 * b] = p.buckets[b].k;
      buckets[4 * b + 1] = p.buckets[b].t;
      buckets[4 * b + 2] = p.buckets[b].first;
      buckets[4 * b + 3] = p.buckets[b].count;
    }
  if (order) std::copy(p.order.begin(), p.order.end(), order);
  return PGM_OK;
}

int pgm_lgs_ibeta_half(double a, double y, double *out) {
  if (!out) return pgmi_failf(PGM_EINVAL, "lgs_ibeta_half: null out");
  *out = pgm_ibeta_half(a, y);
  return PGM_OK;
}
}

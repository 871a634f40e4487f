// pgmfit.hip — parameter learning on the device (gfx950): the family-count kernel and the CPD finishing
// kernel behind DiscreteBayesianNetwork.fit / fit_update, and their C-ABI (pgm_fit_plan_destroy,
// pgm_fit_count, pgm_fit_finish), the E-step kernel of ExpectationMaximization (pgm_fit_estep), and the
// structure-score kernels behind estimators/StructureScore.py and
// HillClimbSearch (pgm_fit_score).  Replaces the reference's per-node pandas groupby
// (estimators/base.py:67-176) and the per-CPD normalisation (MLE.py:183-212, BayesianEstimator.py:252-264).
// The host side (validation, table layout, family groups, argument checks) is pgmfit_plan.cpp.
#include <type_traits>

#include "pgm_fit.h"
#include "pgm_hip_common.h"
#include "pgm_igamc.h"

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
// V4 = true (codes, ld and row0 all multiples of 4: codes_vec4): a lane takes 4 consecutive rows and
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
          if (c >= (uint32_t)F.card[v]) {  // missing, or not a state: the later columns are still checked
            bad |= c != PGM_EV_MISSING;
            skip = true;
            continue;
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

// ---------------------------------------------------------------------------- the E-step
// Expected family counts of a network with latent variables (pgm_fit_estep; the reference's
// _compute_weights + weighted state_counts, EM.py:130-180).  The geometry is k_fit_count<true>'s: workgroup
// b takes row chunk b / n_groups for family group b % n_groups, privatises the group's run of bins in LDS
// as fp64 and adds the non-zero bins to global memory; a global group adds straight into its table.
// A work-item takes one row at a time.  It first walks every family of the plan: the observed part of the
// family's index (code x stride over the observed variables) decides whether the row is counted at all (a
// missing or bad code in any family drops the row from every table), and for a family with a latent it
// goes to the LDS scratch [family][work-item] (consecutive lanes, consecutive banks).  Pass 1 adds
// Z = sum_l p_l over the latent configurations, p_l the product over ALL latent families of the plan of
// max(value, floor), the values gathered from global memory (the tables are small: L1 / L2).  Pass 2
// recomputes p_l and adds p_l / Z to the latent families of the workgroup's own group only; a latent-free
// family of the group gets 1.0 (its factor is the same for every l and cancels; sum_l w_l = 1).  The
// latent digits of l, the latent strides (EmSpec, in the kernarg segment) and the family descriptors are
// workgroup-uniform: scalar work.  Nothing of size [L, rows] leaves the CU.  The workgroups of group 0
// write loglik.
// LDS: the 32 KiB fp64 tile + 1 KiB of scratch per latent family (fit_estep_lds).  A plan with up to 8
// latent families takes at most 40 KiB: 4 workgroups (16 waves) share a CU's 160 KiB; at the cap of 32
// families it is 64 KiB: 2 workgroups, 8 waves per CU.
__device__ inline bool em_observed_index(const FitFam &F, const EmSpec &s, const uint8_t *__restrict__ codes,
                                         int64_t ld, int64_t row, int32_t &idx, bool &bad) {
  bool ok = true;
  idx = 0;
  for (int32_t v = 0; v < F.n_vars; ++v) {
    const int32_t col = F.col[v];
    bool latent = false;
    for (int32_t j = 0; j < s.n_latent; ++j) latent |= s.col[j] == col;
    if (latent) continue;  // virtual: codes is never read for it
    const uint32_t c = codes[(int64_t)col * ld + row];
    if (c >= (uint32_t)F.card[v]) {  // missing, or not a state
      bad |= c != PGM_EV_MISSING;
      ok = false;
    } else {
      idx += (int32_t)c * F.stride[v];
    }
  }
  return ok;
}

// the part of family s.fam[k]'s index that latent configuration d adds
__device__ inline int32_t em_latent_index(const EmSpec &s, int32_t k, const int32_t (&d)[PGM_EM_MAX_LATENT]) {
  int32_t e = 0;
#pragma unroll
  for (int j = 0; j < PGM_EM_MAX_LATENT; ++j) e += d[j] * s.stride[k][j];  // stride 0 past n_latent
  return e;
}

// the next configuration: the last latent fastest
__device__ inline void em_next(const EmSpec &s, int32_t (&d)[PGM_EM_MAX_LATENT]) {
  bool carry = true;
#pragma unroll
  for (int j = PGM_EM_MAX_LATENT - 1; j >= 0; --j)
    if (carry && j < s.n_latent) {
      if (++d[j] == s.card[j]) d[j] = 0;
      else carry = false;
    }
}

__device__ inline double em_floor(double v) { return PGM_EM_FLOOR > v ? PGM_EM_FLOOR : v; }  // Python's max(v, 1e-10)

__global__ __launch_bounds__(kFitBlock) void k_fit_estep(const FitFam *__restrict__ fams,
                                                         const FitGroup *__restrict__ groups, uint32_t n_groups,
                                                         const EmSpec s, const double *__restrict__ values,
                                                         const uint8_t *__restrict__ codes, int64_t ld, int64_t row0,
                                                         int64_t n_rows, double *__restrict__ tables,
                                                         double *__restrict__ loglik, int32_t *__restrict__ err) {
  extern __shared__ unsigned char fit_lds[];
  double *lds = reinterpret_cast<double *>(fit_lds);
  int32_t *scratch = reinterpret_cast<int32_t *>(fit_lds + kFitTileBins * sizeof(double));
  const uint32_t tid = threadIdx.x;
  const uint32_t gi = blockIdx.x % n_groups;
  const FitGroup g = groups[gi];
  const int64_t r_begin = (int64_t)(blockIdx.x / n_groups) * kFitRowsPerBlock;
  const int64_t r_end = r_begin + kFitRowsPerBlock < n_rows ? r_begin + kFitRowsPerBlock : n_rows;
  double *out = tables + g.off;
  if (!g.global) {
    for (int32_t i = (int32_t)tid; i < g.bins; i += kFitBlock) lds[i] = 0.0;
    __syncthreads();
  }
  // the latent families of this group: s.fam[kb .. ke)
  int32_t kb = 0;
  while (kb < s.n_lat_fam && s.fam[kb] < g.fam_begin) ++kb;
  int32_t ke = kb;
  while (ke < s.n_lat_fam && s.fam[ke] < g.fam_end) ++ke;
  const bool want_ll = loglik && gi == 0;
  // p_l of the row whose observed indices are in the scratch
  auto weight = [&](const int32_t (&d)[PGM_EM_MAX_LATENT]) {
    double p = 1.0;
    for (int32_t k = 0; k < s.n_lat_fam; ++k) {
      const int32_t e = scratch[k * kFitBlock + (int32_t)tid] + em_latent_index(s, k, d);
      p *= em_floor(values[fams[s.fam[k]].off + e]);
    }
    return p;
  };
  bool bad = false;
  for (int64_t r = r_begin + tid; r < r_end; r += kFitBlock) {
    const int64_t row = row0 + r;
    bool ok = true;
    for (int32_t f = 0, k = 0; f < s.n_fam; ++f) {
      int32_t idx;
      ok &= em_observed_index(fams[f], s, codes, ld, row, idx, bad);
      if (k < s.n_lat_fam && s.fam[k] == f) scratch[k++ * kFitBlock + (int32_t)tid] = idx;
    }
    if (!ok) {  // not counted in any table
      if (want_ll) loglik[row] = 0.0;
      continue;
    }
    double Z = 0.0;
    {
      int32_t d[PGM_EM_MAX_LATENT] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int32_t l = 0; l < s.n_configs; ++l, em_next(s, d)) Z += weight(d);
    }
    if (kb < ke) {
      int32_t d[PGM_EM_MAX_LATENT] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int32_t l = 0; l < s.n_configs; ++l, em_next(s, d)) {
        const double w = weight(d) / Z;
        for (int32_t k = kb; k < ke; ++k) {
          const int32_t e = scratch[k * kFitBlock + (int32_t)tid] + em_latent_index(s, k, d);
          if (g.global) atomicAdd(&out[e], w);
          else atomicAdd(&lds[(int32_t)(fams[s.fam[k]].off - g.off) + e], w);
        }
      }
    }
    double ll = want_ll ? log(Z) : 0.0;
    for (int32_t f = 0, k = 0; f < s.n_fam; ++f) {
      if (k < s.n_lat_fam && s.fam[k] == f) {
        ++k;
        continue;
      }
      const bool mine = f >= g.fam_begin && f < g.fam_end;
      if (!mine && !want_ll) continue;
      const FitFam &F = fams[f];
      int32_t idx;
      bool unused = false;
      (void)em_observed_index(F, s, codes, ld, row, idx, unused);  // every code is a state: checked above
      if (mine) {
        if (g.global) atomicAdd(&out[idx], 1.0);
        else atomicAdd(&lds[(int32_t)(F.off - g.off) + idx], 1.0);
      }
      if (want_ll) ll += log(em_floor(values[F.off + idx]));
    }
    if (want_ll) loglik[row] = ll;
  }
  if (bad) atomicOr(err, 1);
  if (!g.global) {
    __syncthreads();
    for (int32_t i = (int32_t)tid; i < g.bins; i += kFitBlock) {
      const double v = lds[i];
      if (v != 0.0) atomicAdd(&out[i], v);
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

// ---------------------------------------------------------------------------- structure scores
// The data-dependent sum of a structure score (StructureScore.py:346-380, 462-494, 654-685, 706-728) for
// every family, from the int64 count tables.  Workgroup b takes one chunk of kScoreChunk columns of one
// family (bisection over chunk_off: workgroup-uniform); a work-item takes one column.  For a fixed state
// consecutive work-items read consecutive int64 of the [r, q] table.  A work-item adds its column's
// terms in state order, the workgroup adds its work-items' sums in a fixed tree (work-items past the
// family's last column add +0.0), and writes one partial per chunk: the order of every addition depends
// only on the family's own shape.  fp64 throughout, no floating-point atomics.
template <bool LL>
__global__ __launch_bounds__(kScoreChunk) void k_fit_score(const FitFam *__restrict__ fams,
                                                           const int64_t *__restrict__ chunk_off, int32_t n_fam,
                                                           const int64_t *__restrict__ counts,
                                                           const double *__restrict__ alpha,
                                                           const double *__restrict__ beta, int32_t skip_empty,
                                                           double *__restrict__ part, int64_t *__restrict__ part_obs) {
  __shared__ double s_sum[kScoreChunk];
  __shared__ int32_t s_obs[kScoreChunk];
  const int64_t b = blockIdx.x;
  int32_t lo = 0, hi = n_fam;  // chunk_off[lo] <= b < chunk_off[hi]; empty ranges do not occur (q >= 1)
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= b) lo = mid;
    else hi = mid;
  }
  const FitFam &F = fams[lo];
  const int32_t card = F.card[0];
  const int64_t ncol = F.size / card;
  const int64_t col = (b - chunk_off[lo]) * kScoreChunk + threadIdx.x;
  double sum = 0.0;
  int32_t obs = 0;
  if (col < ncol) {
    const int64_t *cnt = counts + F.off + col;
    int64_t nj = 0;
    for (int32_t s = 0; s < card; ++s) nj += cnt[s * ncol];
    obs = nj > 0;
    if (LL) {
      if (nj > 0) {
        const double lnj = log((double)nj);
        for (int32_t s = 0; s < card; ++s) {
          const int64_t n = cnt[s * ncol];
          if (n > 0) sum += (double)n * (log((double)n) - lnj);
        }
      }
    } else if (nj > 0 || !skip_empty) {
      const double be = beta[lo];
      for (int32_t s = 0; s < card; ++s) sum += lgamma((double)cnt[s * ncol] + be);
      sum -= lgamma((double)nj + alpha[lo]);
    }
  }
  s_sum[threadIdx.x] = sum;
  s_obs[threadIdx.x] = obs;
  __syncthreads();
  for (int32_t w = kScoreChunk / 2; w > 0; w >>= 1) {
    if ((int32_t)threadIdx.x < w) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
      s_obs[threadIdx.x] += s_obs[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[b] = s_sum[0];
    part_obs[b] = s_obs[0];
  }
}

// One workgroup per family adds the family's chunk partials: work-item t takes partials t, t + 64, ... in
// index order, then the same fixed tree.
__global__ __launch_bounds__(kScoreSumBlock) void k_fit_score_sum(const int64_t *__restrict__ chunk_off,
                                                                  const double *__restrict__ part,
                                                                  const int64_t *__restrict__ part_obs,
                                                                  double *__restrict__ scores,
                                                                  int64_t *__restrict__ n_observed) {
  __shared__ double s_sum[kScoreSumBlock];
  __shared__ int64_t s_obs[kScoreSumBlock];
  const int64_t begin = chunk_off[blockIdx.x], end = chunk_off[blockIdx.x + 1];
  double sum = 0.0;
  int64_t obs = 0;
  for (int64_t i = begin + threadIdx.x; i < end; i += kScoreSumBlock) {
    sum += part[i];
    obs += part_obs[i];
  }
  s_sum[threadIdx.x] = sum;
  s_obs[threadIdx.x] = obs;
  __syncthreads();
  for (int32_t w = kScoreSumBlock / 2; w > 0; w >>= 1) {
    if ((int32_t)threadIdx.x < w) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
      s_obs[threadIdx.x] += s_obs[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    scores[blockIdx.x] = s_sum[0];
    if (n_observed) n_observed[blockIdx.x] = s_obs[0];
  }
}

// One workgroup per family marks the states that hold a count in any column (consecutive work-items read
// consecutive bins) and counts the marks.  A cardinality is at most 255, so a state indexes s_seen.
__global__ __launch_bounds__(256) void k_fit_states_observed(const FitFam *__restrict__ fams,
                                                             const int64_t *__restrict__ counts,
                                                             int64_t *__restrict__ n_states) {
  __shared__ int32_t s_seen[256];
  const FitFam &F = fams[blockIdx.x];
  const int32_t card = F.card[0];
  const int64_t size = F.size, ncol = size / card;
  s_seen[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < size; i += 256)
    if (counts[F.off + i] > 0) atomicOr(&s_seen[i / ncol], 1);
  __syncthreads();
  for (int32_t w = 128; w > 0; w >>= 1) {
    if ((int32_t)threadIdx.x < w) s_seen[threadIdx.x] += s_seen[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_states[blockIdx.x] = s_seen[0];
}

// ---------------------------------------------------------------------------- CI tests
// The power-divergence test of X _|_ Y | Z per family (X, Y, Z...) from its int64 table [rx][ry][qz]
// (CITests.py:445-499 over scipy's chi2_contingency).  For a fixed cell consecutive strata are consecutive
// int64, so work-items that take consecutive strata read coalesced.  kind: 0 lambda = 1, 1 lambda = 0,
// 2 lambda = -1, 3 any other lambda; scale: the factor in front of the stratum's sum.
__device__ inline double ci_term(double o, double e, double lambda, int32_t kind) {
  if (kind == 0) {
    const double d = o - e;
    return d * d / e;
  }
  if (kind == 1) return o > 0.0 ? o * log(o / e) : 0.0;
  if (kind == 2) return e * log(e / o);  // o = 0: e * log(inf) = +inf, as scipy's xlogy
  return o * (pow(o / e, lambda) - 1.0);  // o = 0 and lambda < 0: 0 * inf = NaN, as scipy
}

// chi2_contingency's continuity correction: the observed cell moves towards e by min(0.5, |e - o|)
__device__ inline double ci_yates(double o, double e) {
  const double diff = e - o, mag = fmin(0.5, fabs(diff));
  return diff > 0.0 ? o + mag : (diff < 0.0 ? o - mag : o);
}

// One stratum of a small table (rx + ry <= kCiSmall) by one work-item.  cnt points at the stratum's
// [0][0] cell (cells are qz apart); m[k * kCiChunk], k < rx + ry, is the work-item's own column of the LDS
// marginals (consecutive work-items are 8 bytes apart: conflict-free).  Cells are added row-major.
__device__ inline void ci_stratum_small(const int64_t *__restrict__ cnt, int32_t rx, int32_t ry, int64_t qz,
                                        double lambda, int32_t kind, double scale, int32_t yates, int64_t *m,
                                        double &stat, int64_t &dof) {
  stat = 0.0, dof = 0;
  for (int32_t k = 0; k < rx + ry; ++k) m[k * kCiChunk] = 0;
  for (int32_t x = 0; x < rx; ++x)
    for (int32_t y = 0; y < ry; ++y) {
      const int64_t o = cnt[((int64_t)x * ry + y) * qz];
      m[x * kCiChunk] += o;
      m[(rx + y) * kCiChunk] += o;
    }
  int64_t n = 0;
  int32_t nr = 0, nc = 0;
  for (int32_t x = 0; x < rx; ++x) n += m[x * kCiChunk], nr += m[x * kCiChunk] > 0;
  for (int32_t y = 0; y < ry; ++y) nc += m[(rx + y) * kCiChunk] > 0;
  const int32_t d = (nr - 1) * (nc - 1);
  if (n == 0 || d <= 0) return;
  const bool adjust = yates && d == 1;
  double sum = 0.0;
  for (int32_t x = 0; x < rx; ++x) {
    const int64_t R = m[x * kCiChunk];
    if (R == 0) continue;
    for (int32_t y = 0; y < ry; ++y) {
      const int64_t C = m[(rx + y) * kCiChunk];
      if (C == 0) continue;
      const double e = (double)R * (double)C / (double)n;
      double o = (double)cnt[((int64_t)x * ry + y) * qz];
      if (adjust) o = ci_yates(o, e);
      sum += ci_term(o, e, lambda, kind);
    }
  }
  stat = scale * sum, dof = d;
}

// Workgroup b takes one chunk of kCiChunk strata of one family (bisection over multi_off: workgroup-uniform;
// packed families have an empty range there and are never found).  Small table: one work-item per
// stratum, then a fixed tree over the workgroup (work-items past the last stratum add +0.0).  General
// table (any cardinalities): the workgroup takes the chunk's strata one after the other; the marginals of
// a stratum go to LDS (integer sums: exact), work-item t adds the cells t, t + kCiChunk, ... in index order,
// the same fixed tree adds the work-items' sums, and work-item 0 adds the strata in index order.  Either
// way the order of every addition depends only on the family's own shape.
__global__ __launch_bounds__(kCiChunk) void k_fit_ci_chunk(const FitFam *__restrict__ fams,
                                                           const int64_t *__restrict__ ci_off,
                                                           const int64_t *__restrict__ multi_off, int32_t n_fam,
                                                           const int64_t *__restrict__ counts, double lambda,
                                                           int32_t kind, double scale, int32_t yates,
                                                           double *__restrict__ part, int64_t *__restrict__ part_dof) {
  __shared__ int64_t s_m[kCiSmall * kCiChunk];  // general path: R[0 .. rx), C[0 .. ry) (rx + ry <= 510)
  __shared__ double s_sum[kCiChunk];
  __shared__ int64_t s_dof[kCiChunk];
  const int32_t tid = (int32_t)threadIdx.x;
  const int64_t b = blockIdx.x;
  int32_t lo = 0, hi = n_fam;  // the last family with multi_off[lo] <= b: the one whose range holds b
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (multi_off[mid] <= b) lo = mid;
    else hi = mid;
  }
  const FitFam &F = fams[lo];
  const int32_t rx = F.card[0], ry = F.card[1];
  const int64_t qz = (int64_t)F.size / ((int64_t)rx * ry);
  const int64_t chunk = b - multi_off[lo], z0 = chunk * kCiChunk;
  const int64_t *cnt = counts + F.off;
  double sum = 0.0;
  int64_t dof = 0;
  if (rx + ry <= kCiSmall) {
    if (z0 + tid < qz) ci_stratum_small(cnt + z0 + tid, rx, ry, qz, lambda, kind, scale, yates, s_m + tid, sum, dof);
    s_sum[tid] = sum;
    s_dof[tid] = dof;
    __syncthreads();
    for (int32_t w = kCiChunk / 2; w > 0; w >>= 1) {
      if (tid < w) {
        s_sum[tid] += s_sum[tid + w];
        s_dof[tid] += s_dof[tid + w];
      }
      __syncthreads();
    }
    sum = s_sum[0], dof = s_dof[0];
  } else {
    const int64_t z_end = z0 + kCiChunk < qz ? z0 + kCiChunk : qz;
    const int32_t cells = rx * ry;
    for (int64_t z = z0; z < z_end; ++z) {
      for (int32_t k = tid; k < rx + ry; k += kCiChunk) {
        int64_t v = 0;
        if (k < rx)
          for (int32_t y = 0; y < ry; ++y) v += cnt[((int64_t)k * ry + y) * qz + z];
        else
          for (int32_t x = 0; x < rx; ++x) v += cnt[((int64_t)x * ry + (k - rx)) * qz + z];
        s_m[k] = v;
      }
      __syncthreads();
      int64_t n = 0;
      int32_t nr = 0, nc = 0;
      for (int32_t x = 0; x < rx; ++x) n += s_m[x], nr += s_m[x] > 0;
      for (int32_t y = 0; y < ry; ++y) nc += s_m[rx + y] > 0;
      const int32_t d = (nr - 1) * (nc - 1);
      if (n > 0 && d > 0) {  // workgroup-uniform: every work-item read the same marginals
        const bool adjust = yates && d == 1;
        double mine = 0.0;
        for (int32_t i = tid; i < cells; i += kCiChunk) {
          const int64_t R = s_m[i / ry], C = s_m[rx + i % ry];
          if (R == 0 || C == 0) continue;
          const double e = (double)R * (double)C / (double)n;
          double o = (double)cnt[(int64_t)i * qz + z];
          if (adjust) o = ci_yates(o, e);
          mine += ci_term(o, e, lambda, kind);
        }
        s_sum[tid] = mine;
        __syncthreads();
        for (int32_t w = kCiChunk / 2; w > 0; w >>= 1) {
          if (tid < w) s_sum[tid] += s_sum[tid + w];
          __syncthreads();
        }
        if (tid == 0) sum += scale * s_sum[0], dof += d;
      }
      __syncthreads();  // s_m and s_sum are rewritten by the next stratum
    }
  }
  if (tid == 0) {
    part[ci_off[lo] + chunk] = sum;
    part_dof[ci_off[lo] + chunk] = dof;
  }
}

// The packed families (one stratum, small table): one work-item per family, kCiChunk families per workgroup,
// so the n (n - 1) / 2 tests of PC's level 0 are one launch of n (n - 1) / 2 / kCiChunk workgroups.  The value
// is the family's only chunk partial.
__global__ __launch_bounds__(kCiChunk) void k_fit_ci_single(const FitFam *__restrict__ fams,
                                                            const int64_t *__restrict__ ci_off,
                                                            const int32_t *__restrict__ single, int32_t n_single,
                                                            const int64_t *__restrict__ counts, double lambda,
                                                            int32_t kind, double scale, int32_t yates,
                                                            double *__restrict__ part, int64_t *__restrict__ part_dof) {
  __shared__ int64_t s_m[kCiSmall * kCiChunk];
  const int64_t i = (int64_t)blockIdx.x * kCiChunk + threadIdx.x;
  if (i >= n_single) return;
  const int32_t f = single[i];
  const FitFam &F = fams[f];
  double sum;
  int64_t dof;
  ci_stratum_small(counts + F.off, F.card[0], F.card[1], 1, lambda, kind, scale, yates, s_m + threadIdx.x, sum, dof);
  part[ci_off[f]] = sum;
  part_dof[ci_off[f]] = dof;
}

// One work-item per family adds the family's chunk partials in index order and turns the sums into the
// p-value.  dof = 0: 1 without Z (chi2_contingency's answer), NaN with Z (the reference's 1 - chi2.cdf(0, 0)).
__global__ __launch_bounds__(kCiChunk) void k_fit_ci_finish(const FitFam *__restrict__ fams,
                                                            const int64_t *__restrict__ ci_off, int32_t n_fam,
                                                            const double *__restrict__ part,
                                                            const int64_t *__restrict__ part_dof,
                                                            double *__restrict__ stat, int64_t *__restrict__ dof,
                                                            double *__restrict__ pvalue) {
  const int64_t f = (int64_t)blockIdx.x * kCiChunk + threadIdx.x;
  if (f >= n_fam) return;
  double s = 0.0;
  int64_t d = 0;
  for (int64_t i = ci_off[f]; i < ci_off[f + 1]; ++i) s += part[i], d += part_dof[i];
  stat[f] = s;
  dof[f] = d;
  if (d == 0) pvalue[f] = fams[f].n_vars > 2 ? NAN : 1.0;
  else pvalue[f] = pgm_chi2_sf(s, (double)d);
}

// ---------------------------------------------------------------------------- the handle's device side
// The descriptors on the current device, and with a stage what only the score / CI launches need: the work
// lists, and per chunk one fp64 partial and one int64 count (part_obs / dof); the log-probability stage
// (pgmlogp.hip) is its block partials.
int fit_use(FitHandle *h, int stage) {
  using pgmdev::scratch;
  using pgmdev::upload;
  const FitPlan &p = h->p;
  const pgmdev::Slot base[] = {upload(h->d_fams, p.fams), upload(h->d_groups, p.groups), upload(h->d_col_off, p.col_off)};
  if (stage == kFitScore) {
    const size_t chunks = (size_t)p.chunk_off.back();
    const pgmdev::Slot score[] = {upload(h->d_chunk_off, p.chunk_off), scratch(h->d_part, chunks),
                                  scratch(h->d_part_obs, chunks)};
    return h->dev.use(kHipDevOps, base, stage, score);
  }
  if (stage == kFitCi) {
    const size_t chunks = (size_t)p.ci_off.back();
    const pgmdev::Slot ci[] = {upload(h->d_ci_off, p.ci_off), upload(h->d_ci_multi_off, p.ci_multi_off),
                               upload(h->d_ci_single, p.ci_single), scratch(h->d_ci_part, chunks),
                               scratch(h->d_ci_dof, chunks)};
    return h->dev.use(kHipDevOps, base, stage, ci);
  }
  if (stage == kFitLogp) {
    const pgmdev::Slot logp[] = {scratch(h->d_logp_part, (size_t)kLogpMaxBlocks), scratch(h->d_logp_skip, (size_t)kLogpMaxBlocks)};
    return h->dev.use(kHipDevOps, base, stage, logp);
  }
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_fit_plan_destroy(void *plan) { return pgm_plan_destroy<FitHandle>(plan); }

int pgm_fit_count(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                  const double *weights, void *tables, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  int64_t blocks = 0;
  const int st = fit_count_check(h, codes, n_cols, ld, row0, n_rows, tables, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  int up = fit_use(h);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  const uint32_t ng = (uint32_t)h->p.groups.size();
  const dim3 grid((unsigned)blocks), wg(kFitBlock);
  const size_t lds = kFitTileBins * (weights ? sizeof(double) : sizeof(uint32_t));
  const bool v4 = codes_vec4(codes, ld, row0);
#define FIT_LAUNCH(W, V4)                                                                                        \
  hipLaunchKernelGGL((k_fit_count<W, V4>), grid, wg, lds, S(stream), h->d_fams, h->d_groups, ng, codes, ld, row0, \
                     n_rows, weights, tables, h->dev.flag())
  if (weights) {
    if (v4) FIT_LAUNCH(true, true);
    else FIT_LAUNCH(true, false);
  } else {
    if (v4) FIT_LAUNCH(false, true);
    else FIT_LAUNCH(false, false);
  }
#undef FIT_LAUNCH
  // PGM_EINDEX is this call's status: the flag is read back after the launch (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad) return pgmi_fail(PGM_EINDEX, "fit_count: a state code is >= its variable's cardinality");
  return PGM_OK;
}

int pgm_fit_estep(void *plan, const int32_t *latent_cols, int32_t n_latent, const double *values, const uint8_t *codes,
                  int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, double *tables, double *loglik,
                  void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  EmSpec spec;
  int64_t blocks = 0;
  const int st = fit_estep_check(h, latent_cols, n_latent, values, codes, n_cols, ld, row0, n_rows, tables, &spec, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  int up = fit_use(h);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  hipLaunchKernelGGL(k_fit_estep, dim3((unsigned)blocks), dim3(kFitBlock), (size_t)fit_estep_lds(spec.n_lat_fam), S(stream),
                     h->d_fams, h->d_groups, (uint32_t)h->p.groups.size(), spec, values, codes, ld, row0, n_rows, tables,
                     loglik, h->dev.flag());
  // PGM_EINDEX is this call's status, as in pgm_fit_count (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad) return pgmi_fail(PGM_EINDEX, "fit_estep: a state code is >= its variable's cardinality");
  return PGM_OK;
}

int pgm_fit_finish(void *plan, const void *counts, const double *pseudo, int32_t mode, double *values, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  const int st = fit_finish_check(h, counts, mode, values);
  if (st != PGM_OK) return st;
  const int up = fit_use(h);
  if (up != PGM_OK) return up;
  const int64_t cols = h->p.col_off.back();
  const int64_t blocks = (cols + 255) / 256;
  if (blocks > INT32_MAX) return pgmi_fail(PGM_EINVAL, "fit_finish: too many CPD columns for one launch");
  const FitFam *fams = h->d_fams;
  const int64_t *col_off = h->d_col_off;
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

int pgm_fit_score(void *plan, const int64_t *counts, int32_t mode, const double *alpha, const double *beta,
                  double *scores, int64_t *n_observed, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  int64_t blocks = 0;
  const int st = fit_score_check(h, counts, mode, alpha, beta, scores, &blocks);
  if (st != PGM_OK) return st;
  const int up = fit_use(h, kFitScore);
  if (up != PGM_OK) return up;
  const FitFam *fams = h->d_fams;
  const int64_t *chunk_off = h->d_chunk_off;
  double *part = h->d_part;
  int64_t *part_obs = h->d_part_obs;
  const int32_t nf = (int32_t)h->p.fams.size(), skip = mode & PGM_SCORE_SKIP_EMPTY ? 1 : 0;
  const dim3 grid((unsigned)blocks), wg(kScoreChunk);
  if (mode & PGM_SCORE_LL)
    hipLaunchKernelGGL(k_fit_score<true>, grid, wg, 0, S(stream), fams, chunk_off, nf, counts, alpha, beta, skip, part,
                       part_obs);
  else
    hipLaunchKernelGGL(k_fit_score<false>, grid, wg, 0, S(stream), fams, chunk_off, nf, counts, alpha, beta, skip, part,
                       part_obs);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_fit_score_sum, dim3((unsigned)nf), dim3(kScoreSumBlock), 0, S(stream), chunk_off, part, part_obs,
                     scores, n_observed);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_fit_citest(void *plan, const int64_t *counts, double lambda, int32_t flags, double *stat, int64_t *dof,
                   double *pvalue, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  int64_t blocks = 0;
  const int st = fit_citest_check(h, counts, lambda, flags, stat, dof, pvalue, &blocks);
  if (st != PGM_OK) return st;
  const int up = fit_use(h, kFitCi);
  if (up != PGM_OK) return up;
  const FitFam *fams = h->d_fams;
  const int64_t *ci_off = h->d_ci_off, *multi_off = h->d_ci_multi_off;
  const int32_t *single = h->d_ci_single;
  double *part = h->d_ci_part;
  int64_t *part_dof = h->d_ci_dof;
  const int32_t nf = (int32_t)h->p.fams.size(), ns = (int32_t)h->p.ci_single.size();
  const int32_t kind = lambda == 1.0 ? 0 : lambda == 0.0 ? 1 : lambda == -1.0 ? 2 : 3;
  const double scale = kind == 0 ? 1.0 : kind == 3 ? 2.0 / (lambda * (lambda + 1.0)) : 2.0;
  const int32_t yates = flags & PGM_CI_YATES ? 1 : 0;
  const dim3 wg(kCiChunk);
  if (blocks > 0) {
    hipLaunchKernelGGL(k_fit_ci_chunk, dim3((unsigned)blocks), wg, 0, S(stream), fams, ci_off, multi_off, nf, counts,
                       lambda, kind, scale, yates, part, part_dof);
    HIP_TRY(hipGetLastError());
  }
  if (ns > 0) {
    hipLaunchKernelGGL(k_fit_ci_single, dim3((unsigned)((ns + kCiChunk - 1) / kCiChunk)), wg, 0, S(stream), fams, ci_off,
                       single, ns, counts, lambda, kind, scale, yates, part, part_dof);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_fit_ci_finish, dim3((unsigned)((nf + kCiChunk - 1) / kCiChunk)), wg, 0, S(stream), fams, ci_off, nf,
                     part, part_dof, stat, dof, pvalue);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_fit_states_observed(void *plan, const int64_t *counts, int64_t *n_states, void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  const int st = fit_states_check(h, counts, n_states);
  if (st != PGM_OK) return st;
  const int up = fit_use(h);
  if (up != PGM_OK) return up;
  hipLaunchKernelGGL(k_fit_states_observed, dim3((unsigned)h->p.fams.size()), dim3(256), 0, S(stream), h->d_fams, counts,
                     n_states);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

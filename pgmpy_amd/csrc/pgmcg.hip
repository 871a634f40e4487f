// pgmcg.hip — conditional-Gaussian structure scores of mixed data (gfx950; include/pgmhip.h "conditional-
// Gaussian scores"): the grouped moments of every family's continuous columns per configuration of its
// discrete columns as a one-hot-masked product on v_mfma_f64_16x16x4_f64 (k_cg_moments, k_cg_reduce), and
// the scores from them, one small fp64 factorisation in registers per job (k_cg_score, k_cg_score_sum).
// Replaces the reference's pandas groupby per configuration and its scipy multivariate_normal.pdf over the
// rows of each group (estimators/StructureScore.py LogLikelihoodCondGauss).  The host side (validation,
// layout, slices, passes, argument checks) is pgmcg_plan.cpp.
#include "pgm_hip_common.h"
#include "pgm_cg.h"
#include "pgm_lgs.h"

typedef double cg_v4d __attribute__((ext_vector_type(4)));
typedef double cg_v2d __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------- grouped moments
// v_mfma_f64_16x16x4_f64 computes D[i][j] += sum_k A[i][k] B[k][j] over k = 4: lane l holds A[i = l & 15]
// [k = l >> 4], B[k = l >> 4][j = l & 15] and of D the entries [row = (l >> 4) + 4 reg][col = l & 15].  k is a
// row of data.  A's row i of tile t stands for (configuration t cpt + i / mp, padded column i % mp), cpt =
// 16 / mp; B's column j is padded column j for j < mp and zero after.  A lane's padded column i % mp is the
// same in every tile and, for a lane with i < mp, is also its B column: it loads the kCgRowsPerLane = 4
// consecutive rows r + 4 q .. r + 4 q + 3 of that one column per step (k slot q of MFMA s is row r + 4 q + s,
// as in k_lg_gram) and only the comparison of the row's configuration with the tile's differs between tiles.
//
// A step's 16 configurations are computed once: lane l takes row r + (l & 15) (the four 16-lane groups agree),
// and a lane fetches those of its four rows from lanes 4 q + s.  A NaN is seen by the lane of its column
// only; the four rows' NaN bits are OR-ed over the mp lanes of an operand-row group.

// what a lane has loaded of one step
struct CgStepData {
  double raw[kCgRowsPerLane];  // its column's rows r + 4 q + s (0 past the slice or without a data column)
  int32_t cfg;                 // the configuration of row r + (lane & 15); -1: no row, a missing or a bad code
};

template <bool VEC>
__device__ inline void cg_load_step(CgStepData &o, const CgFam &F, const uint8_t *__restrict__ codes, int64_t ld_codes,
                                    const double *__restrict__ xcol, int64_t r, int64_t r_end, int lane, bool &bad) {
  const int64_t rr = r + (lane & 15);
  int32_t cfg = -1;
  if (rr < r_end) {
    bool ok = true;
    cfg = 0;
    for (int32_t d = 0; d < F.n_disc; ++d) {
      const int32_t code = codes[(int64_t)F.dcol[d] * ld_codes + rr];
      const bool state = code < F.card[d];
      bad |= !state && code != PGM_EV_MISSING;
      ok &= state;
      cfg += state ? code * F.stride[d] : 0;
    }
    cfg = ok ? cfg : -1;
  }
  o.cfg = cfg;
  const int64_t rl = r + kCgRowsPerLane * (lane >> 4), nv = r_end - rl;
  if (xcol && VEC && nv >= kCgRowsPerLane) {
    const cg_v2d a = *reinterpret_cast<const cg_v2d *>(xcol + rl), b = *reinterpret_cast<const cg_v2d *>(xcol + rl + 2);
    o.raw[0] = a[0], o.raw[1] = a[1], o.raw[2] = b[0], o.raw[3] = b[1];
  } else {
#pragma unroll
    for (int s = 0; s < kCgRowsPerLane; ++s) o.raw[s] = xcol && s < nv ? xcol[rl + s] : 0.0;
  }
}

// grid (blocks of the pass, slices), one wave each.  part: [tile of the pass][slice][reg][lane].
template <bool VEC>
__global__ __launch_bounds__(64) void k_cg_moments(const CgFam *__restrict__ fams, const CgBlock *__restrict__ blocks,
                                                   const uint8_t *__restrict__ codes, int64_t ld_codes,
                                                   const double *__restrict__ X, int64_t ld_x, int64_t row0, int64_t n_rows,
                                                   int64_t slice, const double *__restrict__ shift, double *__restrict__ part,
                                                   int64_t pass_tile_off, int32_t *__restrict__ flag) {
  const int lane = threadIdx.x, i = lane & 15, q = lane >> 4;
  const CgBlock B = blocks[blockIdx.x];
  const CgFam &F = fams[B.fam];
  const int32_t mp = F.mp, cpt = F.cpt;
  const int32_t c = i & (mp - 1);              // the lane's padded column: 0 ones, 1 .. m data, above padding
  const int32_t cfg0 = B.tile0 * cpt + i / mp;  // the configuration of its operand row in the block's first tile
  const bool is_b = i < mp;                    // it holds a B column too
  const bool data = c >= 1 && c <= F.m;
  const double *xcol = data ? X + (int64_t)F.ccol[c - 1] * ld_x + row0 : nullptr;
  const double sh = data ? shift[F.ccol[c - 1]] : 0.0;
  const double fill = c == 0 ? 1.0 : 0.0;
  const uint8_t *cw = codes + row0;
  const int64_t r_begin = (int64_t)blockIdx.y * slice;
  const int64_t r_end = r_begin + slice < n_rows ? r_begin + slice : n_rows;
  cg_v4d acc[kCgTilesPerWave];
#pragma unroll
  for (int t = 0; t < kCgTilesPerWave; ++t) acc[t] = cg_v4d{0.0, 0.0, 0.0, 0.0};
  bool bad = false;
  // the next step's loads are issued before this step's MFMAs, as in k_lg_gram
  CgStepData cur;
  cg_load_step<VEC>(cur, F, cw, ld_codes, xcol, r_begin, r_end, lane, bad);
  for (int64_t r = r_begin; r < r_end; r += kCgStep) {
    CgStepData nxt;
    cg_load_step<VEC>(nxt, F, cw, ld_codes, xcol, r + kCgStep, r_end, lane, bad);  // past the slice nothing is read
    int32_t nan_bits = 0;
#pragma unroll
    for (int s = 0; s < kCgRowsPerLane; ++s) nan_bits |= (cur.raw[s] != cur.raw[s] ? 1 : 0) << s;
    for (int32_t w = 1; w < mp; w <<= 1) nan_bits |= __shfl_xor(nan_bits, w);
    double val[kCgRowsPerLane], bv[kCgRowsPerLane];
    int32_t rel[kCgRowsPerLane];
#pragma unroll
    for (int s = 0; s < kCgRowsPerLane; ++s) {
      const int32_t cfg = __shfl(cur.cfg, kCgRowsPerLane * q + s);
      const bool live = cfg >= 0 && !((nan_bits >> s) & 1);
      val[s] = live ? (data ? cur.raw[s] - sh : fill) : 0.0;
      bv[s] = is_b ? val[s] : 0.0;
      rel[s] = live ? cfg - cfg0 : -1;
    }
#pragma unroll
    for (int s = 0; s < kCgRowsPerLane; ++s)
#pragma unroll
      for (int t = 0; t < kCgTilesPerWave; ++t) {
        if (t >= B.n_tiles) continue;  // wave-uniform
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(rel[s] == t * cpt ? val[s] : 0.0, bv[s], acc[t], 0, 0, 0);
      }
    cur = nxt;
  }
  if (bad) atomicOr(flag, 1);
  double *out = part + ((B.tile_off - pass_tile_off) * (int64_t)gridDim.y + blockIdx.y) * kCgTileDoubles;
#pragma unroll
  for (int t = 0; t < kCgTilesPerWave; ++t) {
    if (t >= B.n_tiles) continue;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) out[(int64_t)t * gridDim.y * kCgTileDoubles + reg * 64 + lane] = acc[t][reg];
  }
}

// grid (16 x blocks of the pass), 256 work-items: work-item (reg, lane) of a tile adds its entry's slice
// partials in slice order and writes it at (configuration, row column, column) of the family's block.
__global__ __launch_bounds__(kCgTileDoubles) void k_cg_reduce(const CgFam *__restrict__ fams,
                                                              const CgBlock *__restrict__ blocks,
                                                              const double *__restrict__ part, int64_t pass_tile_off,
                                                              int32_t n_slices, double *__restrict__ moments) {
  const CgBlock B = blocks[blockIdx.x / kCgTilesPerWave];
  const int32_t t = (int32_t)(blockIdx.x % kCgTilesPerWave);
  if (t >= B.n_tiles) return;
  const CgFam &F = fams[B.fam];
  const int tid = threadIdx.x, lane = tid & 63, reg = tid >> 6;
  const int32_t a = (lane >> 4) + 4 * reg, col = lane & 15;
  const int32_t cfg = (B.tile0 + t) * F.cpt + a / F.mp;
  if (col >= F.mp || cfg >= F.Q) return;
  const double *p = part + (B.tile_off - pass_tile_off + t) * (int64_t)n_slices * kCgTileDoubles + tid;
  double s = 0.0;
  for (int32_t k = 0; k < n_slices; ++k) s += p[(int64_t)k * kCgTileDoubles];
  moments[F.mom_off + ((int64_t)cfg * F.mp + a % F.mp) * F.mp + col] = s;
}

// ---------------------------------------------------------------------------- scores
// The packed lower triangle of a group's (K + 1) x (K + 1) moment block: index 0 the ones column (the count),
// 1 .. K the family's first K continuous columns.  Every index is a compile-time constant: registers.
#define CG_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))
template <int K>
__device__ __forceinline__ void cg_tri_load(const double *__restrict__ blk, int32_t mp, bool add, double (&M)[CG_TRI(K, K) + 1]) {
#pragma unroll
  for (int i = 0; i <= K; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const double x = blk[i * mp + j];
      M[CG_TRI(i, j)] = add ? M[CG_TRI(i, j)] + x : x;
    }
}

// L(g; the K columns) as `full`, L(g; the leading K - 1) as `lead`, from ONE factorisation: the pivots of the
// leading columns do not depend on the last.  drop_*: the columns the factorisation dropped, 0 under the
// identity-covariance fallback.
struct CgDensity {
  double full, lead;
  int32_t drop_full, drop_lead;
};
__device__ __forceinline__ double cg_fallback(double n, int k, double trace) {
  return -0.5 * n * ((double)k * 1.8378770664093454836) - 0.5 * trace;
}
__device__ __forceinline__ double cg_closed(double n, int r, double logdet) {
  return -0.5 * n * ((double)r * 1.8378770664093454836 + logdet) - 0.5 * (n - 1.0) * (double)r;
}
template <int K>
__device__ __forceinline__ CgDensity cg_density(const double (&M)[CG_TRI(K, K) + 1]) {
  CgDensity o = {0.0, 0.0, 0, 0};
  if constexpr (K > 0) {
    const double n = M[0];
    if (!(n > 0.0)) return o;
    double A[CG_TRI(K - 1, K - 1) + 1];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) A[CG_TRI(i, j)] = M[CG_TRI(i + 1, j + 1)] - M[CG_TRI(i + 1, 0)] * M[CG_TRI(j + 1, 0)] / n;
    double d[K], tr_lead = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      // G_ii - s_i^2 / n carries up to ~3 (n + 2) u G_ii of rounding: at or below that the column is constant
      d[i] = A[CG_TRI(i, i)] > kCgConstant * (n + 2.0) * M[CG_TRI(i + 1, i + 1)] ? A[CG_TRI(i, i)] : 0.0;
      if (i < K - 1) tr_lead += d[i];
    }
    const bool fb_full = n == 1.0 || n < (double)K, fb_lead = n == 1.0 || n < (double)(K - 1);
    // the scaled Cholesky of k_lgs_lane: outer-product form, no pivoting, a pivot at or below RCOND drops its column
    double s[K];
#pragma unroll
    for (int i = 0; i < K; ++i) s[i] = d[i] > 0.0 ? 1.0 / sqrt(d[i]) : 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) A[CG_TRI(i, j)] *= s[i] * s[j];
    int32_t r_lead = 0, r_full = 0;
    double ld_lead = 0.0, ld_full = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double p = A[CG_TRI(j, j)];
      const bool keep = p > kLgsRcond;
      const double inv = keep ? 1.0 / p : 0.0;
      const double term = keep ? log(d[j] * p / (n - 1.0)) : 0.0;  // the pivot in the units of S
      if (j < K - 1) {
        r_lead += keep ? 1 : 0;
        ld_lead += term;
      } else {
        r_full = r_lead + (keep ? 1 : 0);
        ld_full = ld_lead + term;
      }
#pragma unroll
      for (int i = j + 1; i < K; ++i) {
        const double l = A[CG_TRI(i, j)] * inv;
#pragma unroll
        for (int b = j + 1; b <= i; ++b) A[CG_TRI(i, b)] -= l * A[CG_TRI(b, j)];
      }
    }
    o.full = fb_full ? cg_fallback(n, K, tr_lead + d[K - 1]) : cg_closed(n, r_full, ld_full);
    o.drop_full = fb_full ? 0 : K - r_full;
    if (K > 1) {
      o.lead = fb_lead ? cg_fallback(n, K - 1, tr_lead) : cg_closed(n, r_lead, ld_lead);
      o.drop_lead = fb_lead ? 0 : K - 1 - r_lead;
    }
  }
  return o;
}

struct CgTerm {
  double ll, n;
  int32_t observed, dropped;
};

// job h of a family with K = m continuous columns
template <int K>
__device__ __forceinline__ CgTerm cg_job(const CgFam &F, const double *__restrict__ mom, int32_t h) {
  const int32_t mp = F.mp, blk = mp * mp;
  CgTerm o = {0.0, 0.0, 0, 0};
  double M[CG_TRI(K, K) + 1];
  if (!F.var_disc) {
    cg_tri_load<K>(mom + (int64_t)h * blk, mp, false, M);
    o.n = M[0];
    if (!(o.n > 0.0)) return o;
    const CgDensity L = cg_density<K>(M);
    const bool fb_full = o.n == 1.0 || o.n < (double)K;
    o.ll = L.full - L.lead;
    o.dropped = fb_full ? L.drop_lead : L.drop_full;
    o.observed = 1;
    return o;
  }
  // the moments of h: those of (s, h) added in state order
  const int32_t rv = F.card[0];
  for (int32_t s = 0; s < rv; ++s) cg_tri_load<K>(mom + ((int64_t)s * F.QD + h) * blk, mp, s > 0, M);
  o.n = M[0];
  if (!(o.n > 0.0)) return o;
  const CgDensity Lh = cg_density<K>(M);
  const double log_nh = log(o.n);
  o.dropped = Lh.drop_full;
  o.observed = 1;
  double sum = 0.0;
  for (int32_t s = 0; s < rv; ++s) {
    double G[CG_TRI(K, K) + 1];
    cg_tri_load<K>(mom + ((int64_t)s * F.QD + h) * blk, mp, false, G);
    if (!(G[0] > 0.0)) continue;
    const CgDensity Lg = cg_density<K>(G);
    sum += Lg.full + G[0] * (log(G[0]) - log_nh);
    o.dropped += Lg.drop_full;
  }
  o.ll = sum - Lh.full;
  return o;
}

// Workgroup b takes one chunk of kCgScoreChunk jobs of one family (bisection over chunk_off, as k_fit_score);
// a work-item takes one job.  The workgroup adds its jobs' terms in a fixed tree (work-items past the family's
// last job add +0.0) and writes one partial per chunk.
__global__ __launch_bounds__(kCgScoreChunk) void k_cg_score(const CgFam *__restrict__ fams,
                                                            const int64_t *__restrict__ chunk_off, int32_t n_fam,
                                                            const double *__restrict__ moments, double *__restrict__ part,
                                                            int64_t *__restrict__ ipart) {
  __shared__ double s_ll[kCgScoreChunk], s_n[kCgScoreChunk];
  __shared__ int32_t s_obs[kCgScoreChunk], s_drop[kCgScoreChunk];
  const int64_t b = blockIdx.x;
  int32_t lo = 0, hi = n_fam;  // chunk_off[lo] <= b < chunk_off[hi]; a family has at least one job
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= b) lo = mid;
    else hi = mid;
  }
  const CgFam &F = fams[lo];
  const int32_t tid = (int32_t)threadIdx.x;
  const int64_t job = (b - chunk_off[lo]) * kCgScoreChunk + tid;
  CgTerm t = {0.0, 0.0, 0, 0};
  if (job < F.QD) {
    const double *mom = moments + F.mom_off;
    const int32_t h = (int32_t)job;
    static_assert(kCgMaxCont == 7, "one case per number of continuous columns");
    switch (F.m) {  // workgroup-uniform
      case 0: t = cg_job<0>(F, mom, h); break;
      case 1: t = cg_job<1>(F, mom, h); break;
      case 2: t = cg_job<2>(F, mom, h); break;
      case 3: t = cg_job<3>(F, mom, h); break;
      case 4: t = cg_job<4>(F, mom, h); break;
      case 5: t = cg_job<5>(F, mom, h); break;
      case 6: t = cg_job<6>(F, mom, h); break;
      default: t = cg_job<7>(F, mom, h); break;
    }
  }
  s_ll[tid] = t.ll, s_n[tid] = t.n, s_obs[tid] = t.observed, s_drop[tid] = t.dropped;
  __syncthreads();
  for (int32_t w = kCgScoreChunk / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_ll[tid] += s_ll[tid + w];
      s_n[tid] += s_n[tid + w];  // whole numbers below 2^53: exact in any order
      s_obs[tid] += s_obs[tid + w];
      s_drop[tid] += s_drop[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[2 * b] = s_ll[0], part[2 * b + 1] = s_n[0];
    ipart[2 * b] = s_obs[0], ipart[2 * b + 1] = s_drop[0];
  }
}

// one work-item per family adds the family's chunk partials in index order (at most 32 of them)
__global__ __launch_bounds__(kCgSumBlock) void k_cg_score_sum(const int64_t *__restrict__ chunk_off, int32_t n_fam,
                                                              const double *__restrict__ part,
                                                              const int64_t *__restrict__ ipart, double *__restrict__ ll,
                                                              int64_t *__restrict__ n_complete,
                                                              int64_t *__restrict__ n_observed,
                                                              int64_t *__restrict__ n_dropped) {
  const int32_t f = (int32_t)(blockIdx.x * kCgSumBlock + threadIdx.x);
  if (f >= n_fam) return;
  double s = 0.0, n = 0.0;
  int64_t obs = 0, drop = 0;
  for (int64_t b = chunk_off[f]; b < chunk_off[f + 1]; ++b) {
    s += part[2 * b], n += part[2 * b + 1];
    obs += ipart[2 * b], drop += ipart[2 * b + 1];
  }
  ll[f] = s;
  n_complete[f] = (int64_t)n;
  n_observed[f] = obs;
  n_dropped[f] = drop;
}

// ---------------------------------------------------------------------------- the handle's device side
static int cg_use(CgHandle *h, int stage) {
  using pgmdev::scratch;
  using pgmdev::upload;
  const CgPlan &p = h->p;
  const pgmdev::Slot base[] = {upload(h->d_fams, p.fams), upload(h->d_blocks, p.blocks), upload(h->d_chunk_off, p.chunk_off)};
  if (stage == kCgMomentStage) {
    const pgmdev::Slot st[] = {scratch(h->d_part, (size_t)p.stage_tiles * kCgTileDoubles)};
    return h->dev.use(kHipDevOps, base, stage, st);
  }
  const size_t chunks = (size_t)p.chunk_off.back();
  const pgmdev::Slot st[] = {scratch(h->d_score_part, 2 * chunks), scratch(h->d_score_ipart, 2 * chunks)};
  return h->dev.use(kHipDevOps, base, stage, st);
}

extern "C" {

int pgm_cg_plan_destroy(void *plan) { return pgm_plan_destroy<CgHandle>(plan); }

int pgm_cg_moments(void *plan, const uint8_t *codes, int32_t n_code_cols, int64_t ld_codes, const double *X,
                   int32_t n_value_cols, int64_t ld_x, int64_t row0, int64_t n_rows, const double *shift, double *moments,
                   void *stream) {
  CgHandle *h = static_cast<CgHandle *>(plan);
  int64_t slice = 0, n_slices = 0;
  const int st = cg_moments_check(h, codes, n_code_cols, ld_codes, X, n_value_cols, ld_x, row0, n_rows, shift, moments, &slice,
                                  &n_slices);
  if (st != PGM_OK) return st;
  int up = cg_use(h, kCgMomentStage);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  std::vector<CgPass> passes;
  cg_passes(h->p, n_slices, passes);
  const bool vec = cg_vec16(X, ld_x, row0);
  for (const CgPass &ps : passes) {
    const CgBlock *blocks = h->d_blocks + ps.block0;
    if (n_slices > 0) {
      const dim3 grid((unsigned)ps.n_blocks, (unsigned)n_slices), wg(64);
      if (vec)
        hipLaunchKernelGGL(k_cg_moments<true>, grid, wg, 0, S(stream), h->d_fams, blocks, codes, ld_codes, X, ld_x, row0, n_rows,
                           slice, shift, h->d_part, ps.tile_off, h->dev.flag());
      else
        hipLaunchKernelGGL(k_cg_moments<false>, grid, wg, 0, S(stream), h->d_fams, blocks, codes, ld_codes, X, ld_x, row0, n_rows,
                           slice, shift, h->d_part, ps.tile_off, h->dev.flag());
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cg_reduce, dim3((unsigned)(ps.n_blocks * kCgTilesPerWave)), dim3(kCgTileDoubles), 0, S(stream), h->d_fams,
                       blocks, h->d_part, ps.tile_off, (int32_t)n_slices, moments);
    HIP_TRY(hipGetLastError());
  }
  // PGM_EINDEX is this call's status, as in pgm_fit_count (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad) return pgmi_fail(PGM_EINDEX, "cg_moments: a state code is >= its variable's cardinality");
  return PGM_OK;
}

int pgm_cg_score(void *plan, const double *moments, const double *shift, double *ll, int64_t *n_complete, int64_t *n_observed,
                 int64_t *n_dropped, void *stream) {
  (void)shift;  // the centred scatter does not depend on it
  CgHandle *h = static_cast<CgHandle *>(plan);
  const int st = cg_score_check(h, moments, ll, n_complete, n_observed, n_dropped);
  if (st != PGM_OK) return st;
  const int up = cg_use(h, kCgScoreStage);
  if (up != PGM_OK) return up;
  const int32_t nf = (int32_t)h->p.fams.size();
  hipLaunchKernelGGL(k_cg_score, dim3((unsigned)h->p.chunk_off.back()), dim3(kCgScoreChunk), 0, S(stream), h->d_fams,
                     h->d_chunk_off, nf, moments, h->d_score_part, h->d_score_ipart);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_cg_score_sum, dim3((unsigned)((nf + kCgSumBlock - 1) / kCgSumBlock)), dim3(kCgSumBlock), 0, S(stream),
                     h->d_chunk_off, nf, h->d_score_part, h->d_score_ipart, ll, n_complete, n_observed, n_dropped);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

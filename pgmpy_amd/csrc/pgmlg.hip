// pgmlg.hip — linear-Gaussian networks on a resident fp64 value matrix (gfx950): the column sums and the
// shifted Gram matrix every OLS fit is a function of (k_lg_colsum, k_lg_gram on v_mfma_f64_16x16x4_f64),
// forward sampling on the Philox stream of pgm_sample.h (k_lg_sample), the factorised log-density
// (k_lg_logpdf) and the per-row affine map of a conditional mean (k_lg_affine), with their C-ABI.  Replaces
// the reference's per-node scikit-learn regressions, its scipy logpdf and its numpy multivariate_normal
// (models/LinearGaussianBayesianNetwork.py).  The host side (validation, groups, slices, argument checks)
// is pgmlg_plan.cpp.
#include "pgm_hip_common.h"
#include "pgm_lg.h"
#include "pgm_sample.h"

typedef double lg_v4d __attribute__((ext_vector_type(4)));
typedef double lg_v2d __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------- column sums
// grid (pieces, d): workgroup (p, j) adds the rows [p, p + 1) * chunk of column cols[j]; work-item t takes
// the rows t, t + 256, ... of the piece in order, then the fixed tree.
__global__ __launch_bounds__(kLgColsumBlock) void k_lg_colsum(const int32_t *__restrict__ cols,
                                                              const double *__restrict__ X, int64_t ld, int64_t row0,
                                                              int64_t n_rows, int64_t chunk, double *__restrict__ part) {
  __shared__ double red[kLgColsumBlock];
  const int32_t tid = (int32_t)threadIdx.x;
  const double *x = X + (int64_t)cols[blockIdx.y] * ld + row0;
  const int64_t r_begin = (int64_t)blockIdx.x * chunk;
  const int64_t r_end = r_begin + chunk < n_rows ? r_begin + chunk : n_rows;
  double s = 0.0;
  for (int64_t r = r_begin + tid; r < r_end; r += kLgColsumBlock) s += x[r];
  red[tid] = s;
  __syncthreads();
  for (int32_t w = kLgColsumBlock / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// one work-item per column adds its pieces in index order
__global__ __launch_bounds__(kLgColsumBlock) void k_lg_colsum_reduce(const double *__restrict__ part, int32_t d,
                                                                     int32_t n_chunks, int64_t n_rows,
                                                                     double *__restrict__ sums,
                                                                     int64_t *__restrict__ counts) {
  const int32_t j = (int32_t)(blockIdx.x * kLgColsumBlock + threadIdx.x);
  if (j >= d) return;
  double s = 0.0;
  for (int32_t p = 0; p < n_chunks; ++p) s += part[(int64_t)j * n_chunks + p];
  sums[j] = s;
  counts[j] = n_rows;
}

// ---------------------------------------------------------------------------- the Gram matrix
// v_mfma_f64_16x16x4_f64 computes D[i][j] += sum_k A[i][k] B[k][j] over k = 4.  Lane l holds A[i = l & 15]
// [k = l >> 4] and B[k = l >> 4][j = l & 15], and of D the four entries [row = (l >> 4) + 4 reg][col = l & 15]
// (the comment above k_gemm_f64).  Here k is a row of data, A's row i is column 16 ti + i of the padded
// column list and B's column j is column 16 tj + j of it: both operands are the same matrix, so a lane's A
// value of a tile is also its B value of that tile, and a diagonal group loads one side only.
//
// The row a k slot stands for is free as long as both sides agree.  Lane (i, q = l >> 4) therefore holds the
// kLgRowsPerLane = 4 CONSECUTIVE rows r + 4 q .. r + 4 q + 3 of its column, and MFMA s of the step takes the
// s-th of them on both sides: k slot q of MFMA s is row r + 4 q + s.  A lane reads 32 contiguous bytes of a
// column and step, a wave 128 per column, against 8 and 32 with k slot q = row r + q.
//
// A lane's value of a row is x - shift inside the slice and 0 at or past its end; the ones column is 1 and 0;
// a padding column is 0.  VEC (X, ld * 8 and row0 * 8 multiples of 16): a lane whose four rows are inside the
// slice takes two 16-byte loads; any other lane, and every lane without VEC, takes guarded 8-byte loads.
//
// the raw four rows of one column at p (rows past n_valid are not read)
template <bool VEC>
__device__ inline void lg_load4(const double *__restrict__ p, int64_t n_valid, double (&v)[kLgRowsPerLane]) {
  if (VEC && n_valid >= kLgRowsPerLane) {
    const lg_v2d a = *reinterpret_cast<const lg_v2d *>(p), b = *reinterpret_cast<const lg_v2d *>(p + 2);
    v[0] = a[0], v[1] = a[1], v[2] = b[0], v[3] = b[1];
    return;
  }
#pragma unroll
  for (int s = 0; s < kLgRowsPerLane; ++s) v[s] = s < n_valid ? p[s] : 0.0;
}

// one side of a group: what the lane's column of each of the four tiles is
struct LgSide {
  const double *p[kLgSuper];  // the column's window, nullptr: not a data column
  double shift[kLgSuper];
  double fill[kLgSuper];      // the value of a row inside the slice when there is no load: 1 (ones) or 0 (padding)
  bool on[kLgSuper];          // the tile is inside the matrix (wave-uniform)
};
__device__ inline void lg_side(LgSide &s, const int32_t *__restrict__ lane_col, int32_t super, int32_t n_tiles,
                               const double *__restrict__ X, int64_t ld, int64_t row0, const double *__restrict__ shift,
                               int lane) {
#pragma unroll
  for (int t = 0; t < kLgSuper; ++t) {
    const int32_t j = (super * kLgSuper + t) * kLgTile + (lane & 15);
    const int32_t c = lane_col[j];
    s.on[t] = super * kLgSuper + t < n_tiles;
    s.p[t] = c >= 0 ? X + (int64_t)c * ld + row0 : nullptr;
    s.shift[t] = c >= 0 ? shift[j] : 0.0;
    s.fill[t] = c == kLgOnes ? 1.0 : 0.0;
  }
}
template <bool VEC>
__device__ inline void lg_load_side(const LgSide &s, int64_t rl, int64_t nv, double (&raw)[kLgSuper][kLgRowsPerLane]) {
#pragma unroll
  for (int t = 0; t < kLgSuper; ++t) {
    if (s.on[t] && s.p[t]) {
      lg_load4<VEC>(s.p[t] + rl, nv, raw[t]);
    } else {
#pragma unroll
      for (int k = 0; k < kLgRowsPerLane; ++k) raw[t][k] = 0.0;
    }
  }
}
// raw rows to operand values: the shift inside the slice, zero past it
__device__ inline void lg_operand(const LgSide &s, int64_t nv, const double (&raw)[kLgSuper][kLgRowsPerLane],
                                  double (&f)[kLgSuper][kLgRowsPerLane]) {
#pragma unroll
  for (int t = 0; t < kLgSuper; ++t)
#pragma unroll
    for (int k = 0; k < kLgRowsPerLane; ++k) f[t][k] = k < nv ? (s.p[t] ? raw[t][k] - s.shift[t] : s.fill[t]) : 0.0;
}

// the accumulation of one (group, slice); DIAG: I == J, one side, the accumulators a <= b
template <bool VEC, bool DIAG>
__device__ inline void lg_gram_body(const LgSide &sa, const LgSide &sb, int64_t r_begin, int64_t r_end, int lane,
                                    lg_v4d (&acc)[kLgSuper][kLgSuper]) {
  const int q = lane >> 4;
  // The raw rows of step r + 1 are loaded before step r's are turned into operands, so a wave's loads are in
  // flight under its own MFMA work (one wave per SIMD hides nothing by itself).
  double wa[kLgSuper][kLgRowsPerLane], wb[kLgSuper][kLgRowsPerLane];
  int64_t r = r_begin;
  lg_load_side<VEC>(sa, r + kLgRowsPerLane * q, r_end - (r + kLgRowsPerLane * q), wa);
  if (!DIAG) lg_load_side<VEC>(sb, r + kLgRowsPerLane * q, r_end - (r + kLgRowsPerLane * q), wb);
  for (; r < r_end; r += kLgStep) {
    const int64_t rl = r + kLgRowsPerLane * q, nv = r_end - rl;
    double na[kLgSuper][kLgRowsPerLane], nb[kLgSuper][kLgRowsPerLane];
    // past the slice's end nothing is read: n_valid <= 0
    lg_load_side<VEC>(sa, rl + kLgStep, nv - kLgStep, na);
    if (!DIAG) lg_load_side<VEC>(sb, rl + kLgStep, nv - kLgStep, nb);
    double fa[kLgSuper][kLgRowsPerLane], fb[kLgSuper][kLgRowsPerLane];
    lg_operand(sa, nv, wa, fa);
    if (!DIAG) lg_operand(sb, nv, wb, fb);
#pragma unroll
    for (int k = 0; k < kLgRowsPerLane; ++k)
#pragma unroll
      for (int a = 0; a < kLgSuper; ++a)
#pragma unroll
        for (int b = 0; b < kLgSuper; ++b) {
          if (DIAG && a > b) continue;
          if (!sa.on[a] || !sb.on[b]) continue;
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a][k], DIAG ? fa[b][k] : fb[b][k], acc[a][b], 0, 0, 0);
        }
#pragma unroll
    for (int t = 0; t < kLgSuper; ++t)
#pragma unroll
      for (int k = 0; k < kLgRowsPerLane; ++k) {
        wa[t][k] = na[t][k];
        if (!DIAG) wb[t][k] = nb[t][k];
      }
  }
}

// grid (groups, slices), one wave each.  part: [slice][group][a * 4 + b][reg][lane].
template <bool VEC>
__global__ __launch_bounds__(64) void k_lg_gram(const int32_t *__restrict__ lane_col, const LgGroup *__restrict__ groups,
                                                int32_t n_tiles, const double *__restrict__ X, int64_t ld, int64_t row0,
                                                int64_t n_rows, int64_t slice, const double *__restrict__ shift,
                                                double *__restrict__ part) {
  const int lane = threadIdx.x;
  const LgGroup g = groups[blockIdx.x];
  const int64_t r_begin = (int64_t)blockIdx.y * slice;
  const int64_t r_end = r_begin + slice < n_rows ? r_begin + slice : n_rows;
  lg_v4d acc[kLgSuper][kLgSuper];
#pragma unroll
  for (int a = 0; a < kLgSuper; ++a)
#pragma unroll
    for (int b = 0; b < kLgSuper; ++b) acc[a][b] = lg_v4d{0.0, 0.0, 0.0, 0.0};
  LgSide sa;
  lg_side(sa, lane_col, g.I, n_tiles, X, ld, row0, shift, lane);
  if (g.I == g.J) {
    lg_gram_body<VEC, true>(sa, sa, r_begin, r_end, lane, acc);
  } else {
    LgSide sb;
    lg_side(sb, lane_col, g.J, n_tiles, X, ld, row0, shift, lane);
    lg_gram_body<VEC, false>(sa, sb, r_begin, r_end, lane, acc);
  }
  double *out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (kLgAccPerGroup * kLgAccDoubles);
#pragma unroll
  for (int a = 0; a < kLgSuper; ++a)
#pragma unroll
    for (int b = 0; b < kLgSuper; ++b) {
      if (g.I == g.J && a > b) continue;
      if (g.I * kLgSuper + a >= n_tiles || g.J * kLgSuper + b >= n_tiles) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) out[(a * kLgSuper + b) * kLgAccDoubles + reg * 64 + lane] = acc[a][b][reg];
    }
}

// grid (16 accumulators, groups), 256 work-items: work-item (reg, lane) adds its entry's slice partials in slice
// order and writes it at [row][col] and [col][row] of the (d + 1) x (d + 1) matrix (upper-triangle entries only).
__global__ __launch_bounds__(kLgAccDoubles) void k_lg_gram_reduce(const LgGroup *__restrict__ groups, int32_t n_tiles,
                                                                  int32_t d1, const double *__restrict__ part,
                                                                  int32_t n_slices, double *__restrict__ out) {
  const LgGroup g = groups[blockIdx.y];
  const int a = blockIdx.x / kLgSuper, b = blockIdx.x % kLgSuper;
  if (g.I == g.J && a > b) return;
  const int32_t ti = g.I * kLgSuper + a, tj = g.J * kLgSuper + b;
  if (ti >= n_tiles || tj >= n_tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, reg = tid >> 6;
  const int32_t row = ti * kLgTile + (lane >> 4) + 4 * reg, col = tj * kLgTile + (lane & 15);
  if (row > col || col >= d1) return;
  const int64_t stride = (int64_t)gridDim.y * (kLgAccPerGroup * kLgAccDoubles);
  const double *p = part + ((int64_t)blockIdx.y * kLgAccPerGroup + blockIdx.x) * kLgAccDoubles + tid;
  double s = 0.0;
  for (int32_t k = 0; k < n_slices; ++k) s += p[(int64_t)k * stride];
  out[(int64_t)row * d1 + col] = s;
  out[(int64_t)col * d1 + row] = s;
}

// ---------------------------------------------------------------------------- sampling
// One lane per row, families in plan order.  The coefficient, offset and column reads are the same for
// every lane (scalar loads).  The normal of (stream row, column c): one Philox call per column pair, kept
// for the next family when that is the pair's other column.
__global__ __launch_bounds__(kLgBlock) void k_lg_sample(const int32_t *__restrict__ fam_off,
                                                        const int32_t *__restrict__ fam_cols, int32_t n_fams,
                                                        const double *__restrict__ coef, double *X, int64_t ld,
                                                        int64_t row0, int64_t n_rows, uint64_t first_row, uint64_t seed) {
  const int64_t r = (int64_t)blockIdx.x * kLgBlock + threadIdx.x;
  if (r >= n_rows) return;
  const uint64_t srow = first_row + (uint64_t)r;
  double *x = X + row0 + r;
  uint32_t have = 0xffffffffu;
  double zc = 0.0, zs = 0.0;
  for (int32_t f = 0; f < n_fams; ++f) {
    const int32_t o = fam_off[f], np = fam_off[f + 1] - o - 1;
    const double *cf = coef + o + f;
    const int32_t col = fam_cols[o];
    double m = cf[0];
    for (int32_t i = 0; i < np; ++i) m += cf[1 + i] * x[(int64_t)fam_cols[o + 1 + i] * ld];
    const uint32_t pair = (uint32_t)col >> 1;
    if (pair != have) {
      uint32_t w[4];
      philox4x32_10((uint32_t)srow, (uint32_t)(srow >> 32), pair, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
      const double u0 = (double)(((uint64_t)w[0] << 21) | (w[1] >> 11)) * 0x1.0p-53;
      const double u1 = (double)(((uint64_t)w[2] << 21) | (w[3] >> 11)) * 0x1.0p-53;
      const double rho = sqrt(-2.0 * log(1.0 - u0));
      double sn, cs;
      sincospi(2.0 * u1, &sn, &cs);
      zc = rho * cs;
      zs = rho * sn;
      have = pair;
    }
    x[(int64_t)col * ld] = m + cf[1 + np] * (col & 1 ? zs : zc);
  }
}

// ---------------------------------------------------------------------------- log-density
// One lane per row; the workgroup's partial of `total` is the fixed tree over its 256 rows (+0.0 past the
// window), the partials are added by k_lg_logpdf_sum as k_fit_logprob_sum adds its own.
__global__ __launch_bounds__(kLgBlock) void k_lg_logpdf(const int32_t *__restrict__ fam_off,
                                                        const int32_t *__restrict__ fam_cols, int32_t n_fams,
                                                        const double *__restrict__ coef, const double *__restrict__ konst,
                                                        const double *__restrict__ X, int64_t ld, int64_t row0,
                                                        int64_t n_rows, double *__restrict__ logp,
                                                        double *__restrict__ part) {
  __shared__ double red[kLgBlock];
  const int32_t tid = (int32_t)threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kLgBlock + tid;
  double lp = 0.0;
  if (r < n_rows) {
    const double *x = X + row0 + r;
    for (int32_t f = 0; f < n_fams; ++f) {
      const int32_t o = fam_off[f], np = fam_off[f + 1] - o - 1;
      const double *cf = coef + o + f;
      double m = cf[0];
      for (int32_t i = 0; i < np; ++i) m += cf[1 + i] * x[(int64_t)fam_cols[o + 1 + i] * ld];
      const double t = (x[(int64_t)fam_cols[o] * ld] - m) / cf[1 + np];
      lp += konst[f] - 0.5 * (t * t);
    }
    if (logp) logp[r] = lp;
  }
  red[tid] = lp;
  __syncthreads();
  for (int32_t w = kLgBlock / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kLgBlock) void k_lg_logpdf_sum(const double *__restrict__ part, int32_t n,
                                                            double *__restrict__ total) {
  __shared__ double red[kLgBlock];
  const int32_t tid = (int32_t)threadIdx.x;
  double s = 0.0;
  for (int32_t i = tid; i < n; i += kLgBlock) s += part[i];
  red[tid] = s;
  __syncthreads();
  for (int32_t w = kLgBlock / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) *total = red[0];
}

// ---------------------------------------------------------------------------- the affine map
struct LgAffineCols {
  int32_t c[kLgAffineChunk];
};
// grid (row blocks, outputs): the input columns first .. first + n of the map, added in order
__global__ __launch_bounds__(kLgBlock) void k_lg_affine(const LgAffineCols cols, int32_t first, int32_t n,
                                                        const double *__restrict__ W, int32_t n_in,
                                                        const double *__restrict__ c, const double *__restrict__ X,
                                                        int64_t ld, int64_t row0, int64_t n_rows, double *out,
                                                        int64_t ld_out) {
  const int64_t r = (int64_t)blockIdx.x * kLgBlock + threadIdx.x;
  if (r >= n_rows) return;
  const int32_t j = (int32_t)blockIdx.y;
  double *o = out + (int64_t)j * ld_out + r;
  const double *w = W + (int64_t)j * n_in + first;
  double acc = first == 0 ? c[j] : *o;
  for (int32_t i = 0; i < n; ++i) acc += w[i] * X[(int64_t)cols.c[i] * ld + row0 + r];
  *o = acc;
}

// ---------------------------------------------------------------------------- the handles' device side
static int lg_gram_use(LgGramHandle *h, int stage) {
  using pgmdev::scratch;
  using pgmdev::upload;
  const LgGramPlan &p = h->p;
  const pgmdev::Slot base[] = {upload(h->d_lane_col, p.lane_col), upload(h->d_groups, p.groups), upload(h->d_cols, p.cols)};
  if (stage == kLgGramStage) {
    const pgmdev::Slot st[] = {scratch(h->d_part, (size_t)p.max_slices * p.groups.size() * kLgAccPerGroup * kLgAccDoubles)};
    return h->dev.use(kHipDevOps, base, stage, st);
  }
  const pgmdev::Slot st[] = {scratch(h->d_colpart, (size_t)p.d * kLgColsumMaxChunks)};
  return h->dev.use(kHipDevOps, base, stage, st);
}

static int lg_net_use(LgNetHandle *h, bool partials) {
  using pgmdev::scratch;
  using pgmdev::upload;
  const pgmdev::Slot base[] = {upload(h->d_fam_off, h->p.fam_off), upload(h->d_fam_cols, h->p.fam_cols)};
  if (!partials) return h->dev.use(kHipDevOps, base);
  const pgmdev::Slot st[] = {scratch(h->d_part, (size_t)kLgMaxBlocks)};
  return h->dev.use(kHipDevOps, base, 0, st);
}

extern "C" {

int pgm_lg_gram_plan_destroy(void *plan) { return pgm_plan_destroy<LgGramHandle>(plan); }
int pgm_lg_net_destroy(void *plan) { return pgm_plan_destroy<LgNetHandle>(plan); }

int pgm_lg_colsum(void *plan, const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, double *sums,
                  int64_t *counts, void *stream) {
  LgGramHandle *h = static_cast<LgGramHandle *>(plan);
  int64_t chunk = 0, n_chunks = 0;
  const int st = lg_colsum_check(h, X, n_cols, ld, row0, n_rows, sums, counts, &chunk, &n_chunks);
  if (st != PGM_OK) return st;
  if (n_chunks == 0) return PGM_OK;
  const int up = lg_gram_use(h, kLgColsumStage);
  if (up != PGM_OK) return up;
  const int32_t d = h->p.d;
  // grid.y holds 65,535 columns: more go in several launches over the same pieces
  for (int32_t j0 = 0; j0 < d; j0 += 65535) {
    const int32_t nj = d - j0 < 65535 ? d - j0 : 65535;
    hipLaunchKernelGGL(k_lg_colsum, dim3((unsigned)n_chunks, (unsigned)nj), dim3(kLgColsumBlock), 0, S(stream),
                       h->d_cols + j0, X, ld, row0, n_rows, chunk, h->d_colpart + (int64_t)j0 * n_chunks);
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_lg_colsum_reduce, dim3((unsigned)((d + kLgColsumBlock - 1) / kLgColsumBlock)), dim3(kLgColsumBlock),
                     0, S(stream), h->d_colpart, d, (int32_t)n_chunks, n_rows, sums, counts);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_lg_gram(void *plan, const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                const double *shift, double *out, void *stream) {
  LgGramHandle *h = static_cast<LgGramHandle *>(plan);
  int64_t slice = 0, n_slices = 0;
  const int st = lg_gram_check(h, X, n_cols, ld, row0, n_rows, shift, out, &slice, &n_slices);
  if (st != PGM_OK) return st;
  if (n_slices == 0) return PGM_OK;
  const int up = lg_gram_use(h, kLgGramStage);
  if (up != PGM_OK) return up;
  const LgGramPlan &p = h->p;
  const dim3 grid((unsigned)p.groups.size(), (unsigned)n_slices), wg(64);
  if (lg_vec16(X, ld, row0))
    hipLaunchKernelGGL(k_lg_gram<true>, grid, wg, 0, S(stream), h->d_lane_col, h->d_groups, p.n_tiles, X, ld, row0, n_rows,
                       slice, shift, h->d_part);
  else
    hipLaunchKernelGGL(k_lg_gram<false>, grid, wg, 0, S(stream), h->d_lane_col, h->d_groups, p.n_tiles, X, ld, row0, n_rows,
                       slice, shift, h->d_part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_lg_gram_reduce, dim3(kLgAccPerGroup, (unsigned)p.groups.size()), dim3(kLgAccDoubles), 0, S(stream),
                     h->d_groups, p.n_tiles, p.d + 1, h->d_part, (int32_t)n_slices, out);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_lg_sample(void *plan, const double *coef, double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                  int64_t first_row, uint64_t seed, void *stream) {
  LgNetHandle *h = static_cast<LgNetHandle *>(plan);
  int64_t blocks = 0;
  const int st = lg_sample_check(h, coef, X, n_cols, ld, row0, n_rows, first_row, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  const int up = lg_net_use(h, false);
  if (up != PGM_OK) return up;
  hipLaunchKernelGGL(k_lg_sample, dim3((unsigned)blocks), dim3(kLgBlock), 0, S(stream), h->d_fam_off, h->d_fam_cols,
                     (int32_t)h->p.fam_off.size() - 1, coef, X, ld, row0, n_rows, (uint64_t)first_row, seed);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_lg_logpdf(void *plan, const double *coef, const double *konst, const double *X, int32_t n_cols, int64_t ld,
                  int64_t row0, int64_t n_rows, double *logp, double *total, void *stream) {
  LgNetHandle *h = static_cast<LgNetHandle *>(plan);
  int64_t blocks = 0;
  const int st = lg_logpdf_check(h, coef, konst, X, n_cols, ld, row0, n_rows, logp, total, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  const int up = lg_net_use(h, true);
  if (up != PGM_OK) return up;
  hipLaunchKernelGGL(k_lg_logpdf, dim3((unsigned)blocks), dim3(kLgBlock), 0, S(stream), h->d_fam_off, h->d_fam_cols,
                     (int32_t)h->p.fam_off.size() - 1, coef, konst, X, ld, row0, n_rows, logp, h->d_part);
  HIP_TRY(hipGetLastError());
  if (total) {
    hipLaunchKernelGGL(k_lg_logpdf_sum, dim3(1), dim3(kLgBlock), 0, S(stream), h->d_part, (int32_t)blocks, total);
    HIP_TRY(hipGetLastError());
  }
  return PGM_OK;
}

int pgm_lg_affine(const double *W, const double *c, const int32_t *in_cols, int32_t n_in, int32_t n_out, const double *X,
                  int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, double *out, int64_t ld_out, void *stream) {
  int64_t blocks = 0;
  const int st = lg_affine_check(W, c, in_cols, n_in, n_out, X, n_cols, ld, row0, n_rows, out, ld_out, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  const dim3 grid((unsigned)blocks, (unsigned)n_out), wg(kLgBlock);
  int32_t first = 0;
  do {  // n_in == 0: one launch writes the constants
    LgAffineCols cols = {};
    const int32_t n = n_in - first < kLgAffineChunk ? n_in - first : kLgAffineChunk;
    for (int32_t i = 0; i < n; ++i) cols.c[i] = in_cols[first + i];
    hipLaunchKernelGGL(k_lg_affine, grid, wg, 0, S(stream), cols, first, n, W, n_in, c, X, ld, row0, n_rows, out, ld_out);
    HIP_TRY(hipGetLastError());
    first += n;
  } while (first < n_in);
  return PGM_OK;
}
}

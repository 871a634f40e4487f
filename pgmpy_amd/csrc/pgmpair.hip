// pgmpair.hip — the contingency tables of every pair of columns in one launch (gfx950), and the pair
// statistics the tree learners weigh their edges with: k_pair_count (int8 MFMA), k_pair_mi, k_pair_emi and
// their C-ABI (pgm_pair_plan_destroy, pgm_pair_count, pgm_pair_mi, pgm_pair_emi).  Replaces the reference's
// per-pair scikit-learn calls (estimators/TreeSearch.py:196-356).  The host side (validation, the state
// table, the group list, the slice choice, the argument checks) is pgmpair_plan.cpp.
#include "pgm_hip_common.h"
#include "pgm_pair.h"

typedef int pair_v4i __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------- counting
// With O the rows x S one-hot matrix of the codes (S = all states laid end to end), G = O^T O holds the
// table of every pair of variables as a block.  0/1 int8 operands and int32 accumulation are exact.
//
// v_mfma_i32_16x16x64_i8 computes D[i][j] += sum_k A[i][k] B[k][j] over k = 64 rows.  Lane l holds the 16
// bytes A[i = l & 15][k = 16 (l >> 4) .. + 16) and B[k = 16 (l >> 4) .. + 16)][j = l & 15], and of D the
// four entries [i = 4 (l >> 4) + reg][j = l & 15].  Here A's row i is state 16 ti + i and B's column j is
// state 16 tj + j, so the lane's A fragment is the 16 code bytes of its A state's column at the rows
// 16 (l >> 4) .. + 16 of the step, each byte turned into (byte == local state), and its B fragment the
// same for its B state.  Both sides read the same rows at the same k, so the order of k inside the
// instruction does not matter; the row / column maps do (the asymmetric tables of tests/test_pairs_gpu.py).
//
// Missing cells need nothing: 255 matches no state, so a row is left out of exactly the pairs it is missing
// in.  Rows at or past the slice's end are read as 255.  With a stratum column the A fragment is and-ed with
// (stratum byte == blockIdx.z).
//
// Every load is 16 aligned bytes inside a column when codes, ld and row0 are multiples of 16 (vec) and the
// lane's 16 rows are inside the window; any other fragment is read byte by byte, each byte guarded.
//
// 0x01 in every byte of w that equals the byte repeated in krep (exact: no carry crosses a byte)
__device__ inline uint32_t pair_eq_bytes(uint32_t w, uint32_t krep) {
  const uint32_t x = w ^ krep;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return (~(t | x) & 0x80808080u) >> 7;
}
// bit 7 of every byte b of w with card <= b <= 254 (neither a state nor missing): with y = b + 1 (mod 256)
// that is y >= card + 1; c7 / ch are the low seven bits / the top bit of card + 1 in every byte
__device__ inline uint32_t pair_bad_bytes(uint32_t w, uint32_t c7, uint32_t ch) {
  const uint32_t y = ((w & 0x7f7f7f7fu) + 0x01010101u) ^ (w & 0x80808080u);
  const uint32_t d = (y | 0x80808080u) - c7;  // bit 7: low seven bits of y >= those of card + 1
  return (y & ~ch) | (~(y ^ ch) & d);
}
// the lane's 16 code bytes at p; n_valid <= 0 reads nothing (all 255)
__device__ inline uint4 pair_load16(const uint8_t *__restrict__ p, int64_t n_valid, bool vec) {
  if (vec && n_valid >= 16) return *reinterpret_cast<const uint4 *>(p);
  uint32_t w[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  const int n = n_valid < 16 ? (int)(n_valid < 0 ? 0 : n_valid) : 16;
  for (int j = 0; j < n; ++j) w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | ((uint32_t)p[j] << (8 * (j & 3)));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(kPairBlock) void k_pair_count(const PairState *__restrict__ states,
                                                           const PairGroup *__restrict__ groups,
                                                           const uint8_t *__restrict__ codes, int64_t ld, int64_t row0,
                                                           int64_t n_rows, int64_t slice, int32_t strat_col, int32_t vec,
                                                           unsigned long long *__restrict__ counts, int64_t Sp,
                                                           int32_t *__restrict__ err) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PairGroup g = groups[blockIdx.x];
  const int64_t r_begin = (int64_t)blockIdx.y * slice;
  const int64_t r_end = r_begin + slice < n_rows ? r_begin + slice : n_rows;
  const bool diag = g.I == g.J;
  const bool check_a = (g.check & 1) && blockIdx.z == 0, check_b = (g.check & 2) && blockIdx.z == 0;

  const uint8_t *pa[kPairSuper], *pb[kPairSuper];
  uint32_t ka[kPairSuper], kb[kPairSuper], c7a[kPairSuper], cha[kPairSuper], c7b[kPairSuper], chb[kPairSuper];
  bool on_a[kPairSuper], on_b[kPairSuper];
#pragma unroll
  for (int t = 0; t < kPairSuper; ++t) {
    const PairState a = states[(int64_t)g.I * kPairSuperStates + t * kPairTile + (lane & 15)];
    const PairState b = states[(int64_t)g.J * kPairSuperStates + t * kPairTile + (lane & 15)];
    pa[t] = codes + (int64_t)a.col * ld + row0;
    pb[t] = codes + (int64_t)b.col * ld + row0;
    ka[t] = (uint32_t)a.k * 0x01010101u;
    kb[t] = (uint32_t)b.k * 0x01010101u;
    const uint32_t ca = (uint32_t)(a.card + 1) * 0x01010101u, cb = (uint32_t)(b.card + 1) * 0x01010101u;
    c7a[t] = ca & 0x7f7f7f7fu;
    cha[t] = ca & 0x80808080u;
    c7b[t] = cb & 0x7f7f7f7fu;
    chb[t] = cb & 0x80808080u;
    on_a[t] = !a.pad;
    on_b[t] = !b.pad;
  }
  const uint8_t *ps = strat_col >= 0 ? codes + (int64_t)strat_col * ld + row0 : nullptr;
  const uint32_t crep = (uint32_t)blockIdx.z * 0x01010101u;

  pair_v4i acc[kPairSuper][kPairSuper];
#pragma unroll
  for (int a = 0; a < kPairSuper; ++a)
#pragma unroll
    for (int b = 0; b < kPairSuper; ++b) acc[a][b] = pair_v4i{0, 0, 0, 0};
  uint32_t bad = 0;

  // The raw words of step r + 1 are loaded before step r's are turned into fragments, so a wave's loads
  // are in flight under its own VALU and MFMA work (two waves per SIMD hide little by themselves).
  const int64_t stride = (int64_t)kPairStep * kPairWaves;
  uint4 wa[kPairSuper], wb[kPairSuper], ws;
  auto load_step = [&](int64_t r, uint4(&qa)[kPairSuper], uint4(&qb)[kPairSuper], uint4 &qs) {
    const int64_t rl = r + 16 * (lane >> 4);
    const int64_t nv = r_end - rl;  // rows of the lane's 16 that are inside the slice (may be <= 0)
    qs = ps ? pair_load16(ps + rl, nv, vec) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int t = 0; t < kPairSuper; ++t) {
      qb[t] = pair_load16(pb[t] + rl, on_b[t] ? nv : 0, vec);
      qa[t] = pair_load16(pa[t] + rl, on_a[t] ? nv : 0, vec);
    }
  };
  int64_t r = r_begin + (int64_t)wave * kPairStep;
  if (r < r_end) load_step(r, wa, wb, ws);
  for (; r < r_end; r += stride) {
    uint4 na[kPairSuper], nb[kPairSuper], ns;
    load_step(r + stride, na, nb, ns);  // past the slice's end: nothing is read, every byte is 255
    uint4 sm = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
    if (ps)
      sm = make_uint4(pair_eq_bytes(ws.x, crep), pair_eq_bytes(ws.y, crep), pair_eq_bytes(ws.z, crep),
                      pair_eq_bytes(ws.w, crep));
    pair_v4i fb[kPairSuper];
#pragma unroll
    for (int t = 0; t < kPairSuper; ++t) {
      const uint4 w = wb[t];
      if (check_b)
        bad |= pair_bad_bytes(w.x, c7b[t], chb[t]) | pair_bad_bytes(w.y, c7b[t], chb[t]) |
               pair_bad_bytes(w.z, c7b[t], chb[t]) | pair_bad_bytes(w.w, c7b[t], chb[t]);
      fb[t] = pair_v4i{(int)pair_eq_bytes(w.x, kb[t]), (int)pair_eq_bytes(w.y, kb[t]), (int)pair_eq_bytes(w.z, kb[t]),
                       (int)pair_eq_bytes(w.w, kb[t])};
    }
#pragma unroll
    for (int a = 0; a < kPairSuper; ++a) {
      const uint4 w = wa[a];
      if (check_a)
        bad |= pair_bad_bytes(w.x, c7a[a], cha[a]) | pair_bad_bytes(w.y, c7a[a], cha[a]) |
               pair_bad_bytes(w.z, c7a[a], cha[a]) | pair_bad_bytes(w.w, c7a[a], cha[a]);
      const pair_v4i fa = pair_v4i{(int)(pair_eq_bytes(w.x, ka[a]) & sm.x), (int)(pair_eq_bytes(w.y, ka[a]) & sm.y),
                                   (int)(pair_eq_bytes(w.z, ka[a]) & sm.z), (int)(pair_eq_bytes(w.w, ka[a]) & sm.w)};
#pragma unroll
      for (int b = 0; b < kPairSuper; ++b)
        if (!diag || a <= b) acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, fb[b], acc[a][b], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < kPairSuper; ++t) {
      wa[t] = na[t];
      wb[t] = nb[t];
    }
    ws = ns;
  }
  if (bad & 0x80808080u) atomicOr(err, 1);

  // only the non-zero accumulators of tiles inside the table, upper triangle of tiles only
  const int64_t n_tiles = Sp / kPairTile;
  unsigned long long *out = counts + (int64_t)blockIdx.z * Sp * Sp;
#pragma unroll
  for (int a = 0; a < kPairSuper; ++a)
#pragma unroll
    for (int b = 0; b < kPairSuper; ++b) {
      const int64_t ti = (int64_t)g.I * kPairSuper + a, tj = (int64_t)g.J * kPairSuper + b;
      if (ti >= n_tiles || tj >= n_tiles || ti > tj) continue;
      const int64_t col = tj * kPairTile + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int v = acc[a][b][reg];
        const int64_t row = ti * kPairTile + 4 * (lane >> 4) + reg;
        if (v != 0) atomicAdd(&out[row * Sp + col], (unsigned long long)(uint32_t)v);
      }
    }
}

// ---------------------------------------------------------------------------- pair statistics
// One workgroup of kPairStatBlock work-items per (stratum, pair u < v).  Integer work first (the block's
// own row sums a, column sums b and N: exact in any order), then fp64 sums whose order is fixed by the
// block's shape alone: work-item t adds the cells t, t + kPairStatBlock, ... of the block in row-major
// order, then a fixed-shape tree over the work-items.  No floating-point atomics: a pair's numbers do not
// depend on what else is in the launch.
__device__ inline double pair_tree(double *red, double v, uint32_t tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (uint32_t s = kPairStatBlock / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// the marginals of the block into LDS; returns N
__device__ inline int64_t pair_marginals(const int64_t *__restrict__ base, int64_t Sp, int32_t ru, int32_t rv,
                                         int64_t *ra, int64_t *cb, uint32_t tid) {
  for (int32_t i = (int32_t)tid; i < ru; i += kPairStatBlock) {
    int64_t s = 0;
    for (int32_t j = 0; j < rv; ++j) s += base[(int64_t)i * Sp + j];
    ra[i] = s;
  }
  for (int32_t j = (int32_t)tid; j < rv; j += kPairStatBlock) {
    int64_t s = 0;
    for (int32_t i = 0; i < ru; ++i) s += base[(int64_t)i * Sp + j];
    cb[j] = s;
  }
  __syncthreads();
  int64_t N = 0;
  for (int32_t i = 0; i < ru; ++i) N += ra[i];
  return N;
}

__global__ __launch_bounds__(kPairStatBlock) void k_pair_mi(const PairVars *__restrict__ pairs,
                                                            const int64_t *__restrict__ counts, int64_t Sp,
                                                            double *__restrict__ mi, double *__restrict__ hu,
                                                            double *__restrict__ hv, int64_t *__restrict__ n_out) {
  __shared__ int64_t ra[kPairMaxCard], cb[kPairMaxCard];
  __shared__ double la[kPairMaxCard], lb[kPairMaxCard];
  __shared__ double red[kPairStatBlock];
  const uint32_t tid = threadIdx.x;
  const PairVars P = pairs[blockIdx.x];
  const int64_t o = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t *base = counts + (int64_t)blockIdx.y * Sp * Sp + (int64_t)P.off_u * Sp + P.off_v;
  const int32_t ru = P.card_u, rv = P.card_v;
  const int64_t N = pair_marginals(base, Sp, ru, rv, ra, cb, tid);
  if (N == 0) {
    if (tid == 0) {
      mi[o] = 0.0;
      hu[o] = 0.0;
      hv[o] = 0.0;
      n_out[o] = 0;
    }
    return;
  }
  const double dN = (double)N, logN = log(dN);
  for (int32_t i = (int32_t)tid; i < ru; i += kPairStatBlock) la[i] = ra[i] > 0 ? log((double)ra[i]) : 0.0;
  for (int32_t j = (int32_t)tid; j < rv; j += kPairStatBlock) lb[j] = cb[j] > 0 ? log((double)cb[j]) : 0.0;
  __syncthreads();
  double s = 0.0;
  for (int32_t cell = (int32_t)tid; cell < ru * rv; cell += kPairStatBlock) {
    const int32_t i = cell / rv, j = cell - i * rv;
    const int64_t n = base[(int64_t)i * Sp + j];
    if (n > 0) s += ((double)n / dN) * (((log((double)n) + logN) - la[i]) - lb[j]);
  }
  const double tmi = pair_tree(red, s, tid);
  s = 0.0;
  for (int32_t i = (int32_t)tid; i < ru; i += kPairStatBlock)
    if (ra[i] > 0) s += ((double)ra[i] / dN) * (logN - la[i]);
  const double thu = pair_tree(red, s, tid);
  s = 0.0;
  for (int32_t j = (int32_t)tid; j < rv; j += kPairStatBlock)
    if (cb[j] > 0) s += ((double)cb[j] / dN) * (logN - lb[j]);
  const double thv = pair_tree(red, s, tid);
  if (tid == 0) {
    mi[o] = tmi > 0.0 ? tmi : 0.0;
    hu[o] = thu;
    hv[o] = thv;
    n_out[o] = N;
  }
}

// The expected mutual information of the block's marginals under the hypergeometric model
// (scikit-learn's expected_mutual_information): the sum over the states i of u, j of v and
// n = max(1, a_i + b_j - N) .. min(a_i, b_j) of
//   (n / N) (log N + log n - log a_i - log b_j)
//   exp(lgamma(a_i + 1) + lgamma(b_j + 1) + lgamma(N - a_i + 1) + lgamma(N - b_j + 1) - lgamma(N + 1)
//       - lgamma(n + 1) - lgamma(a_i - n + 1) - lgamma(b_j - n + 1) - lgamma(N - a_i - b_j + n + 1)).
// The cells are walked in row-major order by the whole workgroup; work-item t takes n = start + t,
// start + t + kPairStatBlock, ... of each, then the fixed-shape tree.
__global__ __launch_bounds__(kPairStatBlock) void k_pair_emi(const PairVars *__restrict__ pairs,
                                                             const int64_t *__restrict__ counts, int64_t Sp,
                                                             double *__restrict__ emi) {
  __shared__ int64_t ra[kPairMaxCard], cb[kPairMaxCard];
  __shared__ double la[kPairMaxCard], lb[kPairMaxCard], ga[kPairMaxCard], gb[kPairMaxCard];
  __shared__ double red[kPairStatBlock];
  const uint32_t tid = threadIdx.x;
  const PairVars P = pairs[blockIdx.x];
  const int64_t o = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t *base = counts + (int64_t)blockIdx.y * Sp * Sp + (int64_t)P.off_u * Sp + P.off_v;
  const int32_t ru = P.card_u, rv = P.card_v;
  const int64_t N = pair_marginals(base, Sp, ru, rv, ra, cb, tid);
  if (N == 0) {
    if (tid == 0) emi[o] = 0.0;
    return;
  }
  const double dN = (double)N, logN = log(dN), gN = lgamma(dN + 1.0);
  for (int32_t i = (int32_t)tid; i < ru; i += kPairStatBlock) {
    const double a = (double)ra[i];
    la[i] = ra[i] > 0 ? log(a) : 0.0;
    ga[i] = lgamma(a + 1.0) + lgamma(dN - a + 1.0);
  }
  for (int32_t j = (int32_t)tid; j < rv; j += kPairStatBlock) {
    const double b = (double)cb[j];
    lb[j] = cb[j] > 0 ? log(b) : 0.0;
    gb[j] = lgamma(b + 1.0) + lgamma(dN - b + 1.0);
  }
  __syncthreads();
  double s = 0.0;
  for (int32_t i = 0; i < ru; ++i) {
    const int64_t a = ra[i];
    if (a == 0) continue;
    for (int32_t j = 0; j < rv; ++j) {
      const int64_t b = cb[j];
      if (b == 0) continue;
      const int64_t start = a + b - N > 1 ? a + b - N : 1, end = a < b ? a : b;
      const double g0 = (ga[i] + gb[j]) - gN, l0 = (logN - la[i]) - lb[j];
      for (int64_t n = start + tid; n <= end; n += kPairStatBlock) {
        const double dn = (double)n;
        const double gln = (((g0 - lgamma(dn + 1.0)) - lgamma((double)(a - n) + 1.0)) - lgamma((double)(b - n) + 1.0)) -
                           lgamma((double)(N - a - b + n) + 1.0);
        s += (dn / dN) * (l0 + log(dn)) * exp(gln);
      }
    }
  }
  const double t = pair_tree(red, s, tid);
  if (tid == 0) emi[o] = t;
}

// ---------------------------------------------------------------------------- the handle's device side
static int pair_use(PairHandle *h) {
  using pgmdev::upload;
  const PairPlan &p = h->p;
  const pgmdev::Slot base[] = {upload(h->d_states, p.states), upload(h->d_groups, p.groups), upload(h->d_pairs, p.pairs)};
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_pair_plan_destroy(void *plan) { return pgm_plan_destroy<PairHandle>(plan); }

int pgm_pair_count(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                   int32_t strat_col, int32_t n_strata, int64_t *counts, void *stream) {
  PairHandle *h = static_cast<PairHandle *>(plan);
  int64_t slice = 0, n_slices = 0;
  const int st = pair_count_check(h, codes, n_cols, ld, row0, n_rows, strat_col, n_strata, counts, &slice, &n_slices);
  if (st != PGM_OK) return st;
  if (n_slices == 0) return PGM_OK;
  int up = pair_use(h);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  const dim3 grid((unsigned)h->p.groups.size(), (unsigned)n_slices, (unsigned)n_strata), wg(kPairBlock);
  hipLaunchKernelGGL(k_pair_count, grid, wg, 0, S(stream), h->d_states, h->d_groups, codes, ld, row0, n_rows, slice,
                     strat_col, pair_codes_vec16(codes, ld, row0) ? 1 : 0, reinterpret_cast<unsigned long long *>(counts),
                     h->p.Sp, h->dev.flag());
  // PGM_EINDEX is this call's status: the flag is read back after the launch (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad) return pgmi_fail(PGM_EINDEX, "pair_count: a state code is >= its variable's cardinality");
  return PGM_OK;
}

int pgm_pair_mi(void *plan, const int64_t *counts, int32_t n_strata, double *mi, double *hu, double *hv, int64_t *n,
                void *stream) {
  PairHandle *h = static_cast<PairHandle *>(plan);
  const void *outs[] = {mi, hu, hv, n};
  const int st = pair_stat_check("pair_mi", h, counts, n_strata, outs, 4);
  if (st != PGM_OK) return st;
  if (h->p.pairs.empty()) return PGM_OK;
  const int up = pair_use(h);
  if (up != PGM_OK) return up;
  const dim3 grid((unsigned)h->p.pairs.size(), (unsigned)n_strata), wg(kPairStatBlock);
  hipLaunchKernelGGL(k_pair_mi, grid, wg, 0, S(stream), h->d_pairs, counts, h->p.Sp, mi, hu, hv, n);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_pair_emi(void *plan, const int64_t *counts, int32_t n_strata, double *emi, void *stream) {
  PairHandle *h = static_cast<PairHandle *>(plan);
  const void *outs[] = {emi};
  const int st = pair_stat_check("pair_emi", h, counts, n_strata, outs, 1);
  if (st != PGM_OK) return st;
  if (h->p.pairs.empty()) return PGM_OK;
  const int up = pair_use(h);
  if (up != PGM_OK) return up;
  const dim3 grid((unsigned)h->p.pairs.size(), (unsigned)n_strata), wg(kPairStatBlock);
  hipLaunchKernelGGL(k_pair_emi, grid, wg, 0, S(stream), h->d_pairs, counts, h->p.Sp, emi);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

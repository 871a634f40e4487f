// pgmdbn_pf.hip — the bootstrap particle filter for dynamic networks on the device (gfx950): the running-sum
// kernel, the fused draw / weight / histogram / resample kernel and the trajectory trace behind
// DBNInference.particle_filter_codes / posterior_sample_codes and ApproxInference on a DynamicBayesianNetwork, and
// their C-ABI (pgm_dbn_pf_plan_destroy, pgm_dbn_pf_run, pgm_dbn_pf_trace).  The contract is include/pgmhip.h
// "dynamic Bayesian networks: the particle filter"; the host side (validation, plan order, LDS geometry, argument
// checks, pgm_dbn_pf_plan_info) is pgmdbn_pf_plan.cpp.  fp64 and integers only.
#include "pgm_hip_common.h"
#include "pgm_dbn_pf.h"
#include "pgm_sample.h"

typedef unsigned long long u64;

// ---------------------------------------------------------------------------- running sums
// One work-item per CPD column of one set (the family is found by bisection over col_off, as k_sample_cdf does):
// c_0 = p_0, c_s = c_{s-1} + p_s, strictly in state order.  A column whose total is not finite or not > 0 cannot
// be drawn from: bit 2 of *err is raised.
__global__ __launch_bounds__(256) void k_dbn_pf_cdf(const PfFam *__restrict__ fams, const int64_t *__restrict__ col_off,
                                                    int32_t n_fam, const double *__restrict__ values,
                                                    double *__restrict__ cdf, int32_t *__restrict__ err) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= col_off[n_fam]) return;
  int32_t lo = 0, hi = n_fam;  // col_off[lo] <= c < col_off[hi]
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (col_off[mid] <= c) lo = mid;
    else hi = mid;
  }
  const PfFam &F = fams[lo];
  const int64_t ncol = F.ncol, at = (int64_t)F.off + (c - col_off[lo]);
  double sum = 0.0;
  for (int32_t s = 0; s < F.card; ++s) {
    sum += values[at + s * ncol];
    cdf[at + s * ncol] = sum;
  }
  if (!(sum > 0.0) || !(sum <= 1.79769313486231570815e308)) atomicOr(err, 2);
}

// ---------------------------------------------------------------------------- the filter
struct PfArgs {
  const PfFam *fams;     // [2 n]: the slice-0 set in plan order, then the transition set
  const int32_t *tab;    // card, iface, qnode, qoff at the offsets below
  int32_t o_card, o_iface, o_qnode, o_qoff;
  int32_t n, n_iface, n_q, bins, N, T;
  const uint8_t *codes;
  int64_t ld, row0;
  const double *val0, *val1, *cdf0, *cdf1;
  uint64_t first_row, seed;
  double *filter, *loglik, *ess;
  uint8_t *flags;
  uint16_t *anc;
  uint8_t *traj;
  int32_t *err;
};

// what a sequence that is not (or no longer) run gets at slice t: NaN marginals and ess, identity ancestors, and
// PGM_EV_MISSING trajectories unless the slice's drawn codes were written already
__device__ __forceinline__ void pf_blank_slice(const PfArgs &a, double *filter, double *ess, uint16_t *anc, uint8_t *traj,
                                               int32_t t, bool blank_traj) {
  const uint32_t tid = threadIdx.x, block = blockDim.x, N = (uint32_t)a.N;
  if (filter)
    for (uint32_t s = tid; s < (uint32_t)a.bins; s += block) filter[(int64_t)t * a.bins + s] = (double)NAN;
  if (ess && tid == 0) ess[t] = (double)NAN;
  if (anc)
    for (uint32_t j = tid; j < N; j += block) anc[(int64_t)t * N + j] = (uint16_t)j;
  if (traj && blank_traj)
    for (int64_t i = tid; i < (int64_t)a.n_q * N; i += block) traj[(int64_t)t * a.n_q * N + i] = PGM_EV_MISSING;
}

// Workgroup b runs sequence b of the call through every slice with N particles in LDS; work-item l owns particles
// l, l + block, ... (so a wave's bytes of a tile row are consecutive: conflict-free read-back, as in pgmlw.hip),
// except in the scan, where it owns the N / block consecutive entries from l N / block.  SINGLE: N = 64, the
// workgroup is one wave and no reduction or scan crosses waves.  Dynamic LDS as pf_lds_bytes lays it out.
template <bool SINGLE>
__global__ __launch_bounds__(kPfMaxBlock) void k_dbn_pf(PfArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t tid = threadIdx.x, block = blockDim.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t N = (uint32_t)a.N;
  const int32_t n = a.n, T = a.T, n_q = a.n_q, bins = a.bins;
  const size_t tile_bytes = ((size_t)(n + a.n_iface) * N + 7) / 8 * 8;
  uint8_t *tile = reinterpret_cast<uint8_t *>(smem);           // [n + n_iface][N]
  u64 *qs = reinterpret_cast<u64 *>(smem + tile_bytes);        // [N]: w, then q, then the inclusive scan of q
  double *wbuf = reinterpret_cast<double *>(qs);
  u64 *hist = qs + N;                                          // [bins]
  char *pad = reinterpret_cast<char *>(hist + bins);
  double *wave_max = reinterpret_cast<double *>(pad);          // [4]
  u64 *wave_tot = reinterpret_cast<u64 *>(pad + 32);           // [4]
  u64 *rsum = reinterpret_cast<u64 *>(pad + 64);               // S1, S2
  uint8_t *ev = reinterpret_cast<uint8_t *>(pad + kPfPadBytes);  // [n]
  const int32_t *card = a.tab + a.o_card, *iface = a.tab + a.o_iface, *qnode = a.tab + a.o_qnode, *qoff = a.tab + a.o_qoff;

  const int64_t b = blockIdx.x, row = a.row0 + b;
  double *filter = a.filter ? a.filter + b * T * bins : nullptr;
  double *ess = a.ess ? a.ess + b * T : nullptr;
  uint16_t *anc = a.anc ? a.anc + b * T * N : nullptr;
  uint8_t *traj = a.traj ? a.traj + b * T * n_q * N : nullptr;

  // a bad cell anywhere: the sequence is not run
  int bad = 0;
  for (int32_t c = (int32_t)tid; c < T * n; c += (int32_t)block) {
    const uint32_t g = a.codes[(int64_t)c * a.ld + row];
    if (g != PGM_EV_MISSING && g >= (uint32_t)card[c % n]) bad = 1;
  }
  if (__syncthreads_or(bad)) {
    for (int32_t t = 0; t < T; ++t) pf_blank_slice(a, filter, ess, anc, traj, t, true);
    if (tid == 0) {
      if (a.loglik) a.loglik[b] = (double)NAN;
      if (a.flags) a.flags[b] = PGM_DBN_PF_BAD;
      atomicOr(a.err, 1);
    }
    return;
  }

  const uint64_t srow0 = a.first_row + (uint64_t)b * N, seed = a.seed;
  const uint32_t ppl = N / block;
  double ll = 0.0;
  bool dead = false;
  for (int32_t t = 0; t < T; ++t) {
    if (dead) {  // workgroup-uniform
      pf_blank_slice(a, filter, ess, anc, traj, t, true);
      continue;
    }
    for (int32_t c = (int32_t)tid; c < n; c += (int32_t)block) ev[c] = a.codes[((int64_t)t * n + c) * a.ld + row];
    for (int32_t s = (int32_t)tid; s < bins; s += (int32_t)block) hist[s] = 0;
    if (tid < 2) rsum[tid] = 0;
    __syncthreads();

    // 1. propagate: every node in plan order; parents from the tile, tables through the caches, Philox in registers
    const PfFam *fams = a.fams + (t ? n : 0);
    const double *val = t ? a.val1 : a.val0, *cdf = t ? a.cdf1 : a.cdf0;
    double m = 0.0;
    for (uint32_t p = tid; p < N; p += block) {
      double w = 1.0;
      for (int32_t f = 0; f < n; ++f) {
        const PfFam &F = fams[f];  // workgroup-uniform: scalar loads
        int32_t col = 0;
        for (int32_t j = 0; j < F.n_par; ++j) col += (int32_t)tile[(uint32_t)F.src[j] * N + p] * F.stride[j];
        const int64_t at = (int64_t)F.off + col;
        const uint32_t g = ev[F.node];
        uint32_t s;
        if (g == PGM_EV_MISSING) {
          s = (uint32_t)sample_select(cdf + at, F.card, F.ncol, sample_uniform(seed, srow0 + p, (uint32_t)(t * n + F.node)));
        } else {
          s = g;
          w *= val[at + (int64_t)s * F.ncol] / cdf[at + (int64_t)(F.card - 1) * F.ncol];  // no addition: nothing to contract
        }
        tile[(uint32_t)F.node * N + p] = (uint8_t)s;
      }
      wbuf[p] = w;
      if (w > m) m = w;
      if (traj)
        for (int32_t k = 0; k < n_q; ++k) traj[((int64_t)t * n_q + k) * N + p] = tile[(uint32_t)qnode[k] * N + p];
    }

    // 2. the largest weight of the sequence
    for (int d = 32; d > 0; d >>= 1) {
      const double o = __shfl_xor(m, d);
      if (o > m) m = o;
    }
    if constexpr (!SINGLE) {
      if (lane == 0) wave_max[wave] = m;
      __syncthreads();
      m = wave_max[0];
      for (uint32_t w = 1; w < block / 64; ++w)
        if (wave_max[w] > m) m = wave_max[w];
    }
    const double wmax = m;
    if (!(wmax > 0.0)) {  // impossible from this slice on
      pf_blank_slice(a, filter, ess, anc, traj, t, false);
      ll = -INFINITY;
      dead = true;
      continue;
    }

    // 3. quantise; the histogram of the queried nodes and the two sums of the effective sample size
    u64 s1 = 0, s2 = 0;
    for (uint32_t p = tid; p < N; p += block) {
      const u64 q = (u64)ldexp(wbuf[p] / wmax, kPfQuantBits);  // truncated
      qs[p] = q;
      if (q == 0) continue;
      const u64 q1 = q >> kPfEssShift;
      s1 += q1, s2 += q1 * q1;
      for (int32_t k = 0; k < n_q; ++k) atomicAdd(&hist[qoff[k] + (int32_t)tile[(uint32_t)qnode[k] * N + p]], q);
    }
    atomicAdd(&rsum[0], s1);
    atomicAdd(&rsum[1], s2);
    __syncthreads();

    // 4. inclusive scan of q: a lane's consecutive entries, a wave scan with cross-lane moves, the waves through LDS
    const uint32_t seg = tid * ppl;
    u64 tot = 0;
    for (uint32_t j = 0; j < ppl; ++j) tot += qs[seg + j];
    u64 inc = tot;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const u64 o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    u64 run = inc - tot;
    if constexpr (!SINGLE) {
      if (lane == 63) wave_tot[wave] = inc;
      __syncthreads();
      for (uint32_t w = 0; w < wave; ++w) run += wave_tot[w];
    }
    for (uint32_t j = 0; j < ppl; ++j) {
      run += qs[seg + j];
      qs[seg + j] = run;
    }
    __syncthreads();
    const u64 Q = qs[N - 1];

    // 5. systematic resampling in integers; 6. the gather of the ancestor's interface codes is the slice advance
    uint32_t x[4];
    philox4x32_10((uint32_t)srow0, (uint32_t)(srow0 >> 32), (uint32_t)t, PGM_DBN_PF_RESAMPLE, (uint32_t)seed,
                  (uint32_t)(seed >> 32), x);
    const u64 r = __umul64hi((((u64)x[0] << 21) | (x[1] >> 11)) << 11, Q);
    for (uint32_t j = tid; j < N; j += block) {
      const u64 thr = (u64)j * Q + r;
      uint32_t lo = 0, hi = N - 1;  // the first i with N C_i > thr; i = N - 1 always has it
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((u64)N * qs[mid] > thr) hi = mid;
        else lo = mid + 1;
      }
      if (anc) anc[(int64_t)t * N + j] = (uint16_t)lo;
      for (int32_t i = 0; i < a.n_iface; ++i) tile[(uint32_t)(n + i) * N + j] = tile[(uint32_t)iface[i] * N + lo];
    }

    // 7. the slice's outputs
    if (filter)
      for (int32_t s = (int32_t)tid; s < bins; s += (int32_t)block) filter[(int64_t)t * bins + s] = (double)hist[s] / (double)Q;
    if (tid == 0) {
      if (ess) ess[t] = (double)rsum[0] * (double)rsum[0] / (double)rsum[1];
      ll += log(wmax) + log((double)Q * 0x1.0p-36 / (double)N);
    }
    __syncthreads();  // the next slice draws over the codes the gather has read
  }
  if (tid == 0) {
    if (a.loglik) a.loglik[b] = ll;
    if (a.flags) a.flags[b] = dead ? PGM_DBN_PF_IMPOSSIBLE : 0;
  }
}

// ---------------------------------------------------------------------------- the trace
// One work-item per final particle g = b N + j: i_{T-1} = a_{T-1}[j], i_{t-1} = a_{t-1}[i_t]; the queried nodes'
// codes of particle i_t at slice t go to column t n_q + k, row row0_out + g.  An index is masked to N - 1, so
// no content of `anc` reads outside the buffers.
__global__ __launch_bounds__(256) void k_dbn_pf_trace(const uint16_t *__restrict__ anc, const uint8_t *__restrict__ traj,
                                                      int64_t total, int32_t T, int32_t N, int32_t n_q,
                                                      uint8_t *__restrict__ out, int64_t ld_out, int64_t row0_out) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const int64_t b = g / N;
  uint32_t i = (uint32_t)(g % N);
  for (int32_t t = T - 1; t >= 0; --t) {
    i = anc[(b * T + t) * N + i] & (uint32_t)(N - 1);
    for (int32_t k = 0; k < n_q; ++k)
      out[((int64_t)t * n_q + k) * ld_out + row0_out + g] = traj[((b * T + t) * n_q + k) * N + i];
  }
}

// ---------------------------------------------------------------------------- the handle's device side
static int pf_use(PfHandle *h) {
  const PfPlan &p = h->p;
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_fams, p.fams), pgmdev::upload(h->d_col_off, p.col_off),
                               pgmdev::upload(h->d_tab, p.tab), pgmdev::scratch(h->d_cdf0, (size_t)p.total[0]),
                               pgmdev::scratch(h->d_cdf1, (size_t)p.total[1])};
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_dbn_pf_plan_destroy(void *plan) { return pgm_plan_destroy<PfHandle>(plan); }

int pgm_dbn_pf_run(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                   int32_t n_slices, const double *values0, const double *values1, int32_t n_particles, int64_t first_row,
                   uint64_t seed, double *filter, double *loglik, double *ess, uint8_t *flags, uint16_t *ancestors,
                   uint8_t *traj, void *stream) {
  PfHandle *h = static_cast<PfHandle *>(plan);
  bool launch = false;
  const int st = pf_run_check(h, codes, n_cols, ld, row0, n_rows, n_slices, values0, values1, n_particles, first_row, filter,
                              loglik, ess, ancestors, traj, &launch);
  if (st != PGM_OK || !launch) return st;
  const PfPlan &p = h->p;
  int up = pf_use(h);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  const double *values[2] = {values0, values1};
  double *cdf[2] = {h->d_cdf0, h->d_cdf1};
  for (int k = 0; k < 2; ++k) {
    const int64_t blocks = (p.col_off[(size_t)k * (p.n + 1) + p.n] + 255) / 256;
    hipLaunchKernelGGL(k_dbn_pf_cdf, dim3((unsigned)blocks), dim3(256), 0, S(stream), h->d_fams + (size_t)k * p.n,
                       h->d_col_off + (size_t)k * (p.n + 1), p.n, values[k], cdf[k], h->dev.flag());
    HIP_TRY(hipGetLastError());
  }
  const int64_t lds = pf_lds_bytes(p.n, p.n_iface, p.bins, n_particles);
  const bool single = n_particles == 64;
  const void *kernel = single ? reinterpret_cast<const void *>(&k_dbn_pf<true>) : reinterpret_cast<const void *>(&k_dbn_pf<false>);
  // above 64 KiB of dynamic LDS a kernel has to be told so before the launch
  if (lds > 65536) HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  PfArgs a = {};
  a.fams = h->d_fams, a.tab = h->d_tab;
  a.o_card = p.o_card, a.o_iface = p.o_iface, a.o_qnode = p.o_qnode, a.o_qoff = p.o_qoff;
  a.n = p.n, a.n_iface = p.n_iface, a.n_q = p.n_qnodes, a.bins = p.bins, a.N = n_particles, a.T = n_slices;
  a.codes = codes, a.ld = ld, a.row0 = row0;
  a.val0 = values0, a.val1 = values1, a.cdf0 = h->d_cdf0, a.cdf1 = h->d_cdf1;
  a.first_row = (uint64_t)first_row, a.seed = seed;
  a.filter = filter, a.loglik = loglik, a.ess = ess, a.flags = flags, a.anc = ancestors, a.traj = traj;
  a.err = h->dev.flag();
  const dim3 grid((unsigned)n_rows), wg((unsigned)(n_particles < kPfMaxBlock ? n_particles : kPfMaxBlock));
  if (single) hipLaunchKernelGGL(k_dbn_pf<true>, grid, wg, (size_t)lds, S(stream), a);
  else hipLaunchKernelGGL(k_dbn_pf<false>, grid, wg, (size_t)lds, S(stream), a);
  // PGM_EINDEX / PGM_EINVAL is this call's status: the flag is read back after the launches (synchronises the stream)
  int32_t bits = 0;
  const int rd = flag_read(h->dev, stream, &bits);
  if (rd != PGM_OK) return rd;
  if (bits & 2) return pgmi_fail(PGM_EINVAL, "dbn_pf_run: a CPD column's total is not finite or not > 0");
  if (bits & 1) return pgmi_fail(PGM_EINDEX, "dbn_pf_run: an evidence code is >= its node's cardinality");
  return PGM_OK;
}

int pgm_dbn_pf_trace(void *plan, const uint16_t *ancestors, const uint8_t *traj, int64_t n_rows, int32_t n_slices,
                     int32_t n_particles, uint8_t *out, int64_t ld_out, int64_t row0_out, void *stream) {
  PfHandle *h = static_cast<PfHandle *>(plan);
  bool launch = false;
  const int st = pf_trace_check(h, ancestors, traj, n_rows, n_slices, n_particles, out, ld_out, row0_out, &launch);
  if (st != PGM_OK || !launch) return st;
  const int64_t total = n_rows * n_particles;
  hipLaunchKernelGGL(k_dbn_pf_trace, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(stream), ancestors, traj, total,
                     n_slices, n_particles, h->p.n_qnodes, out, ld_out, row0_out);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}
}

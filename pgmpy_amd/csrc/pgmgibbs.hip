// pgmgibbs.hip — Gibbs sampling on the device (gfx950): the fused sweep kernel behind
// pgmpy_amd.sampling.GibbsSampling and its C-ABI (pgm_gibbs_plan_destroy, pgm_gibbs_start,
// pgm_gibbs_sweep).  Replaces the reference's transition table over every joint configuration of the other
// variables and its one-chain Python walk (sampling/Sampling.py:409-631): the conditional of a variable is
// the product of the few factors that contain it, read at the chain's current codes, and one lane owns one
// chain.  The host side (validation, incidence lists, argument checks, host-only queries) is
// pgmgibbs_plan.cpp.
#include <cstring>

#include "pgm_gibbs.h"
#include "pgm_hip_common.h"

// Every product and sum of a conditional is a separately rounded fp64 operation (__dmul_rn / __dadd_rn;
// the pragma covers what is left): hipcc would contract c + w * v into an FMA, and the draw would differ
// from a plain restatement where t = u * total lands on a running sum.
#pragma clang fp contract(off)

// what a launch reads, passed by value (workgroup-uniform: scalar loads from the kernarg segment)
struct GibbsArgs {
  const int32_t *card, *inc_off;
  const GibbsInc *inc;
  const GibbsOther *others;
  const double *values;
  uint8_t *codes;  // ONE pointer, read and written (see k_gibbs_sweep)
  const uint8_t *clamp;
  uint8_t *trace;
  const double *uniforms;
  int32_t *err;
  int64_t ld, row0, n_chains, first_chain, first_sweep, n_sweeps, ld_trace, thin;
  uint64_t seed;
  int32_t n_cols;       // columns of the plan
  int32_t n_cols_codes;  // columns of codes (the layout of uniforms)
};

static constexpr int32_t kGibbsErrTotal = 1, kGibbsErrCode = 2;

// the table index of a factor at the chain's current codes of its other columns
__device__ __forceinline__ int32_t gibbs_base(const GibbsInc &I, const GibbsOther *__restrict__ others, const uint8_t *st,
                                              int64_t sld) {
  int32_t base = 0;
  for (int32_t o = I.other_begin; o < I.other_end; ++o) base += (int32_t)st[(int64_t)others[o].col * sld] * others[o].stride;
  return base;
}

// One launch advances n_chains chains through n_sweeps sweeps: workgroup b owns chains [b, b + 1) *
// kGibbsBlock, one per lane; a lane walks the columns in ascending order and never reads another lane's
// state, so there is no barrier.
// LDS: the workgroup's codes live in LDS as [column][lane] bytes for the whole launch (loaded once, written
// back once); else the state stays in the code matrix.  There `codes` is ONE pointer, read and written,
// without __restrict__: a lane reads back the codes it stored itself, and a const __restrict__ input next
// to a __restrict__ output would let the compiler move that read above the store (as in k_sample_forward).
// U: uniforms from the caller's [n_sweeps, n_cols, ld] matrix, not Philox.
// A chain that holds a code >= its column's cardinality is not advanced (nothing is indexed with it).
template <bool LDS, bool U>
__global__ __launch_bounds__(kGibbsBlock) void k_gibbs_sweep(const GibbsArgs a) {
  extern __shared__ __align__(16) uint8_t gibbs_lds[];
  const int64_t r = (int64_t)blockIdx.x * kGibbsBlock + threadIdx.x;
  if (r >= a.n_chains) return;
  uint8_t *g = a.codes + a.row0 + r;  // this chain's code of column 0
  uint8_t *st = LDS ? gibbs_lds + threadIdx.x : g;
  const int64_t sld = LDS ? (int64_t)kGibbsBlock : a.ld;
  bool bad = false;
  for (int32_t c = 0; c < a.n_cols; ++c) {
    const uint32_t q = g[(int64_t)c * a.ld];
    bad |= q >= (uint32_t)a.card[c];
    if constexpr (LDS) st[(int64_t)c * sld] = (uint8_t)q;
  }
  if (bad) {
    atomicOr(a.err, kGibbsErrCode);
    return;
  }
  const uint64_t chain = (uint64_t)(a.first_chain + r);
  bool undrawn = false;
  for (int64_t j = 1; j <= a.n_sweeps; ++j) {
    const uint32_t sweep = (uint32_t)(a.first_sweep + j - 1);
    for (int32_t c = 0; c < a.n_cols; ++c) {
      if (a.clamp && a.clamp[c]) continue;
      const int32_t K = a.card[c], e0 = a.inc_off[c], e1 = a.inc_off[c + 1];
      double u;
      if constexpr (U) u = a.uniforms[((j - 1) * a.n_cols_codes + c) * a.ld + a.row0 + r];
      else u = sample_uniform3(a.seed, chain, (uint32_t)c, sweep);
      int32_t k;
      double total;
      if (K <= kGibbsRegCard) {
        // the K weights in registers, one factor at a time; then their running sums in place
        double w[kGibbsRegCard];
        for (int32_t e = e0; e < e1; ++e) {
          const GibbsInc &I = a.inc[e];
          const double *p = a.values + I.off + gibbs_base(I, a.others, st, sld);
#pragma unroll
          for (int s = 0; s < kGibbsRegCard; ++s)
            if (s < K) {
              const double v = p[(int64_t)s * I.stride];
              w[s] = e == e0 ? v : __dmul_rn(w[s], v);
            }
        }
        total = w[0];
#pragma unroll
        for (int s = 1; s < kGibbsRegCard; ++s)
          if (s < K) w[s] = total = __dadd_rn(total, w[s]);
        const double t = __dmul_rn(u, total);
        k = K;
#pragma unroll
        for (int s = kGibbsRegCard - 1; s >= 0; --s)
          if (s < K && w[s] > t) k = s;
        if (k == K) {  // u * total rounded up to the total: the first state that reaches it
#pragma unroll
          for (int s = kGibbsRegCard - 1; s >= 0; --s)
            if (s < K && w[s] == total) k = s;
        }
      } else {
        // weight s again whenever it is needed: the same factors in the same order, so the same bits
        auto weight = [&](int32_t s) {
          double w = 0.0;
          for (int32_t e = e0; e < e1; ++e) {
            const GibbsInc &I = a.inc[e];
            const double v = a.values[I.off + gibbs_base(I, a.others, st, sld) + (int64_t)s * I.stride];
            w = e == e0 ? v : __dmul_rn(w, v);
          }
          return w;
        };
        total = weight(0);
        for (int32_t s = 1; s < K; ++s) total = __dadd_rn(total, weight(s));
        const double t = __dmul_rn(u, total);
        int32_t first_total = K;
        double cs = 0.0;
        k = K;
        for (int32_t s = 0; s < K; ++s) {
          cs = s == 0 ? weight(0) : __dadd_rn(cs, weight(s));
          if (cs > t) {
            k = s;
            break;
          }
          if (first_total == K && cs == total) first_total = s;
        }
        if (k == K) k = first_total;
      }
      // a total that is not finite or not > 0: the state has probability 0; the code stays
      if (total > 0.0 && total <= 1.79769313486231570815e308 && k < K) st[(int64_t)c * sld] = (uint8_t)k;
      else undrawn = true;
    }
    if (a.trace && j % a.thin == 0) {
      uint8_t *t = a.trace + (j / a.thin - 1) * a.n_chains + r;  // a record is a contiguous run of chains
      for (int32_t c = 0; c < a.n_cols; ++c) t[(int64_t)c * a.ld_trace] = st[(int64_t)c * sld];
    }
  }
  if constexpr (LDS)
    for (int32_t c = 0; c < a.n_cols; ++c) g[(int64_t)c * a.ld] = st[(int64_t)c * sld];
  if (undrawn) atomicOr(a.err, kGibbsErrTotal);
}

// the start state of a model that cannot be forward-sampled: column c of chain r is floor(u * card) from
// the sweep-0 uniform of (seed, r, c)
__global__ __launch_bounds__(kGibbsBlock) void k_gibbs_start(const int32_t *__restrict__ card, int32_t n_cols,
                                                            uint8_t *__restrict__ codes, int64_t ld, int64_t row0,
                                                            int64_t n_chains, int64_t first_chain, uint64_t seed) {
  const int64_t r = (int64_t)blockIdx.x * kGibbsBlock + threadIdx.x;
  if (r >= n_chains) return;
  for (int32_t c = 0; c < n_cols; ++c) {
    const int32_t K = card[c];
    const int32_t s = (int32_t)(sample_uniform3(seed, (uint64_t)(first_chain + r), (uint32_t)c, 0u) * (double)K);
    codes[(int64_t)c * ld + row0 + r] = (uint8_t)(s < K - 1 ? s : K - 1);
  }
}

// ---------------------------------------------------------------------------- the handle's device side
// the descriptors and the staging buffer of a call's clamp on the current device
static int gibbs_use(GibbsHandle *h) {
  using pgmdev::upload;
  const GibbsPlan &p = h->p;
  const pgmdev::Slot base[] = {upload(h->d_card, p.card), upload(h->d_inc_off, p.inc_off), upload(h->d_inc, p.inc),
                               upload(h->d_others, p.others), pgmdev::scratch(h->d_clamp, p.card.size())};
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_gibbs_plan_destroy(void *plan) { return pgm_plan_destroy<GibbsHandle>(plan); }

int pgm_gibbs_start(void *plan, uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_chains,
                    int64_t first_chain, uint64_t seed, void *stream) {
  GibbsHandle *h = static_cast<GibbsHandle *>(plan);
  int64_t blocks = 0;
  const int st = gibbs_start_check(h, codes, n_cols, ld, row0, n_chains, first_chain, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  const int up = gibbs_use(h);
  if (up != PGM_OK) return up;
  hipLaunchKernelGGL(k_gibbs_start, dim3((unsigned)blocks), dim3(kGibbsBlock), 0, S(stream), h->d_card, h->p.n_cols, codes,
                     ld, row0, n_chains, first_chain, seed);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_gibbs_sweep(void *plan, const double *values, uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                    int64_t n_chains, int64_t first_chain, int64_t first_sweep, int64_t n_sweeps, uint64_t seed,
                    const uint8_t *clamp, uint8_t *trace, int64_t ld_trace, int64_t thin, const double *uniforms,
                    void *stream) {
  GibbsHandle *h = static_cast<GibbsHandle *>(plan);
  int64_t blocks = 0;
  const int st = gibbs_sweep_check(h, values, codes, n_cols, ld, row0, n_chains, first_chain, first_sweep, n_sweeps,
                                   trace, ld_trace, thin, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  const GibbsPlan &p = h->p;
  GibbsArgs a;
  memset(&a, 0, sizeof a);
  int up = gibbs_use(h);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up == PGM_OK) up = stage_bytes(h->d_clamp, clamp, (size_t)p.n_cols, stream, &a.clamp);
  if (up != PGM_OK) return up;
  a.card = h->d_card, a.inc_off = h->d_inc_off, a.inc = h->d_inc, a.others = h->d_others;
  a.values = values, a.codes = codes, a.trace = trace, a.uniforms = uniforms, a.err = h->dev.flag();
  a.ld = ld, a.row0 = row0, a.n_chains = n_chains, a.first_chain = first_chain, a.first_sweep = first_sweep;
  a.n_sweeps = n_sweeps, a.ld_trace = ld_trace, a.thin = thin, a.seed = seed;
  a.n_cols = p.n_cols, a.n_cols_codes = n_cols;
  const dim3 grid((unsigned)blocks), wg(kGibbsBlock);
  if (gibbs_lds_path(p)) {
    const size_t lds = (size_t)p.n_cols * kGibbsBlock;
    if (uniforms) hipLaunchKernelGGL((k_gibbs_sweep<true, true>), grid, wg, lds, S(stream), a);
    else hipLaunchKernelGGL((k_gibbs_sweep<true, false>), grid, wg, lds, S(stream), a);
  } else {
    if (uniforms) hipLaunchKernelGGL((k_gibbs_sweep<false, true>), grid, wg, 0, S(stream), a);
    else hipLaunchKernelGGL((k_gibbs_sweep<false, false>), grid, wg, 0, S(stream), a);
  }
  // the status is this call's: the flags are read back after the launch (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad & kGibbsErrCode) return pgmi_fail(PGM_EINDEX, "gibbs_sweep: a state code is >= its variable's cardinality");
  if (bad & kGibbsErrTotal)
    return pgmi_fail(PGM_EINVAL, "gibbs_sweep: a conditional's total is not finite or not > 0 (the state has probability 0)");
  return PGM_OK;
}
}

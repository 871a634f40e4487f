// pgmsample.hip — forward sampling on the device (gfx950): the running-sum kernel and the sampling kernel
// behind pgmpy_amd.sampling.BayesianModelSampling and DiscreteBayesianNetwork.simulate, and their C-ABI
// (pgm_sample_plan_destroy, pgm_sample_cdf, pgm_sample_forward).  Replaces the reference's per-node numpy
// loop over the unique parent configurations (sampling/Sampling.py:89-133, :341-400).  The host side
// (validation, argument checks, the host-only queries) is pgmsample_plan.cpp.
#include "pgm_hip_common.h"
#include "pgm_sample.h"

// ---------------------------------------------------------------------------- running sums
// One work-item per CPD column (a parent configuration of one family; the family is found by bisection
// over col_off, as k_fit_finish does): c_0 = p_0, c_s = c_{s-1} + p_s, strictly in state order.  A column
// whose total is not finite or not > 0 cannot be drawn from: *err is raised.
__global__ __launch_bounds__(256) void k_sample_cdf(const FitFam *__restrict__ fams,
                                                    const int64_t *__restrict__ col_off, int32_t n_fam,
                                                    const double *__restrict__ values, double *__restrict__ cdf,
                                                    int32_t *__restrict__ err) {
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
  const int64_t ncol = F.stride[0];  // parent configurations
  const int64_t at = F.off + (c - col_off[lo]);
  double sum = 0.0;
  for (int32_t s = 0; s < card; ++s) {
    sum += values[at + s * ncol];
    cdf[at + s * ncol] = sum;
  }
  if (!(sum > 0.0) || !(sum <= 1.79769313486231570815e308)) atomicOr(err, 1);
}

// ---------------------------------------------------------------------------- sampling
// N rows of one lane through every family in plan order (N = 4: the 4 codes of a column are one aligned
// dword; N = 1: one byte).  `at` is the first row's index in the buffer (row0 + r), `srow` its index in
// the stream (first_row + r).  Returns whether a given code was neither a state nor PGM_EV_MISSING.
template <int N, bool W, bool U>
__device__ __forceinline__ bool sample_walk(const FitFam *__restrict__ fams, int32_t n_fam,
                                            const uint8_t *__restrict__ modes, const double *__restrict__ values,
                                            const double *__restrict__ cdf, uint8_t *codes, int64_t ld, int64_t at,
                                            uint64_t srow, uint64_t seed, double *__restrict__ weights,
                                            const double *__restrict__ uniforms) {
  static_assert(N == 1 || N == 4, "a byte or a dword of codes");
  auto load = [](const uint8_t *p) -> uint32_t {
    if constexpr (N == 4) return *reinterpret_cast<const uint32_t *>(p);
    else return *p;
  };
  double w[N];
#pragma unroll
  for (int j = 0; j < N; ++j) w[j] = 1.0;
  uint32_t dead = 0;  // bit j: row j met a bad given code; the nodes after it are PGM_EV_MISSING
  for (int32_t f = 0; f < n_fam; ++f) {
    const FitFam &F = fams[f];  // workgroup-uniform: scalar loads
    const uint32_t mode = modes ? modes[f] : (uint32_t)PGM_SAMPLE_FREE;
    const int32_t nv = F.n_vars, card = F.card[0], ncol = F.stride[0];
    // the CPD column of each row, from the parent codes this lane stored itself (or was given)
    int32_t col[N];
#pragma unroll
    for (int j = 0; j < N; ++j) col[j] = 0;
    for (int32_t v = 1; v < nv; ++v) {
      const uint32_t q = load(codes + (int64_t)F.col[v] * ld + at);
      const int32_t stride = F.stride[v];
#pragma unroll
      for (int j = 0; j < N; ++j) col[j] += (int32_t)((q >> (8 * j)) & 255u) * stride;
    }
    uint8_t *cp = codes + (int64_t)F.col[0] * ld + at;
    const uint32_t given = mode != PGM_SAMPLE_FREE ? load(cp) : 0xffffffffu;
    const double *cc = cdf + F.off;
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const uint32_t g = (given >> (8 * j)) & 255u;
      uint32_t s;
      if (dead >> j & 1u) {
        s = PGM_EV_MISSING;  // its parents may be missing too: col[j] is not used
      } else if (g == PGM_EV_MISSING) {
        double u;
        if constexpr (U) u = uniforms[(int64_t)F.col[0] * ld + at + j];
        else u = sample_uniform(seed, srow + (uint64_t)j, (uint32_t)F.col[0]);
        s = (uint32_t)sample_select(cc + col[j], card, ncol, u);
      } else if (g >= (uint32_t)card) {
        s = g;  // stays as given; never an index
        dead |= 1u << j;
        w[j] = 0.0;
      } else {
        s = g;
        if constexpr (W) {
          if (mode == PGM_SAMPLE_OBSERVED) {
            const int64_t i = F.off + col[j];
            w[j] *= values[i + (int64_t)s * ncol] / cdf[i + (int64_t)(card - 1) * ncol];
          }
        }
      }
      out |= s << (8 * j);
    }
    if constexpr (N == 4) *reinterpret_cast<uint32_t *>(cp) = out;
    else *cp = (uint8_t)out;
  }
  if constexpr (W) {
#pragma unroll
    for (int j = 0; j < N; ++j) weights[at + j] = w[j];
  }
  return dead != 0;
}

// One launch draws every node of n_rows rows: workgroup b takes rows [b, b + 1) * kSampleRowsPerBlock, a
// work-item owns rows and walks the families in plan order.
// `codes` is ONE pointer, read and written, without __restrict__: a work-item reads back the parent codes
// it stored itself, so a const __restrict__ input next to a __restrict__ output would promise the compiler
// an absence of aliasing that is false and would let it move the read-back above the store.
// V4 (codes, ld and row0 multiples of 4: codes_vec4): a lane owns 4 consecutive rows and moves their 4
// codes of a column as one aligned dword, so a wave's store is 256 contiguous bytes; the rows of the tail
// that do not fill a dword take the one-row path.
// W: an fp64 weight per row (likelihood weighting).  U: uniforms from the caller's matrix, not Philox.
template <bool V4, bool W, bool U>
__global__ __launch_bounds__(kSampleBlock) void k_sample_forward(const FitFam *__restrict__ fams, int32_t n_fam,
                                                                 const uint8_t *__restrict__ modes,
                                                                 const double *__restrict__ values,
                                                                 const double *__restrict__ cdf, uint8_t *codes,
                                                                 int64_t ld, int64_t row0, int64_t n_rows,
                                                                 int64_t first_row, uint64_t seed,
                                                                 double *__restrict__ weights,
                                                                 const double *__restrict__ uniforms,
                                                                 int32_t *__restrict__ err) {
  const int64_t r_begin = (int64_t)blockIdx.x * kSampleRowsPerBlock;
  const int64_t r_end = r_begin + kSampleRowsPerBlock < n_rows ? r_begin + kSampleRowsPerBlock : n_rows;
  constexpr int RPL = V4 ? 4 : 1;  // rows per lane and step
  bool bad = false;
  for (int64_t r = r_begin + (int64_t)threadIdx.x * RPL; r < r_end; r += kSampleBlock * RPL) {
    if (V4 && r + 4 <= r_end) {
      bad |= sample_walk<4, W, U>(fams, n_fam, modes, values, cdf, codes, ld, row0 + r, (uint64_t)(first_row + r), seed,
                                  weights, uniforms);
      continue;
    }
    const int64_t r_stop = r + RPL < r_end ? r + RPL : r_end;
    for (int64_t rr = r; rr < r_stop; ++rr)
      bad |= sample_walk<1, W, U>(fams, n_fam, modes, values, cdf, codes, ld, row0 + rr, (uint64_t)(first_row + rr),
                                  seed, weights, uniforms);
  }
  if (bad) atomicOr(err, 1);
}

// ---------------------------------------------------------------------------- the handle's device side
// the descriptors and the staging buffer of a call's modes on the current device
int sample_use(SampleHandle *h, int stage) {
  const FitPlan &p = h->p.fit;
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_fams, p.fams), pgmdev::upload(h->d_col_off, p.col_off),
                               pgmdev::scratch(h->d_modes, p.fams.size())};
  if (stage == kSamplePosterior) {
    const pgmdev::Slot lw[] = {pgmdev::scratch(h->d_lw_max, (size_t)PGM_LW_MAX_GROUPS),
                               pgmdev::scratch(h->d_lw_sums, (size_t)3 * PGM_LW_MAX_GROUPS)};
    return h->dev.use(kHipDevOps, base, stage, lw);
  }
  return h->dev.use(kHipDevOps, base);
}

extern "C" {

int pgm_sample_plan_destroy(void *plan) { return pgm_plan_destroy<SampleHandle>(plan); }

int pgm_sample_cdf(void *plan, const double *values, double *cdf, void *stream) {
  SampleHandle *h = static_cast<SampleHandle *>(plan);
  const int st = sample_cdf_check(h, values, cdf);
  if (st != PGM_OK) return st;
  int up = sample_use(h);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  const int64_t blocks = (h->p.fit.col_off.back() + 255) / 256;
  hipLaunchKernelGGL(k_sample_cdf, dim3((unsigned)blocks), dim3(256), 0, S(stream), h->d_fams, h->d_col_off,
                     (int32_t)h->p.fit.fams.size(), values, cdf, h->dev.flag());
  // PGM_EINVAL is this call's status: the flag is read back after the launch (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad) return pgmi_fail(PGM_EINVAL, "sample_cdf: a CPD column's total is not finite or not > 0");
  return PGM_OK;
}

int pgm_sample_forward(void *plan, const double *values, const double *cdf, const uint8_t *modes, uint8_t *codes,
                       int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int64_t first_row, uint64_t seed,
                       double *weights, const double *uniforms, void *stream) {
  SampleHandle *h = static_cast<SampleHandle *>(plan);
  int64_t blocks = 0;
  const int st = sample_forward_check(h, values, cdf, modes, codes, n_cols, ld, row0, n_rows, first_row, weights, &blocks);
  if (st != PGM_OK) return st;
  if (blocks == 0) return PGM_OK;
  const int32_t nf = (int32_t)h->p.fit.fams.size();
  const uint8_t *d_modes = nullptr;  // FREE is 0: a call whose modes are all free passes none
  int up = sample_use(h);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up == PGM_OK) up = stage_bytes(h->d_modes, modes, (size_t)nf, stream, &d_modes);
  if (up != PGM_OK) return up;
  const dim3 grid((unsigned)blocks), wg(kSampleBlock);
  const bool v4 = codes_vec4(codes, ld, row0);
#define SAMPLE_LAUNCH(V4, W, U)                                                                                  \
  hipLaunchKernelGGL((k_sample_forward<V4, W, U>), grid, wg, 0, S(stream), h->d_fams, nf, d_modes, values, cdf, \
                     codes, ld, row0, n_rows, first_row, seed, weights, uniforms, h->dev.flag())
#define SAMPLE_LAUNCH_WU(V4)               \
  do {                                     \
    if (weights && uniforms) SAMPLE_LAUNCH(V4, true, true);   \
    else if (weights) SAMPLE_LAUNCH(V4, true, false);         \
    else if (uniforms) SAMPLE_LAUNCH(V4, false, true);        \
    else SAMPLE_LAUNCH(V4, false, false);                     \
  } while (0)
  if (v4) SAMPLE_LAUNCH_WU(true);
  else SAMPLE_LAUNCH_WU(false);
#undef SAMPLE_LAUNCH_WU
#undef SAMPLE_LAUNCH
  // PGM_EINDEX is this call's status: the flag is read back after the launch (synchronises the stream)
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad) return pgmi_fail(PGM_EINDEX, "sample_forward: a given state code is >= its variable's cardinality");
  return PGM_OK;
}
}

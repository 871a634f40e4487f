// pgmemrows.hip — the E-step on rows with missing cells (gfx950): pgm_fit_estep_rows, behind
// ExpectationMaximization(incomplete="marginalize") and BayesianModelProbability.log_probability(incomplete=
// "marginalize").  The set of unobserved variables differs from row to row, so a row that needs work gets a wave,
// not a lane; the sum over its unobserved variables is taken per connected component of those variables (two
// are linked when a family holds both), so a row costs the sum of its components' configurations, not their
// product.  The contract is include/pgmhip.h's; the host side (column lists, checks) is pgmemrows_plan.cpp.
//
// A workgroup takes kEmrRows rows in passes of kEmrBlock.
// Phase 0: lane t scans row t of the pass over the plan's column list (for a fixed column consecutive lanes read
//   consecutive bytes), counts its unobserved cells and checks its codes; a complete row (unless loglik is
//   wanted), a row with a bad code and a row with more than kEmrMaxU unobserved cells are settled here, the
//   others are compacted into the LDS queue by ballot and prefix.
// Phase 1: wave w takes the queue entries w, w + kEmrWaves, ...  For a row (slice: EmrWave):
//   (a) lanes stride over the columns and append U(r) in ascending column order (ballot / prefix);
//   (b) lanes stride over the (u, incident family) pairs of the host-built column -> families lists; the lane
//       whose u is the family's first member of U appends the family with its mask of U members (ballot /
//       prefix again: the touched list is ordered by (first member, family), whatever the timing);
//   (c) label propagation: one lane per touched family takes the minimum label of its members and atomicMin's
//       it back, until a wave-wide ballot shows no change (at most |U| rounds);
//   (d) every component's configurations and families are counted and the limits decided before any add;
//   (e) per component in ascending label: the component's digits (its variables with >= 2 states, the last in
//       U-order fastest) and its families are staged (one lane per family: table offset, observed part of the
//       entry, stride per digit); lane i takes the configurations i, i + 64, ... in ascending order, forms p_l
//       by gathers from values (small tables: L1 / L2) in the staged family order, a butterfly adds Z_c; a
//       second sweep recomputes p_l and adds p_l / Z_c.  With PGM_EMR_NO_FLOOR every Z_c is taken before the
//       first add, since one Z_c = 0 makes the whole row impossible;
//   (f) for loglik lanes stride over the plan's families, add log(value) of the untouched ones in ascending
//       family order each, and a butterfly adds the lanes.
// Every order above depends on the row's own codes only, so a row's loglik and status are bit-identical
// wherever the row sits.  The adds go to the workgroup's fp64 LDS tile when the plan's total_bins fits
// kFitTileBins (flushed once, non-zero bins only, as k_fit_count does), else to global memory; fp64 atomics in
// no fixed order either way.  No matrix instruction applies: gathers and short products without a shared operand.
#include "pgm_emrows.h"
#include "pgm_hip_common.h"

namespace {

__device__ inline void emr_wave_sync() {
  // the lanes of a wave exchange data through the wave's LDS slice: order the accesses around the exchange
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ inline double emr_wave_sum(double v) {
  for (int x = 32; x > 0; x >>= 1) v += __shfl_xor(v, x, 64);  // a + b == b + a: every lane holds the same bits
  return v;
}

__device__ inline bool emr_is_latent(const EmrSpec &s, int32_t pos) {
  bool latent = false;
  for (int32_t j = 0; j < s.n_latent; ++j) latent |= s.pos[j] == pos;
  return latent;
}

// the index in U of code column col, or -1 (u_col ascends)
__device__ inline int32_t emr_find(const EmrWave &w, int32_t n_u, int32_t col) {
  int32_t lo = 0, hi = n_u;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (w.u_col[mid] < col) lo = mid + 1;
    else hi = mid;
  }
  return lo < n_u && w.u_col[lo] == col ? lo : -1;
}

struct EmrArgs {
  const FitFam *fams;
  const int32_t *cols, *card, *inc_off, *inc_fam;
  const double *values;
  const uint8_t *codes;
  int64_t ld;
  double *tables;  // global tables, or nullptr
  double *tile;    // the LDS tile, or nullptr
};

__device__ inline double emr_value(const EmrSpec &s, const double *__restrict__ values, int64_t at) {
  const double v = values[at];
  return (s.flags & PGM_EMR_NO_FLOOR) || v > PGM_EM_FLOOR ? v : PGM_EM_FLOOR;
}

// Stage component `root` (its digits and families) into the slice; *n_dig digits, returns its families.
__device__ inline int32_t emr_stage(EmrWave &w, const EmrArgs &a, int32_t lane, int32_t n_u, int32_t n_f, int32_t root,
                                    int64_t row, int32_t *n_dig) {
  const unsigned long long lt = (1ull << lane) - 1;
  {
    const bool in = lane < n_u && w.u_label[lane] == root;
    const bool dig = in && w.u_card[lane] >= 2;
    const unsigned long long m = __ballot(dig);
    if (lane < n_u) w.u_slot[lane] = dig ? (int32_t)__popcll(m & lt) : -1;
    if (dig) w.c_card[__popcll(m & lt)] = w.u_card[lane];
    *n_dig = (int32_t)__popcll(m);  // <= kEmrMaxDigits: the limits were decided before
  }
  emr_wave_sync();
  int32_t n_cf = 0;
  for (int32_t f0 = 0; f0 < n_f; f0 += 64) {
    const int32_t fi = f0 + lane;
    const bool in = fi < n_f && w.u_label[__ffs((int)w.f_mask[fi < n_f ? fi : 0]) - 1] == root;
    const unsigned long long m = __ballot(in);
    if (in) {
      const int32_t cf = n_cf + (int32_t)__popcll(m & lt);  // < kEmrMaxFam: decided before
      const FitFam &F = a.fams[w.f_id[fi]];
      int32_t base = 0;
      for (int32_t j = 0; j < kEmrMaxDigits; ++j) w.c_stride[cf][j] = 0;
      for (int32_t v = 0; v < F.n_vars; ++v) {
        const int32_t u = emr_find(w, n_u, F.col[v]);
        if (u < 0) base += (int32_t)a.codes[(int64_t)F.col[v] * a.ld + row] * F.stride[v];  // a state: checked in phase 0
        else if (w.u_slot[u] >= 0) w.c_stride[cf][w.u_slot[u]] += F.stride[v];
      }
      w.c_base[cf] = base;
      w.c_off[cf] = F.off;
    }
    n_cf += (int32_t)__popcll(m);
  }
  emr_wave_sync();
  return n_cf;
}

// the digits of configuration l of the staged component: the last digit fastest, 0 past n_dig
__device__ inline void emr_digits(const EmrWave &w, int32_t n_dig, int32_t l, int32_t (&d)[kEmrMaxDigits]) {
#pragma unroll
  for (int j = kEmrMaxDigits - 1; j >= 0; --j) {
    d[j] = 0;
    if (j < n_dig) {
      const int32_t c = w.c_card[j];
      d[j] = l % c;
      l /= c;
    }
  }
}

// where staged family cf keeps the configuration with digits d, in the flat layout
__device__ inline int64_t emr_entry(const EmrWave &w, int32_t cf, const int32_t (&d)[kEmrMaxDigits]) {
  int32_t e = w.c_base[cf];
#pragma unroll
  for (int j = 0; j < kEmrMaxDigits; ++j) e += d[j] * w.c_stride[cf][j];
  return w.c_off[cf] + e;
}

// p_l: the product over the staged families, in their order
__device__ inline double emr_weight(const EmrWave &w, const EmrSpec &s, const EmrArgs &a, int32_t n_cf,
                                    const int32_t (&d)[kEmrMaxDigits]) {
  double p = 1.0;
  for (int32_t cf = 0; cf < n_cf; ++cf) p *= emr_value(s, a.values, emr_entry(w, cf, d));
  return p;
}

// One queued row by one wave.  Returns the status; *ll_out: the row's log-likelihood when want_ll.
__device__ int32_t emr_row(EmrWave &w, const EmrSpec &s, const EmrArgs &a, int32_t lane, int64_t row, int32_t n_unobs,
                           bool want_ll, double *ll_out) {
  const unsigned long long lt = (1ull << lane) - 1;
  const bool want_add = a.tables || a.tile;
  const bool no_floor = s.flags & PGM_EMR_NO_FLOOR;
  double ll = 0.0;
  int32_t n_u = 0, n_f = 0;
  bool impossible = false;
  // (f) the logs of the plan's untouched families; taken before (e), since without the floor a zero here
  // makes the row impossible and nothing may be added
  const bool want_rest = want_ll || (no_floor && want_add);
  auto untouched = [&]() {
    double sum = 0.0;
    for (int32_t f = lane; f < s.n_fam; f += 64) {
      const FitFam &F = a.fams[f];
      int32_t idx = 0;
      bool touched = false;
      for (int32_t v = 0; v < F.n_vars; ++v) {
        if (n_unobs > 0 && emr_find(w, n_u, F.col[v]) >= 0) touched = true;
        else idx += (int32_t)a.codes[(int64_t)F.col[v] * a.ld + row] * F.stride[v];
      }
      if (!touched) sum += log(emr_value(s, a.values, F.off + idx));
    }
    return emr_wave_sum(sum);
  };
  if (n_unobs == 0) {
    if (want_rest) ll = untouched();
  } else {
    // (a) U(r), ascending columns
    for (int32_t j0 = 0; j0 < s.n_pos; j0 += 64) {
      const int32_t j = j0 + lane;
      bool un = false;
      int32_t col = 0;
      if (j < s.n_pos) {
        col = a.cols[j];
        un = emr_is_latent(s, j) || a.codes[(int64_t)col * a.ld + row] == PGM_EV_MISSING;
      }
      const unsigned long long m = __ballot(un);
      const int32_t at = n_u + (int32_t)__popcll(m & lt);
      if (un && at < kEmrMaxU) {  // phase 0 counted the same cells: at < n_unobs <= kEmrMaxU
        w.u_col[at] = col;
        w.u_card[at] = a.card[j];
        w.u_label[at] = at;
        w.u_poff[at] = a.inc_off[j];  // for now: where the column's families start
        w.u_nfam[at] = a.inc_off[j + 1] - a.inc_off[j];
      }
      n_u += (int32_t)__popcll(m);
    }
    n_u = n_u < kEmrMaxU ? n_u : kEmrMaxU;
    emr_wave_sync();
    // (b) the touched families: lanes stride over the (u, incident family) pairs
    int32_t my_start = 0, my_deg = 0, total = 0;
    if (lane < n_u) my_start = w.u_poff[lane], my_deg = w.u_nfam[lane];
    {
      int32_t incl = my_deg;  // inclusive prefix over the lanes
      for (int x = 1; x < 64; x <<= 1) {
        const int32_t o = __shfl_up(incl, x, 64);
        if (lane >= x) incl += o;
      }
      total = __shfl(incl, 63, 64);
      emr_wave_sync();
      if (lane < n_u) w.u_poff[lane] = incl - my_deg, w.u_nfam[lane] = my_start;
      if (lane == 0) w.u_poff[n_u] = total;
    }
    emr_wave_sync();
    bool over = false;
    for (int32_t p0 = 0; p0 < total; p0 += 64) {
      const int32_t p = p0 + lane;
      bool own = false;
      int32_t f = 0;
      uint32_t mask = 0;
      if (p < total) {
        int32_t u = 0;
        while (w.u_poff[u + 1] <= p) ++u;  // u < n_u: p < total = u_poff[n_u]
        f = a.inc_fam[w.u_nfam[u] + (p - w.u_poff[u])];
        const FitFam &F = a.fams[f];
        for (int32_t v = 0; v < F.n_vars; ++v) {
          const int32_t m = emr_find(w, n_u, F.col[v]);
          if (m >= 0) mask |= 1u << m;
        }
        own = (__ffs((int)mask) - 1) == u;
      }
      const unsigned long long m = __ballot(own);
      const int32_t at = n_f + (int32_t)__popcll(m & lt);
      if (own && at < kEmrMaxRowFam) w.f_id[at] = f, w.f_mask[at] = mask;
      n_f += (int32_t)__popcll(m);
      if (n_f > kEmrMaxRowFam) {  // wave-uniform
        over = true;
        break;
      }
    }
    emr_wave_sync();
    if (over) return 2;
    // (c) label propagation
    for (;;) {
      bool changed = false;
      for (int32_t fi = lane; fi < n_f; fi += 64) {
        const uint32_t mask = w.f_mask[fi];
        int32_t lo = kEmrMaxU;
        for (uint32_t b = mask; b; b &= b - 1) {
          const int32_t l = w.u_label[__ffs((int)b) - 1];
          lo = l < lo ? l : lo;
        }
        for (uint32_t b = mask; b; b &= b - 1) changed |= atomicMin(&w.u_label[__ffs((int)b) - 1], lo) > lo;
      }
      emr_wave_sync();
      if (!__any(changed)) break;
    }
    // (d) the limits of every component, before any add
    if (lane < n_u) w.u_nfam[lane] = 0;
    emr_wave_sync();
    for (int32_t fi = lane; fi < n_f; fi += 64) atomicAdd(&w.u_nfam[w.u_label[__ffs((int)w.f_mask[fi]) - 1]], 1);
    emr_wave_sync();
    bool bad = false;
    if (lane < n_u && w.u_label[lane] == lane) {
      int64_t configs = 1;
      for (int32_t u = lane; u < n_u; ++u)
        if (w.u_label[u] == lane && configs <= PGM_EM_MAX_CONFIGS) configs *= w.u_card[u];
      bad = configs > PGM_EM_MAX_CONFIGS || w.u_nfam[lane] > kEmrMaxFam;
      w.u_configs[lane] = bad ? 0 : (int32_t)configs;
    }
    emr_wave_sync();
    if (__any(bad)) return 2;
    const double rest = want_rest ? untouched() : 0.0;
    impossible = rest == -INFINITY;  // only without the floor
    // (e) the components in ascending label; with the floor Z_c > 0, so the adds follow each Z_c at once
    for (int32_t pass = 0; pass < 2 && !impossible; ++pass) {
      if (pass == 1 && !(no_floor && want_add)) break;
      for (int32_t root = 0; root < n_u; ++root) {
        if (w.u_label[root] != root) continue;
        int32_t n_dig = 0;
        const int32_t n_cf = emr_stage(w, a, lane, n_u, n_f, root, row, &n_dig);
        const int32_t configs = w.u_configs[root];
        double z;
        if (pass == 0) {
          z = 0.0;
          for (int32_t l = lane; l < configs; l += 64) {
            int32_t d[kEmrMaxDigits];
            emr_digits(w, n_dig, l, d);
            z += emr_weight(w, s, a, n_cf, d);
          }
          z = emr_wave_sum(z);
          if (lane == 0) w.u_z[root] = z;
          if (z == 0.0) impossible = true;  // only without the floor
          ll += log(z);
        } else {
          z = w.u_z[root];
        }
        if (want_add && (pass == 1 || !no_floor))
          for (int32_t l = lane; l < configs; l += 64) {
            int32_t d[kEmrMaxDigits];
            emr_digits(w, n_dig, l, d);
            const double wgt = emr_weight(w, s, a, n_cf, d) / z;
            for (int32_t cf = 0; cf < n_cf; ++cf) {
              if (a.tile) atomicAdd(&a.tile[emr_entry(w, cf, d)], wgt);
              else atomicAdd(&a.tables[emr_entry(w, cf, d)], wgt);
            }
          }
        emr_wave_sync();  // the stage is rewritten by the next component
      }
    }
    ll += rest;
  }
  impossible |= ll == -INFINITY;  // a complete row with a zero entry
  if (want_ll) *ll_out = impossible ? -INFINITY : ll;
  return impossible ? 3 : (n_unobs > 0 ? 1 : 0);
}

__global__ __launch_bounds__(kEmrBlock) void k_fit_estep_rows(const FitFam *__restrict__ fams,
                                                              const int32_t *__restrict__ cols,
                                                              const int32_t *__restrict__ card,
                                                              const int32_t *__restrict__ inc_off,
                                                              const int32_t *__restrict__ inc_fam, const EmrSpec s,
                                                              const double *__restrict__ values,
                                                              const uint8_t *__restrict__ codes, int64_t ld, int64_t row0,
                                                              int64_t n_rows, double *__restrict__ tables,
                                                              double *__restrict__ loglik, uint8_t *__restrict__ status,
                                                              unsigned long long *__restrict__ skipped,
                                                              int32_t *__restrict__ err) {
  extern __shared__ unsigned char emr_lds[];
  __shared__ EmrWave s_wave[kEmrWaves];
  __shared__ int32_t s_queue[kEmrBlock];
  __shared__ int32_t s_qn, s_skip;
  double *tile = s.tile ? reinterpret_cast<double *>(emr_lds) : nullptr;
  const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned long long lt = (1ull << lane) - 1;
  const int64_t r_begin = (int64_t)blockIdx.x * kEmrRows;
  const int64_t r_end = r_begin + kEmrRows < n_rows ? r_begin + kEmrRows : n_rows;
  const bool want_ll = loglik != nullptr;
  if (tile)
    for (int32_t i = tid; i < s.total_bins; i += kEmrBlock) tile[i] = 0.0;
  if (tid == 0) s_skip = 0;
  const EmrArgs a = {fams, cols, card, inc_off, inc_fam, values, codes, ld, tile ? nullptr : tables, tile};
  bool any_bad = false;
  int32_t n_skip = 0;  // lane 0 of each wave counts
  for (int64_t r0 = r_begin; r0 < r_end; r0 += kEmrBlock) {
    if (tid == 0) s_qn = 0;
    __syncthreads();
    // phase 0: one row per lane
    const int64_t r = r0 + tid;
    bool queue = false;
    int32_t n_unobs = 0;
    if (r < r_end) {
      const int64_t row = row0 + r;
      bool bad = false;
      for (int32_t j = 0, k = 0; j < s.n_pos; ++j) {
        if (k < s.n_latent && s.pos[k] == j) {  // virtual: never read
          ++k, ++n_unobs;
          continue;
        }
        const uint32_t c = codes[(int64_t)cols[j] * ld + row];
        if (c == PGM_EV_MISSING) ++n_unobs;
        else bad |= c >= (uint32_t)card[j];
      }
      if (bad) {
        any_bad = true;
        if (status) status[row] = 4;
        if (want_ll) loglik[row] = NAN;
      } else if (n_unobs > kEmrMaxU) {
        atomicAdd(&s_skip, 1);
        if (status) status[row] = 2;
        if (want_ll) loglik[row] = NAN;
      } else if (n_unobs > 0 || want_ll) {
        queue = true;
      } else if (status) {
        status[row] = 0;
      }
    }
    {
      const unsigned long long m = __ballot(queue);
      int32_t base = 0;
      if (lane == 0 && m) base = atomicAdd(&s_qn, (int32_t)__popcll(m));
      base = __shfl(base, 0, 64);
      if (queue) s_queue[base + (int32_t)__popcll(m & lt)] = tid | (n_unobs << 16);
    }
    __syncthreads();
    // phase 1: one wave per queued row
    const int32_t qn = s_qn;
    for (int32_t q = wv; q < qn; q += kEmrWaves) {
      const int32_t ent = s_queue[q];
      const int64_t row = row0 + r0 + (ent & 0xffff);
      double ll = 0.0;
      const int32_t st = emr_row(s_wave[wv], s, a, lane, row, ent >> 16, want_ll, &ll);
      if (lane == 0) {
        if (st == 2) ++n_skip;
        if (status) status[row] = (uint8_t)st;
        if (want_ll) loglik[row] = st == 2 ? NAN : ll;
      }
      emr_wave_sync();  // the slice is rewritten by the next row
    }
    __syncthreads();  // the queue is rewritten by the next pass
  }
  if (n_skip) atomicAdd(&s_skip, n_skip);
  if (any_bad) atomicOr(err, 1);
  __syncthreads();
  if (tid == 0 && s_skip) atomicAdd(skipped, (unsigned long long)s_skip);
  if (tile)
    for (int32_t i = tid; i < s.total_bins; i += kEmrBlock) {
      const double v = tile[i];
      if (v != 0.0) atomicAdd(&tables[i], v);
    }
}

}  // namespace

extern "C" int pgm_fit_estep_rows(void *plan, const int32_t *latent_cols, int32_t n_latent, int32_t flags,
                                  const double *values, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                                  int64_t n_rows, double *tables, double *loglik, uint8_t *status, int64_t *n_skipped,
                                  void *stream) {
  FitHandle *h = static_cast<FitHandle *>(plan);
  EmrSpec spec;
  int64_t blocks = 0;
  const int st = emr_check(h, latent_cols, n_latent, flags, values, codes, n_cols, ld, row0, n_rows, tables, loglik, &spec,
                           &blocks);
  if (st != PGM_OK) return st;
  if (n_skipped) *n_skipped = 0;
  if (blocks == 0) return PGM_OK;
  int up = fit_use(h, kFitEmRows);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  HIP_TRY(hipMemsetAsync(h->d_emr_skipped, 0, sizeof(unsigned long long), S(stream)));
  const size_t lds = spec.tile ? (size_t)spec.total_bins * sizeof(double) : 0;
  hipLaunchKernelGGL(k_fit_estep_rows, dim3((unsigned)blocks), dim3(kEmrBlock), lds, S(stream), h->d_fams, h->d_emr_cols,
                     h->d_emr_card, h->d_emr_inc_off, h->d_emr_inc_fam, spec, values, codes, ld, row0, n_rows, tables,
                     loglik, status, h->d_emr_skipped, h->dev.flag());
  // PGM_EINDEX is this call's status, as in pgm_fit_count; the count of skipped rows comes with the flag word
  unsigned long long skipped = 0;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&skipped, h->d_emr_skipped, sizeof skipped, hipMemcpyDeviceToHost, S(stream)));
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (n_skipped) *n_skipped = (int64_t)skipped;
  if (bad) return pgmi_fail(PGM_EINDEX, "fit_estep_rows: a state code is neither missing nor < its variable's cardinality");
  return PGM_OK;
}

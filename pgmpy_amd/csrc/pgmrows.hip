// pgmrows.hip — the device side and the C-ABI of the fused row plan (the path bench.py measures).
//
// Built with pgmhip.hip in one hipcc command (pgmpy_amd/build.py).  The host arithmetic — validating
// and compiling a pgm_rows_plan into descriptors, generating the plan-specialised kernel source, the
// two-rows-per-thread predicates — is pgmrows_plan.cpp; the structs both sides share: pgm_rows.h.
//
// Kernels
//   k_rows          fused per-row plan: reduce -> sum-product -> normalize -> marginals / joint / MAP,
//                   one lane per evidence row, table-driven components
//   k_rows_affine   the same for all-affine plans, descriptors in registers
// C-ABI
//   pgm_rows_plan_create / source / destroy / run / bind, pgm_rows_bound_*, pgm_rows_shard_run,
//   pgm_rows_ring_*; pgmi_rows_bound_jit for the direct AQL path (pgmdq.cpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "pgmhip.h"
#include "pgm_internal.h"
#include "pgm_hip_common.h"
#include "pgm_rows.h"

// ----------------------------------------------------------------------------- fused row plan
// One workgroup owns 64 evidence rows (one per lane) for RG consecutive row groups; its waves split
// the plan's independent components (wave w takes components w, w+W, ...), so every descriptor
// read, loop bound and branch is wave-uniform (scalar) and a row's work is spread over W
// wavefronts.  A wave loads only its components' evidence codes (all in flight at once) and
// stages only their CPT values into LDS.  Components meet once per row group through LDS: masses
// (impossible evidence makes every marginal NaN), MAP index digits and MAP gaps.
// (descriptor layout: pgm_rows.h)
template <bool VL, bool AL, int MAXFC, int MAXT>
__global__ __launch_bounds__(64 * PGM_ROWS_MAX_COMP) void k_rows(
    const RowsK p, const double *__restrict__ gvals, const int32_t *__restrict__ desc,
    const uint8_t *__restrict__ codes, int64_t ld_codes, int64_t row0, int64_t n_rows, int32_t mode, int32_t RG,
    double *__restrict__ marg, double *__restrict__ joint, int64_t ld_out, int32_t *__restrict__ map,
    double *__restrict__ gap, int32_t *__restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // this wave's component
  const int NC = p.n_comp;
  const RowsComp &cd = ((const RowsComp *)desc)[c];
  const RowsTerm *__restrict__ tt = (const RowsTerm *)(desc + p.terms_off) + cd.ev_lo;
  const int32_t *__restrict__ tab = desc + p.tab_off;
  double *svals = lds;
  double *xmass = lds + (VL ? ((p.n_values + 1) & ~1) : 0);  // [NC][64]
  double *xgap = xmass + NC * 64;                              // [NC][64]
  int32_t *xmap = (int32_t *)(xgap + NC * 64);                 // [NC][64]
  double *sacc = (double *)(xmap + NC * 64);                   // [n_marg][64]
  const bool do_marg = (mode & PGM_ROWS_MARGINALS) != 0;
  const bool do_joint = (mode & PGM_ROWS_JOINT) != 0;
  const bool do_map = (mode & (PGM_ROWS_MAP | PGM_ROWS_MAPGAP)) != 0;
  const int nf = cd.nf, nq = cd.nq, nt = cd.nt;
  const uint32_t P = cd.P, H = cd.H;
  auto val = [&](int32_t i) -> double {
    if constexpr (VL) return svals[i];
    else return gvals[i];
  };
  // stage this component's CPT values once per workgroup (no other wave reads them: no barrier)
  if constexpr (VL) {
    if (lane == 0) svals[p.one_idx] = 1.0;
    for (int i = cd.val_lo + lane; i < cd.val_hi; i += 64) svals[i] = gvals[i];
  }
  // evidence codes of row group g (MAXT <= 8: padded terms, static descriptor offsets)
  constexpr int NT = MAXT <= 8 ? MAXT : 1;
  auto load_codes = [&](int g, uint32_t (&code)[NT]) {
    const int64_t r = ((int64_t)blockIdx.x * RG + g) * 64 + lane;
    const uint8_t *crow = codes + row0 + (r < n_rows ? r : 0);
#pragma unroll
    for (int j = 0; j < NT; ++j) code[j] = crow[(int64_t)tt[j].col * ld_codes];
  };
  uint32_t nxt[NT];
  if (MAXT <= 8 && nt > 0) load_codes(0, nxt);
  for (int g = 0; g < RG; ++g) {
    const int64_t r = ((int64_t)blockIdx.x * RG + g) * 64 + lane;
    const bool live = r < n_rows;
    auto acc = [&](int32_t t) -> double & {
      if constexpr (AL) return sacc[t * 64 + lane];
      else return marg[(int64_t)t * ld_out + r];
    };
    int32_t cb[MAXFC];  // slots >= nf point at the constant 1.0 (fbase = one_idx, fstride = 0)
#pragma unroll
    for (int j = 0; j < MAXFC; ++j) cb[j] = cd.fbase[j];
    bool bad = false;
    if (nt == 0) {
      // no evidence in this component: nothing to load (codes may have no columns at all)
    } else if constexpr (MAXT <= 8) {
      uint32_t code[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) code[j] = nxt[j];
      if (g + 1 < RG) load_codes(g + 1, nxt);  // next row group's codes in flight during this one
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const RowsTerm &t = tt[j];
        const bool oob = code[j] >= (uint32_t)t.card;
        bad |= oob;
        const int32_t w = oob ? 0 : (int32_t)code[j] * t.stride;
#pragma unroll
        for (int k = 0; k < MAXFC; ++k) cb[k] += (k == t.slot) ? w : 0;
      }
    } else {
      const uint8_t *crow = codes + row0 + (live ? r : 0);
      for (int j = 0; j < nt; ++j) {
        const RowsTerm &t = tt[j];
        uint32_t cv = crow[(int64_t)t.col * ld_codes];
        if (cv >= (uint32_t)t.card) {
          bad = true;
          cv = 0;
        }
        const int32_t w = (int32_t)cv * t.stride;
#pragma unroll
        for (int k = 0; k < MAXFC; ++k) cb[k] += (k == t.slot) ? w : 0;
      }
    }
    if (bad && live && err) atomicOr(err, 1);
    double mass = 0.0, best = -1.0, second = -1.0;
    int32_t best_map = 0;
    if (cd.simple) {
      // affine: states [0, RC) stay in registers (branch-free clamped loads, all LDS reads of
      // the pass in flight at once); states >= RC are recomputed in the write pass
      const int32_t ms = cd.mstride;
      constexpr int RC = 8;
      double pc[RC];
      const int32_t plast = (int32_t)P - 1;
#pragma unroll
      for (int qs = 0; qs < RC; ++qs) {
        const int32_t q = qs < plast ? qs : plast;
        double prod = val(cb[0] + q * cd.fstride[0]);
#pragma unroll
        for (int j = 1; j < MAXFC; ++j) prod *= val(cb[j] + q * cd.fstride[j]);
        pc[qs] = prod;
      }
      auto visit = [&](uint32_t qs, double prod) {
        mass += prod;
        if (do_joint && live) joint[(int64_t)qs * ms * ld_out + r] = prod;
        if (do_map) {
          if (prod > best) {
            second = best;
            best = prod;
            best_map = (int32_t)qs * ms;
          } else if (prod > second) {
            second = prod;
          }
        }
      };
#pragma unroll
      for (int qs = 0; qs < RC; ++qs)
        if ((uint32_t)qs < P) visit(qs, pc[qs]);
      for (uint32_t qs = RC; qs < P; ++qs) {
        double prod = val(cb[0] + (int32_t)qs * cd.fstride[0]);
#pragma unroll
        for (int j = 1; j < MAXFC; ++j) prod *= val(cb[j] + (int32_t)qs * cd.fstride[j]);
        visit(qs, prod);
      }
      if (do_marg && nq && live) {  // normalised marginal streamed straight to HBM
        const double inv = 1.0 / mass;
        double *out = marg + (int64_t)cd.marg0 * ld_out + r;
#pragma unroll
        for (int qs = 0; qs < RC; ++qs)
          if ((uint32_t)qs < P) __builtin_nontemporal_store(pc[qs] * inv, out + (int64_t)qs * ld_out);
        for (uint32_t qs = RC; qs < P; ++qs) {
          double prod = val(cb[0] + (int32_t)qs * cd.fstride[0]);
#pragma unroll
          for (int j = 1; j < MAXFC; ++j) prod *= val(cb[j] + (int32_t)qs * cd.fstride[j]);
          __builtin_nontemporal_store(prod * inv, out + (int64_t)qs * ld_out);
        }
      }
    } else if (live) {
      const int32_t *toff = tab + cd.off_base;
      const int32_t *tmarg = tab + cd.marg_base;
      const int32_t *tmap = tab + cd.map_base;
      if (do_marg && nq > 1) {
        for (int q = cd.q_lo; q < cd.q_hi; ++q)
          for (int s = 0; s < p.q_card[q]; ++s) acc(p.q_marg_off[q] + s) = 0.0;
      }
      uint32_t e = 0;
#pragma unroll 2
      for (uint32_t qi = 0; qi < P; ++qi) {
        double v = 0.0;
        if (H == 1) {  // no hidden dims: one product per query entry
          const int32_t *o = toff + qi * nf;
          double prod = 1.0;
#pragma unroll
          for (int j = 0; j < MAXFC; ++j)
            if (j < nf) prod *= val(cb[j] + o[j]);
          v = prod;
        } else {
          for (uint32_t hi = 0; hi < H; ++hi, ++e) {
            const int32_t *o = toff + e * nf;
            double prod = 1.0;
#pragma unroll
            for (int j = 0; j < MAXFC; ++j)
              if (j < nf) prod *= val(cb[j] + o[j]);
            v += prod;
          }
        }
        mass += v;
        if (do_marg) {
          if (nq == 1) {
            acc(tmarg[qi]) = v;  // each marginal row is hit exactly once
          } else {
            for (int i = 0; i < nq; ++i) acc(tmarg[qi * nq + i]) += v;
          }
        }
        if (do_joint) joint[(int64_t)tmap[qi] * ld_out + r] = v;
        if (do_map) {
          if (v > best) {
            second = best;
            best = v;
            best_map = tmap[qi];
          } else if (v > second) {
            second = v;
          }
        }
      }
      if (do_marg && nq > 0) {  // component marginals normalised by the component mass
        const double inv = 1.0 / mass;
        for (int q = cd.q_lo; q < cd.q_hi; ++q)
          for (int s = 0; s < p.q_card[q]; ++s) {
            const int a = p.q_marg_off[q] + s;
            if constexpr (AL) marg[(int64_t)a * ld_out + r] = acc(a) * inv;
            else acc(a) *= inv;
          }
      }
    }
    if (NC > 1 || do_map) {
      xmass[c * 64 + lane] = mass;
      if (do_map) {
        xmap[c * 64 + lane] = best_map;
        xgap[c * 64 + lane] = (P > 1) ? (best > 0.0 ? (best - (second < 0.0 ? 0.0 : second)) / best : 0.0) : 1.0;
      }
    }
    if (NC > 1) __syncthreads();
    if (live) {
      double z = mass;
      if (NC > 1) {
        z = 1.0;
        for (int c2 = 0; c2 < NC; ++c2) z *= xmass[c2 * 64 + lane];
      }
      // impossible evidence (zero total mass): every marginal is 0/0 = NaN and np.argmax gives 0
      const bool dead = !(z > 0.0);
      if (do_marg && dead) {
        const double nan = __builtin_nan("");
        for (int q = cd.q_lo; q < cd.q_hi; ++q)
          for (int s = 0; s < p.q_card[q]; ++s) marg[(int64_t)(p.q_marg_off[q] + s) * ld_out + r] = nan;
      }
      if (do_joint && c == 0) {  // single-component plans only
        const double inv = 1.0 / z;
        for (int q = 0; q < p.n_joint; ++q) {
          double *j = joint + (int64_t)q * ld_out + r;
          *j = dead ? __builtin_nan("") : *j * inv;
        }
      }
      if (do_map && c == 0) {
        int32_t m = 0;
        double mg = 1.0;
        for (int c2 = 0; c2 < NC; ++c2) {
          m += xmap[c2 * 64 + lane];
          mg = fmin(mg, xgap[c2 * 64 + lane]);
        }
        if (map) map[r] = dead ? 0 : m;
        if (gap && (mode & PGM_ROWS_MAPGAP)) gap[r] = dead ? 0.0 : mg;
      }
    }
    if (NC > 1 && g + 1 < RG) __syncthreads();  // the exchange slots are reused by the next row group
  }
}

// workgroup barrier for LDS-only exchanges: waits for this wave's LDS traffic, not for its global
// loads/stores (__syncthreads' release fence would wait for every outstanding store to be acked)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// All-affine plans (every component one query dim, no hidden dim, <= 4 factors, <= 8 evidence
// terms: the common batched-predict shape, e.g. munin C3).  Same work split as k_rows, but each
// wave loads its component's descriptor into registers once, folds evidence with multiply-adds
// against host-precomputed per-slot strides, and carries the MAP bookkeeping only when asked.
// Latency shape (one row group per wave at 100k rows): descriptor -> {codes, CPT staging} in
// flight together (staging issues every load before any LDS write) -> products -> LDS-only
// exchange of component masses -> stores.  PGM_ROWS_TIMELINE builds add per-wave s_memrealtime
// stamps (tools/rows_timeline.py).
template <bool VL, int NF, int NT, bool MAP>
__global__ __launch_bounds__(64 * PGM_ROWS_MAX_COMP) void k_rows_affine(
    const RowsK p, const double *__restrict__ gvals, const int32_t *__restrict__ desc,
    const uint8_t *__restrict__ codes, int64_t ld_codes, int64_t row0, int64_t n_rows, int32_t mode, int32_t RG,
    double *__restrict__ marg, int64_t ld_out, int32_t *__restrict__ map, double *__restrict__ gap,
    int32_t *__restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
#ifdef PGM_ROWS_TIMELINE
  const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
#endif
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // this wave's component
  const int NC = p.n_comp;
  const RowsComp &cd = ((const RowsComp *)desc)[c];
  double *svals = lds;
  double *xmass = lds + (VL ? ((p.n_values + 1) & ~1) : 0);  // [NC][64]
  double *xgap = xmass + NC * 64;                              // [NC][64] (MAP only)
  int32_t *xmap = (int32_t *)(xgap + NC * 64);                 // [NC][64] (MAP only)
  const bool do_marg = (mode & PGM_ROWS_MARGINALS) != 0;
  // descriptor -> registers (wave-uniform)
  int32_t fb[NF], fs[NF], S[NT][NF];
  uint32_t card[NT];
  int64_t cofs[NT];
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    fb[k] = cd.fbase[k];
    fs[k] = cd.fstride[k];
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    card[j] = (uint32_t)cd.a_card[j];
    cofs[j] = (int64_t)cd.a_col[j] * ld_codes + row0;
#pragma unroll
    for (int k = 0; k < NF; ++k) S[j][k] = cd.a_S[j][k];
  }
  const int nt = cd.nt;
  const bool has_q = cd.nq != 0;
  const uint32_t P = (uint32_t)cd.P;
  const int32_t ms = cd.mstride;
  double *mrow = marg + (int64_t)cd.marg0 * ld_out;
  auto val = [&](int32_t i) -> double {
    if constexpr (VL) return svals[i];
    else return gvals[i];
  };
  auto load_codes = [&](int g, uint32_t (&code)[NT]) {
    const int64_t r = ((int64_t)blockIdx.x * RG + g) * 64 + lane;
    const uint8_t *crow = codes + (r < n_rows ? r : 0);
#pragma unroll
    for (int j = 0; j < NT; ++j) code[j] = crow[cofs[j]];
  };
  // this wave's first 256 CPT values, then the first row group's codes, all in flight before the
  // LDS writes (vmcnt is in order: the writes wait only for the value loads); larger components
  // stage the rest in further 256-value batches
  uint32_t nx[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) nx[j] = 0;
  const int vlo = cd.val_lo, vhi = cd.val_hi;
  double t[4];
  // (a component without factors has vlo == vhi == 0: nothing to stage, and vhi - 1 is no index)
  if constexpr (VL) {
    if (vlo < vhi) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = vlo + u * 64 + lane;
        t[u] = gvals[i < vhi ? i : vhi - 1];
      }
    }
  }
  if (nt > 0) load_codes(0, nx);
  if constexpr (VL) {
    if (lane == 0) svals[p.one_idx] = 1.0;
    if (vlo < vhi) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // clamped lanes rewrite the last value with itself: no branches
        const int i = vlo + u * 64 + lane;
        svals[i < vhi ? i : vhi - 1] = t[u];
      }
    }
    for (int base = vlo + 256; base < vhi; base += 256) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = base + u * 64 + lane;
        t[u] = gvals[i < vhi ? i : vhi - 1];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = base + u * 64 + lane;
        if (i < vhi) svals[i] = t[u];
      }
    }
  }
#ifdef PGM_ROWS_TIMELINE
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  const uint64_t t_ready = __builtin_amdgcn_s_memrealtime();
#endif
  for (int g = 0; g < RG; ++g) {
    const int64_t r = ((int64_t)blockIdx.x * RG + g) * 64 + lane;
    const bool live = r < n_rows;
    uint32_t code[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) code[j] = nx[j];
    if (nt > 0 && g + 1 < RG) load_codes(g + 1, nx);  // next group's codes in flight during this one
    int32_t cb[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) cb[k] = fb[k];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const bool oob = code[j] >= card[j];
      bad |= oob;
      const int32_t cj = oob ? 0 : (int32_t)code[j];
#pragma unroll
      for (int k = 0; k < NF; ++k) cb[k] += cj * S[j][k];
    }
    if (bad && live && err) atomicOr(err, 1);
    constexpr int RC = 8;
    double pc[RC];
    const int32_t plast = (int32_t)P - 1;
#pragma unroll
    for (int qs = 0; qs < RC; ++qs) {
      const int32_t q = qs < plast ? qs : plast;
      double prod = val(cb[0] + q * fs[0]);
#pragma unroll
      for (int k = 1; k < NF; ++k) prod *= val(cb[k] + q * fs[k]);
      pc[qs] = prod;
    }
    double mass = 0.0, best = -1.0, second = -1.0;
    int32_t best_s = 0;
    auto visit = [&](uint32_t qs, double prod) {
      mass += prod;
      if constexpr (MAP) {
        if (prod > best) {
          second = best;
          best = prod;
          best_s = (int32_t)qs;
        } else if (prod > second) {
          second = prod;
        }
      }
    };
#pragma unroll
    for (int qs = 0; qs < RC; ++qs)
      if ((uint32_t)qs < P) visit(qs, pc[qs]);
    for (uint32_t qs = RC; qs < P; ++qs) {
      double prod = val(cb[0] + (int32_t)qs * fs[0]);
#pragma unroll
      for (int k = 1; k < NF; ++k) prod *= val(cb[k] + (int32_t)qs * fs[k]);
      visit(qs, prod);
    }
    // the component waves of a row group meet BEFORE any store, through an LDS-only barrier
    // (no wait for global stores to be acknowledged, as __syncthreads' release fence would)
    double z = mass;
    if (NC > 1) {
      xmass[c * 64 + lane] = mass;
      if constexpr (MAP) {
        xmap[c * 64 + lane] = best_s * ms;
        xgap[c * 64 + lane] = (P > 1) ? (best > 0.0 ? (best - (second < 0.0 ? 0.0 : second)) / best : 0.0) : 1.0;
      }
      lds_barrier();
      z = 1.0;
      for (int c2 = 0; c2 < NC; ++c2) z *= xmass[c2 * 64 + lane];
    }
    // impossible evidence (zero total mass): every marginal is 0/0 = NaN and np.argmax gives 0
    const bool dead = !(z > 0.0);
    // (a component without a query dim has P == 1 and no marginal row: nothing to store, as in k_rows)
    if (do_marg && live && has_q) {  // normalised marginal streamed straight to HBM
      const double inv = dead ? __builtin_nan("") : 1.0 / mass;
      double *out = mrow + r;
#pragma unroll
      for (int qs = 0; qs < RC; ++qs)
        if ((uint32_t)qs < P) out[(int64_t)qs * ld_out] = pc[qs] * inv;
      for (uint32_t qs = RC; qs < P; ++qs) {
        double prod = val(cb[0] + (int32_t)qs * fs[0]);
#pragma unroll
        for (int k = 1; k < NF; ++k) prod *= val(cb[k] + (int32_t)qs * fs[k]);
        out[(int64_t)qs * ld_out] = prod * inv;
      }
    }
    if constexpr (MAP) {
      if (live && c == 0) {
        int32_t m = best_s * ms;
        double mg = (P > 1) ? (best > 0.0 ? (best - (second < 0.0 ? 0.0 : second)) / best : 0.0) : 1.0;
        if (NC > 1) {
          m = 0;
          mg = 1.0;
          for (int c2 = 0; c2 < NC; ++c2) {
            m += xmap[c2 * 64 + lane];
            mg = fmin(mg, xgap[c2 * 64 + lane]);
          }
        }
        if (map) map[r] = dead ? 0 : m;
        if (gap && (mode & PGM_ROWS_MAPGAP)) gap[r] = dead ? 0.0 : mg;
      }
    }
    if (NC > 1 && g + 1 < RG) lds_barrier();  // the exchange slots are reused by the next row group
  }
#ifdef PGM_ROWS_TIMELINE
  {  // [entry, ready, stores issued, stores acked, HW_ID, XCC_ID] per wave into `gap`
    const uint64_t t_issued = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const uint64_t t_done = __builtin_amdgcn_s_memrealtime();
    if (gap && !(mode & PGM_ROWS_MAPGAP) && lane == 0) {
      double *tl = gap + ((int64_t)blockIdx.x * (blockDim.x >> 6) + c) * 6;
      tl[0] = (double)t_entry;
      tl[1] = (double)t_ready;
      tl[2] = (double)t_issued;
      tl[3] = (double)t_done;
      tl[4] = (double)__builtin_amdgcn_s_getreg(4 | (31 << 11));
      tl[5] = (double)__builtin_amdgcn_s_getreg(20 | (15 << 11));
    }
  }
#endif
}

template <bool VL, int NF, int NT>
static void launch_affine_m(bool do_map, dim3 g, dim3 b, size_t lds, hipStream_t s, const RowsK &k,
                            const double *v, const int32_t *t, const uint8_t *codes, int64_t ldc, int64_t row0,
                            int64_t n, int32_t mode, int32_t RG, double *marg, int64_t ldo, int32_t *map,
                            double *gap, int32_t *err) {
  if (do_map)
    hipLaunchKernelGGL((k_rows_affine<VL, NF, NT, true>), g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, ldo, map, gap, err);
  else
    hipLaunchKernelGGL((k_rows_affine<VL, NF, NT, false>), g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, ldo, map, gap, err);
}

// the launchers take the template arguments rows_launch_choose picked (pgm_rows_launch_info_t)
template <bool VL>
static void launch_affine(int nf, int nt, bool do_map, dim3 g, dim3 b, size_t lds, hipStream_t s,
                          const RowsK &k, const double *v, const int32_t *t, const uint8_t *codes, int64_t ldc,
                          int64_t row0, int64_t n, int32_t mode, int32_t RG, double *marg, int64_t ldo,
                          int32_t *map, double *gap, int32_t *err) {
#define PGM_AFF(NF, NT) launch_affine_m<VL, NF, NT>(do_map, g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, ldo, map, gap, err)
  if (nt == 4) {
    if (nf == 1) PGM_AFF(1, 4);
    else if (nf == 2) PGM_AFF(2, 4);
    else PGM_AFF(4, 4);
  } else {
    if (nf == 1) PGM_AFF(1, 8);
    else if (nf == 2) PGM_AFF(2, 8);
    else PGM_AFF(4, 8);
  }
#undef PGM_AFF
}

template <bool VL, bool AL, int MAXT>
static void launch_rows_t(int maxfc, dim3 g, dim3 b, size_t lds, hipStream_t s, const RowsK &k, const double *v,
                          const int32_t *t, const uint8_t *codes, int64_t ldc, int64_t row0, int64_t n, int32_t mode,
                          int32_t RG, double *marg, double *joint, int64_t ldo, int32_t *map, double *gap, int32_t *err) {
  if (maxfc == 2)
    hipLaunchKernelGGL((k_rows<VL, AL, 2, MAXT>), g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, joint, ldo, map, gap, err);
  else if (maxfc == 4)
    hipLaunchKernelGGL((k_rows<VL, AL, 4, MAXT>), g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, joint, ldo, map, gap, err);
  else if (maxfc == 8)
    hipLaunchKernelGGL((k_rows<VL, AL, 8, MAXT>), g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, joint, ldo, map, gap, err);
  else
    hipLaunchKernelGGL((k_rows<VL, AL, PGM_ROWS_MAX_FAC, MAXT>), g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, joint, ldo, map, gap, err);
}

template <bool VL, bool AL>
static void launch_rows_f(int maxt, int maxfc, dim3 g, dim3 b, size_t lds, hipStream_t s, const RowsK &k,
                          const double *v, const int32_t *t, const uint8_t *codes, int64_t ldc, int64_t row0, int64_t n,
                          int32_t mode, int32_t RG, double *marg, double *joint, int64_t ldo, int32_t *map, double *gap,
                          int32_t *err) {
  if (maxt == 4)
    launch_rows_t<VL, AL, 4>(maxfc, g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, joint, ldo, map, gap, err);
  else if (maxt == 8)
    launch_rows_t<VL, AL, 8>(maxfc, g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, joint, ldo, map, gap, err);
  else
    launch_rows_t<VL, AL, PGM_ROWS_MAX_EV>(maxfc, g, b, lds, s, k, v, t, codes, ldc, row0, n, mode, RG, marg, joint, ldo, map, gap, err);
}

// ----------------------------------------------------------------------------- plan handle
// a compiled plan (RowsPlan) on a device
struct RowsHandle : RowsPlan {
  double *d_values = nullptr;
  int32_t *d_desc = nullptr;
  // plan-specialised kernels (hipRTC): jit_src is generated at create for all-affine plans; one program
  // per cache policy of the stream (RowsPolicy), each compiled on first use
  struct Prog {
    std::string src;
    int state = 0;  // 0 not compiled, 1 ready, -1 unavailable
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    hipFunction_t fn2 = nullptr;        // two rows per thread
    hipFunction_t fn_floor = nullptr;   // PGM_ROWS_FLOOR: the same dispatch's loads + stores only
    hipFunction_t fn_floor2 = nullptr;  // ... of the two-rows-per-thread dispatch
    hipFunction_t fn_ring = nullptr;    // the resident ring kernel (pgm_rows_ring_*)
    std::vector<char> code;             // the compiled code object (the direct AQL path loads it again)
    const char *name_of(hipFunction_t f) const {
      return f == fn2 ? "pgm_rows_jit2" : f == fn_floor ? "pgm_rows_floor" : f == fn_floor2 ? "pgm_rows_floor2" : "pgm_rows_jit";
    }
  };
  std::mutex jit_mu;
  Prog prog_default;  // jit_src: when it is unavailable (state -1) the AOT kernels run instead
  Prog prog_stream;   // the same kernels under the streaming policy (rows_stream_policy), bit-identical outputs
  int64_t stream_min_rows = 0;        // launches of at least this many rows run prog_stream (rows_prog)
  bool jit_write_through = false;     // its output stores are write-through (kRowsJitWriteThrough)
  int device = 0;                     // the HIP device current at create (its buffers / module live there)
  // pgm_rows_shard_run's resources on this handle's device, created on first use and kept until the
  // handle is destroyed: two streams, each with its own grow-only device chunk buffer (codes of the
  // columns the plan reads, outputs, error flag) and a pinned error word, so consecutive chunks
  // alternate between them (chunk c + 1's copy-in and pass overlap chunk c's copy-out)
  struct ShardSide {
    hipStream_t s = nullptr;
    char *buf = nullptr;
    size_t cap = 0;
    int32_t *h_err = nullptr;
  };
  ShardSide shard[2];
  std::mutex shard_mu;  // one pgm_rows_shard_run shard at a time per handle
};

// compile + load one program of the handle once; false when unavailable
static bool rows_prog_ready(RowsHandle *h, RowsHandle::Prog &pg, const char *what) {
  if (pg.src.empty()) return false;
  std::lock_guard<std::mutex> lk(h->jit_mu);
  if (pg.state != 0) return pg.state > 0;
  pg.state = -1;
  static const bool disabled = getenv("PGM_NO_JIT") != nullptr;  // testing: AOT kernels only
  if (disabled) return false;
  std::vector<char> code;
  if (!pgmi_rtc_code(pg.src, what, code)) return false;
  pg.code = code;
  if (hipModuleLoadData(&pg.mod, code.data()) != hipSuccess) {
    (void)hipGetLastError();
    pg.mod = nullptr;
    return false;
  }
  if (hipModuleGetFunction(&pg.fn, pg.mod, "pgm_rows_jit") != hipSuccess ||
      hipModuleGetFunction(&pg.fn2, pg.mod, "pgm_rows_jit2") != hipSuccess ||
      hipModuleGetFunction(&pg.fn_floor, pg.mod, "pgm_rows_floor") != hipSuccess ||
      hipModuleGetFunction(&pg.fn_floor2, pg.mod, "pgm_rows_floor2") != hipSuccess ||
      hipModuleGetFunction(&pg.fn_ring, pg.mod, "pgm_rows_ring") != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  pg.state = 1;
  return true;
}

// the specialised kernels exist for this handle; false: the AOT kernels run
static bool rows_jit_ready(RowsHandle *h) { return rows_prog_ready(h, h->prog_default, "specialised row kernel"); }

// The cache policy of the streaming program and the row count from which a launch runs it: THE rule for
// pgm_rows_plan_run / _bind (and through the bound launch the direct queues) and the ring.
// Measured on MI355X (profiles/r07stream/, DESIGN.md "cache policy of the stream"): launches of at least
// 50,000 rows store their outputs write-through AND nontemporal (sc1 nt) and load their codes as before.
//   - The outputs are never read on the device; as plain write-through lines they are allocated in the 256
//     MiB Infinity Cache and push out the evidence codes every new dispatch waits for before its first
//     store.  With `nt` the 96 x 100k-row bench window runs 2.5-2.6 -> 1.9-2.0 us of GPU span per dispatch
//     (bench value 27.5-28.3 -> 33.7-34.4 G rows/s at 20 steps, 32.4-33.7 -> 41.5-42.7 G at 50, six
//     interleaved rounds); WRITE_SIZE stays 13,281.25 KB per launch, so the stores are still write-through.
//   - Nontemporal code loads undo it (2.6-2.9 us alone, 2.6-2.7 us with the stores): they keep the codes
//     out of that cache.  sc0 sc1 nt stores measure the same as sc1 nt.  Neither is kept.
//   - From 50,000 rows: 96 batches of 50 k rows (0.69 GB) gain 1.7 -> 1.15-1.2 us; at 20 k and 10 k rows
//     (sets that fit the cache) streaming is even or 2-4 % behind, and four 100k-row launches rewriting the
//     same cached outputs lose 1.6 -> 1.9 us — the price where a set does fit.
static constexpr bool kRowsStreamLoads = false;
static constexpr int kRowsStreamStores = RowsPolicy::kStoreSc1Nt;
static constexpr int64_t kRowsStreamMinRows = 50000;
// A/B switch PGM_ROWS_STREAM, read when a plan is created: unset = the rule above; 0 = the default
// program for every launch; a policy word w in 1..5 = the streaming program for every launch, with
// nontemporal code loads if w & 1 and store form (w >> 1): 0 sc1, 1 sc1 nt, 2 sc0 sc1 nt
static RowsPolicy rows_stream_policy(int64_t *min_rows) {
  RowsPolicy pol;
  pol.nt_loads = kRowsStreamLoads;
  pol.stores = kRowsStreamStores;
  *min_rows = kRowsStreamMinRows;
  const char *e = getenv("PGM_ROWS_STREAM");
  if (e && *e) {
    const int w = atoi(e);
    if (w < 0 || w > 5) return pol;
    pol.nt_loads = (w & 1) != 0;
    pol.stores = w >> 1;
    *min_rows = w == 0 ? INT64_MAX : 0;
  }
  return pol;
}

// the program a launch of n_rows rows runs (call after rows_jit_ready(h) held); the streaming program
// computes what the default one does, so where it cannot be built the default one runs
static RowsHandle::Prog *rows_prog(RowsHandle *h, int64_t n_rows) {
  if (n_rows >= h->stream_min_rows && rows_prog_ready(h, h->prog_stream, "specialised row kernel (streaming)"))
    return &h->prog_stream;
  return &h->prog_default;
}

extern "C" {

int pgm_rows_plan_create(const pgm_rows_plan *pl, const double *host_values, void **handle) {
  STALE_PROBE();
  if (!pl || !handle || (!host_values && pl->n_values > 0)) return pgmi_failf(PGM_EINVAL, "rows_plan_create: null argument");
  *handle = nullptr;
  RowsPlan plan;
  const int st = rows_plan_compile(pl, plan);
  if (st != PGM_OK) return st;
  RowsHandle *h = new (std::nothrow) RowsHandle;
  if (!h) return pgmi_failf(PGM_ENOMEM, "rows_plan_create: host allocation");
  static_cast<RowsPlan &>(*h) = std::move(plan);
  h->jit_write_through = !h->jit_src.empty() && kRowsJitWriteThrough;
  h->prog_default.src = h->jit_src;
  const RowsPolicy pol = rows_stream_policy(&h->stream_min_rows);
  if (h->jit_src.empty() || pol.is_default()) h->stream_min_rows = INT64_MAX;  // one program
  else (void)rows_plan_source(pl, h->prog_stream.src, pol);
  (void)hipGetDevice(&h->device);
  hipError_t e = hipSuccess;
  e = hipMalloc((void **)&h->d_values, sizeof(double) * (pl->n_values + 1));
  if (e == hipSuccess && pl->n_values > 0)
    e = hipMemcpy(h->d_values, host_values, sizeof(double) * pl->n_values, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const double one = 1.0;
    e = hipMemcpy(h->d_values + pl->n_values, &one, sizeof(double), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMalloc((void **)&h->d_desc, sizeof(int32_t) * h->desc.size());
  if (e == hipSuccess)
    e = hipMemcpy(h->d_desc, h->desc.data(), sizeof(int32_t) * h->desc.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (h->d_values) (void)hipFree(h->d_values);
    if (h->d_desc) (void)hipFree(h->d_desc);
    delete h;
    return pgmi_failf(e == hipErrorOutOfMemory ? PGM_ENOMEM : PGM_EDEVICE, "rows_plan_create: %s", hipGetErrorString(e));
  }
  std::vector<int32_t>().swap(h->desc);  // the kernels read the device copy
  *handle = h;
  return PGM_OK;
}

int pgm_rows_plan_source(const pgm_rows_plan *pl, char *buf, size_t len, size_t *needed) {
  STALE_PROBE();
  std::string src;
  const int st = rows_plan_source(pl, src);
  if (st != PGM_OK) return st;
  if (needed) *needed = src.size() + 1;
  if (buf && len > 0) {
    const size_t n = std::min(len - 1, src.size());
    memcpy(buf, src.data(), n);
    buf[n] = 0;
  }
  return PGM_OK;
}

int pgm_rows_plan_stream_source(const pgm_rows_plan *pl, char *buf, size_t len, size_t *needed, int64_t *min_rows) {
  STALE_PROBE();
  int64_t from = 0;
  const RowsPolicy pol = rows_stream_policy(&from);
  std::string src;
  const int st = rows_plan_source(pl, src, pol);
  if (st != PGM_OK) return st;
  if (min_rows) *min_rows = pol.is_default() ? INT64_MAX : from;
  if (needed) *needed = src.size() + 1;
  if (buf && len > 0) {
    const size_t n = std::min(len - 1, src.size());
    memcpy(buf, src.data(), n);
    buf[n] = 0;
  }
  return PGM_OK;
}

int pgm_rows_launch_info(const pgm_rows_plan *pl, int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0,
                         int64_t n_rows, const double *marg, const double *joint, int64_t ld_out, const int32_t *map,
                         const double *gap, int32_t jit_available, pgm_rows_launch_info_t *info) {
  STALE_PROBE();
  return rows_launch_info(pl, mode, codes, ld_codes, row0, n_rows, marg, joint, ld_out, map, gap, jit_available != 0,
                          info);
}

int pgm_rows_plan_destroy(void *handle) {
  STALE_PROBE();
  RowsHandle *h = (RowsHandle *)handle;
  if (!h) return PGM_OK;
  int prev = 0;
  (void)hipGetDevice(&prev);
  if (h->shard[0].s || h->shard[1].s) (void)hipSetDevice(h->device);
  for (auto &sd : h->shard) {
    if (sd.s) (void)hipStreamSynchronize(sd.s);
    if (sd.buf) (void)hipFree(sd.buf);
    if (sd.h_err) (void)hipHostFree(sd.h_err);
    if (sd.s) (void)hipStreamDestroy(sd.s);
  }
  (void)hipSetDevice(prev);
  if (h->d_values) (void)hipFree(h->d_values);
  if (h->d_desc) (void)hipFree(h->d_desc);
  if (h->prog_default.mod) (void)hipModuleUnload(h->prog_default.mod);
  if (h->prog_stream.mod) (void)hipModuleUnload(h->prog_stream.mod);
  delete h;
  return PGM_OK;
}

}  // extern "C"

// dry: validate and size the launch only (pgm_rows_plan_bind)
static int rows_plan_run(void *handle, int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0,
                         int64_t n_rows, double *marg, double *joint, int64_t ld_out, int32_t *map, double *gap,
                         int32_t *err_flag, void *stream, bool dry) {
  RowsHandle *h = (RowsHandle *)handle;
  if (!h) return pgmi_failf(PGM_EINVAL, "rows_plan_run: null handle");
  if (n_rows <= 0) return PGM_OK;
  int st = rows_launch_check(*h, mode, codes, n_rows, marg, joint, ld_out, map, gap);
  if (st != PGM_OK) return st;
  // which kernel, with which template arguments, grid and LDS: rows_launch_choose (pgmrows_plan.cpp)
  const bool jit = rows_jit_mode(mode) && rows_jit_ready(h);
  pgm_rows_launch_info_t li;
  st = rows_launch_choose(*h, mode, codes, ld_codes, row0, n_rows, marg, ld_out, map, gap, jit, &li);
  if (st != PGM_OK) return st;
  if (dry) return PGM_OK;
  RowsK k = h->k;
  k.n_waves = k.n_comp;  // one wave per component
  hipStream_t s = S(stream);
  const double *v = h->d_values;
  const int32_t *t = h->d_desc;
  if (li.kernel == PGM_RK_JIT || li.kernel == PGM_RK_JIT2) {
    const uint8_t *cp = codes;
    int64_t ldc = ld_codes, r0 = row0, nr = n_rows, ldo = ld_out;
    double *mg = marg, *gp = gap;
    int32_t *mp = map, *ef = err_flag;
    int32_t md = mode;
    void *args[] = {(void *)&v, (void *)&cp, &ldc, &r0, &nr, (void *)&mg, &ldo, (void *)&mp, (void *)&gp, (void *)&ef, &md};
    const RowsHandle::Prog *pg = rows_prog(h, n_rows);
    HIP_TRY(hipModuleLaunchKernel(li.kernel == PGM_RK_JIT2 ? pg->fn2 : pg->fn, li.blocks, 1, 1, li.wg, 1, 1, 0, s,
                                  args, nullptr));
    return PGM_OK;
  }
  const dim3 g(li.blocks), b(li.wg);
  const size_t lds = li.lds_bytes;
  const int32_t RG = li.rg;
  if (li.kernel == PGM_RK_AFFINE) {
    if (li.values_lds)
      launch_affine<true>(li.nf, li.nt, li.map != 0, g, b, lds, s, k, v, t, codes, ld_codes, row0, n_rows, mode, RG, marg, ld_out, map, gap, err_flag);
    else
      launch_affine<false>(li.nf, li.nt, li.map != 0, g, b, lds, s, k, v, t, codes, ld_codes, row0, n_rows, mode, RG, marg, ld_out, map, gap, err_flag);
    HIP_TRY(hipGetLastError());
    return PGM_OK;
  }
  if (li.values_lds && li.acc_lds)
    launch_rows_f<true, true>(li.maxt, li.maxfc, g, b, lds, s, k, v, t, codes, ld_codes, row0, n_rows, mode, RG, marg, joint, ld_out, map, gap, err_flag);
  else if (li.values_lds)
    launch_rows_f<true, false>(li.maxt, li.maxfc, g, b, lds, s, k, v, t, codes, ld_codes, row0, n_rows, mode, RG, marg, joint, ld_out, map, gap, err_flag);
  else if (li.acc_lds)
    launch_rows_f<false, true>(li.maxt, li.maxfc, g, b, lds, s, k, v, t, codes, ld_codes, row0, n_rows, mode, RG, marg, joint, ld_out, map, gap, err_flag);
  else
    launch_rows_f<false, false>(li.maxt, li.maxfc, g, b, lds, s, k, v, t, codes, ld_codes, row0, n_rows, mode, RG, marg, joint, ld_out, map, gap, err_flag);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

extern "C" {

int pgm_rows_plan_run(void *handle, int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0, int64_t n_rows,
                      double *marg, double *joint, int64_t ld_out, int32_t *map, double *gap, int32_t *err_flag,
                      void *stream) {
  STALE_PROBE();
  return rows_plan_run(handle, mode, codes, ld_codes, row0, n_rows, marg, joint, ld_out, map, gap, err_flag, stream,
                       false);
}

// A validated, fully bound pgm_rows_plan_run (a prepared launch): repeated batches over the same
// buffers pay one argument-free call each instead of re-marshalling thirteen arguments.
struct RowsJitArgs {  // pgm_rows_jit's parameters, packed as the kernel's argument segment
  const double *V;
  const uint8_t *C;
  int64_t ldc, row0, n;
  double *M;
  int64_t ldo;
  int32_t *MP;
  double *G;
  int32_t *E;
  int32_t mode;
  int32_t pad;
};

struct RowsBound {
  // specialised kernel bound: the packed argument segment and launch shape, launched directly
  hipFunction_t fn = nullptr;
  const RowsHandle::Prog *prog = nullptr;  // the program fn belongs to (rows_prog)
  RowsJitArgs args;
  size_t args_size = sizeof(RowsJitArgs);
  unsigned blocks = 0;
  void *handle;
  int32_t mode;
  const uint8_t *codes;
  int64_t ld_codes, row0, n_rows;
  double *marg, *joint;
  int64_t ld_out;
  int32_t *map;
  double *gap;
  int32_t *err;
  void *stream;
};

int pgm_rows_plan_bind(void *handle, int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0,
                       int64_t n_rows, double *marg, double *joint, int64_t ld_out, int32_t *map, double *gap,
                       int32_t *err_flag, void *stream, void **bound) {
  STALE_PROBE();
  if (!bound) return pgmi_failf(PGM_EINVAL, "rows_plan_bind: null output pointer");
  *bound = nullptr;
  const bool floor = (mode & PGM_ROWS_FLOOR) != 0;
  mode &= ~PGM_ROWS_FLOOR;
  if (floor && (mode & (PGM_ROWS_JOINT | PGM_ROWS_GENERIC | PGM_ROWS_NO_JIT | PGM_ROWS_VALUES_GLOBAL | PGM_ROWS_ONE_GROUP)))
    return pgmi_failf(PGM_EINVAL, "rows_plan_bind: the floor kernel exists for the specialised kernel's modes only");
  const int st = rows_plan_run(handle, mode, codes, ld_codes, row0, n_rows, marg, joint, ld_out, map, gap, err_flag,
                               stream, true);
  if (st != PGM_OK) return st;
  RowsBound *b = new (std::nothrow) RowsBound;
  if (!b) return pgmi_failf(PGM_ENOMEM, "rows_plan_bind: out of host memory");
  b->handle = handle;
  b->mode = mode;
  b->codes = codes;
  b->ld_codes = ld_codes;
  b->row0 = row0;
  b->n_rows = n_rows;
  b->marg = marg;
  b->joint = joint;
  b->ld_out = ld_out;
  b->map = map;
  b->gap = gap;
  b->err = err_flag;
  b->stream = stream;
  RowsHandle *h = (RowsHandle *)handle;
  // the same choice rows_plan_run makes (the dry run above compiled the kernel if it applies)
  pgm_rows_launch_info_t li;
  if (n_rows > 0 && h->prog_default.state > 0 && rows_jit_mode(mode) &&
      rows_launch_choose(*h, mode, codes, ld_codes, row0, n_rows, marg, ld_out, map, gap, true, &li) == PGM_OK) {
    const bool two = li.kernel == PGM_RK_JIT2;
    const RowsHandle::Prog *pg = rows_prog(h, n_rows);  // the floor carries the policy of the kernel it stands for
    b->prog = pg;
    b->fn = floor ? (two ? pg->fn_floor2 : pg->fn_floor) : two ? pg->fn2 : pg->fn;
    b->args = RowsJitArgs{h->d_values, codes, ld_codes, row0, n_rows, marg, ld_out, map, gap, err_flag, mode, 0};
    b->blocks = li.blocks;
  } else if (floor) {
    delete b;
    return pgmi_failf(PGM_EINVAL, "rows_plan_bind: the floor kernel needs the plan-specialised (hipRTC) kernel");
  }
  *bound = b;
  return PGM_OK;
}

int pgm_rows_bound_run(void *bound) {
  STALE_PROBE();
  RowsBound *b = (RowsBound *)bound;
  if (!b) return pgmi_failf(PGM_EINVAL, "rows_bound_run: null handle");
  if (b->fn) {
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &b->args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &b->args_size,
                     HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(b->fn, b->blocks, 1, 1, (unsigned)jit_wg(), 1, 1, 0, S(b->stream), nullptr, extra));
    return PGM_OK;
  }
  return rows_plan_run(b->handle, b->mode, b->codes, b->ld_codes, b->row0, b->n_rows, b->marg, b->joint, b->ld_out,
                       b->map, b->gap, b->err, b->stream, false);
}

int pgm_rows_bound_kernel(void *bound, char *name, size_t cap, uint32_t *blocks, uint32_t *wg) {
  RowsBound *b = (RowsBound *)bound;
  if (!b || !name || cap == 0) return pgmi_failf(PGM_EINVAL, "rows_bound_kernel: null argument");
  const char *k = !b->fn ? "" : b->prog->name_of(b->fn);
  snprintf(name, cap, "%s", k);
  if (blocks) *blocks = b->fn ? b->blocks : 0;
  if (wg) *wg = b->fn ? (uint32_t)jit_wg() : 0;
  return PGM_OK;
}

int pgm_rows_bound_destroy(void *bound) {
  STALE_PROBE();
  delete (RowsBound *)bound;
  return PGM_OK;
}

// ---------------------------------------------------------------------------- rows sharded over GPUs
// One shard of pgm_rows_shard_run on its plan's device, on its own host thread: its rows in chunks of
// at most shard_chunk_rows(), chunk c on side c % 2 of the handle's kept resources (stream + device
// buffer): the chunk's rows of the columns the plan reads in (one copy per run of adjacent columns),
// the plan's pass, its outputs out to the caller's host arrays at the chunk's columns.  Each side's
// stream orders its own chunks, so chunk c + 2 reuses the buffer only after chunk c's copy-out; with
// pinned host arrays (pgm_host_alloc / hipHostRegister) the two sides' DMA and kernels overlap.
static constexpr int64_t shard_chunk_rows() { return 262144; }  // 256 K rows: 36 MB of marginals per chunk

static int shard_side_ready(RowsHandle::ShardSide &sd, size_t need) {
  if (!sd.s) HIP_TRY(hipStreamCreateWithFlags(&sd.s, hipStreamNonBlocking));
  if (!sd.h_err) HIP_TRY(hipHostMalloc((void **)&sd.h_err, 64, hipHostMallocDefault));
  if (sd.cap < need) {
    if (sd.buf) {
      HIP_TRY(hipStreamSynchronize(sd.s));
      (void)hipFree(sd.buf);
      sd.buf = nullptr;
      sd.cap = 0;
    }
    HIP_TRY(hipMalloc((void **)&sd.buf, need));
    sd.cap = need;
  }
  return PGM_OK;
}

static int rows_shard_one(RowsHandle *h, int32_t mode, const uint8_t *host_codes, int64_t ld_codes, int64_t r0,
                          int64_t nr, double *host_marg, int64_t ld_out, int32_t *host_map, int32_t *err_any) {
  std::lock_guard<std::mutex> lk(h->shard_mu);
  HIP_TRY(hipSetDevice(h->device));
  const int64_t chunk = std::min<int64_t>(nr, shard_chunk_rows());
  // device layout of a chunk: codes [h->n_cols][ldc] (only the plan's columns are written), marg
  // [n_marg][ldc], map [ldc], err; ldc a multiple of 16 so the two-rows-per-lane kernel takes full chunks
  const int64_t ldc = (chunk + 15) & ~(int64_t)15;
  const bool want_m = (mode & PGM_ROWS_MARGINALS) != 0, want_p = (mode & PGM_ROWS_MAP) != 0;
  const size_t b_codes = (size_t)std::max(h->n_cols, 1) * ldc;
  const size_t o_marg = (b_codes + 255) & ~(size_t)255;
  const size_t b_marg = want_m ? (size_t)h->k.n_marg * ldc * sizeof(double) : 0;
  const size_t o_map = o_marg + ((b_marg + 255) & ~(size_t)255);
  const size_t b_map = want_p ? (size_t)ldc * sizeof(int32_t) : 0;
  const size_t o_err = o_map + ((b_map + 255) & ~(size_t)255);
  const int n_sides = nr > chunk ? 2 : 1;
  for (int i = 0; i < n_sides; ++i) {
    const int st = shard_side_ready(h->shard[i], o_err + 256);
    if (st != PGM_OK) return st;
    h->shard[i].h_err[0] = 0;
    HIP_TRY(hipMemsetAsync(h->shard[i].buf + o_err, 0, sizeof(int32_t), h->shard[i].s));
  }
  // runs of adjacent plan columns: one 2-D copy each
  std::vector<std::pair<int, int>> runs;
  for (int c : h->cols) {
    if (!runs.empty() && runs.back().first + runs.back().second == c) ++runs.back().second;
    else runs.push_back({c, 1});
  }
  int st = PGM_OK;
  hipError_t e = hipSuccess;
  int64_t c = 0;
  for (int64_t a = r0; a < r0 + nr && st == PGM_OK && e == hipSuccess; a += chunk, ++c) {
    RowsHandle::ShardSide &sd = h->shard[c % n_sides];
    const int64_t m = std::min(chunk, r0 + nr - a);
    uint8_t *d_codes = (uint8_t *)sd.buf;
    double *d_marg = want_m ? (double *)(sd.buf + o_marg) : nullptr;
    int32_t *d_map = want_p ? (int32_t *)(sd.buf + o_map) : nullptr;
    int32_t *d_err = (int32_t *)(sd.buf + o_err);
    for (size_t k = 0; k < runs.size() && e == hipSuccess; ++k)
      e = hipMemcpy2DAsync(d_codes + (size_t)runs[k].first * ldc, (size_t)ldc,
                           host_codes + (size_t)runs[k].first * ld_codes + a, (size_t)ld_codes, (size_t)m,
                           (size_t)runs[k].second, hipMemcpyHostToDevice, sd.s);
    if (e != hipSuccess) break;
    st = rows_plan_run(h, mode, d_codes, ldc, 0, m, d_marg, nullptr, ldc, d_map, nullptr, d_err, sd.s, false);
    if (st == PGM_OK && want_m)
      e = hipMemcpy2DAsync(host_marg + a, (size_t)ld_out * sizeof(double), d_marg, (size_t)ldc * sizeof(double),
                           (size_t)m * sizeof(double), (size_t)h->k.n_marg, hipMemcpyDeviceToHost, sd.s);
    if (st == PGM_OK && e == hipSuccess && want_p)
      e = hipMemcpyAsync(host_map + a, d_map, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, sd.s);
  }
  int32_t h_err = 0;
  for (int i = 0; i < n_sides; ++i) {
    RowsHandle::ShardSide &sd = h->shard[i];
    if (e == hipSuccess && st == PGM_OK)
      e = hipMemcpyAsync(sd.h_err, sd.buf + o_err, sizeof(int32_t), hipMemcpyDeviceToHost, sd.s);
    const hipError_t es = hipStreamSynchronize(sd.s);
    if (e == hipSuccess) e = es;
    h_err |= sd.h_err[0];
  }
  if (st != PGM_OK) return st;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return pgmi_failf(PGM_EDEVICE, "rows_shard_run: %s", hipGetErrorString(e));
  }
  if (h_err && err_any) __atomic_fetch_or(err_any, h_err, __ATOMIC_RELAXED);
  return PGM_OK;
}

int pgm_rows_shard_run(void *const *handles, int32_t n_shards, int32_t mode, const uint8_t *host_codes,
                       int64_t ld_codes, int64_t n_cols, int64_t n_rows, double *host_marg, int64_t ld_out,
                       int32_t *host_map, int32_t *err_any) {
  STALE_PROBE();
  if (!handles || n_shards < 1) return pgmi_failf(PGM_EINVAL, "rows_shard_run: no plan handles");
  if (n_rows < 0 || ld_codes < n_rows || n_cols < 0) return pgmi_failf(PGM_EINVAL, "rows_shard_run: bad shape");
  if (mode & ~(PGM_ROWS_MARGINALS | PGM_ROWS_MAP))
    return pgmi_failf(PGM_EINVAL, "rows_shard_run: mode takes PGM_ROWS_MARGINALS | PGM_ROWS_MAP only");
  if (!(mode & (PGM_ROWS_MARGINALS | PGM_ROWS_MAP))) return pgmi_failf(PGM_EINVAL, "rows_shard_run: no output requested");
  if ((mode & PGM_ROWS_MARGINALS) && (!host_marg || ld_out < n_rows))
    return pgmi_failf(PGM_EINVAL, "rows_shard_run: marginals need host_marg with ld_out >= n_rows");
  if ((mode & PGM_ROWS_MAP) && !host_map) return pgmi_failf(PGM_EINVAL, "rows_shard_run: MAP needs host_map");
  int32_t n_marg = -1;
  for (int32_t i = 0; i < n_shards; ++i) {
    const RowsHandle *h = (const RowsHandle *)handles[i];
    if (!h) return pgmi_failf(PGM_EINVAL, "rows_shard_run: null handle %d", i);
    if (h->n_cols > n_cols) return pgmi_failf(PGM_EINVAL, "rows_shard_run: plan %d reads column %d of %lld", i, h->n_cols - 1,
                                              (long long)n_cols);
    if (n_marg >= 0 && h->k.n_marg != n_marg) return pgmi_failf(PGM_EINVAL, "rows_shard_run: plans differ (marginal rows)");
    n_marg = h->k.n_marg;
  }
  if (n_rows == 0) return PGM_OK;
  if (n_cols > 0 && !host_codes) return pgmi_failf(PGM_EINVAL, "rows_shard_run: null codes");
  int prev = 0;
  (void)hipGetDevice(&prev);
  // contiguous shards (distributed.shard_bounds): shard i = rows [i n / S, (i + 1) n / S)
  std::vector<int> st(n_shards, PGM_OK);
  std::vector<std::string> msg(n_shards);
  std::vector<std::thread> th;
  th.reserve(n_shards);
  for (int32_t i = 0; i < n_shards; ++i) {
    const int64_t a = n_rows * i / n_shards, b = n_rows * (i + 1) / n_shards;
    th.emplace_back([&, i, a, b] {
      if (b > a) {
        st[i] = rows_shard_one((RowsHandle *)handles[i], mode, host_codes, ld_codes, a, b - a, host_marg, ld_out,
                               host_map, err_any);
        if (st[i] != PGM_OK) {  // the worker's thread-local message
          char buf[512];
          (void)pgm_last_error(buf, sizeof buf);
          msg[i] = buf;
        }
      }
    });
  }
  for (auto &t : th) t.join();
  (void)hipSetDevice(prev);
  for (int32_t i = 0; i < n_shards; ++i)
    if (st[i] != PGM_OK) return pgmi_failf(st[i], "rows_shard_run: shard %d: %s", i, msg[i].c_str());
  return PGM_OK;
}

// ---------------------------------------------------------------------------- resident ring of batches
struct PgmRingSlot {  // pgm_ring_slot of the generated source (64 B)
  const uint8_t *C;
  int64_t ldc, row0;
  double *M;
  int64_t ldo;
  int32_t *MP;
  double *G;
  int64_t pad;
};
static_assert(sizeof(PgmRingSlot) == 64, "ring slot layout");

struct RowsRing {
  RowsHandle *h = nullptr;
  int32_t mode = 0;
  int64_t n_rows = 0;
  uint32_t n_slots = 0;
  PgmRingSlot *d_slots = nullptr;  // device
  unsigned *ctl = nullptr;         // pinned host: [0] batches posted, [1] cancel, [2] status (|2: timed out)
  unsigned *ctl_dev = nullptr;     // its device address
  unsigned *gctl = nullptr;        // device memory: [0] mirror of ctl[0], [1] host-poll token, [2] stop
  int32_t *err = nullptr;
  hipStream_t stream = nullptr;
  unsigned blocks = 0;
  bool running = false;
  bool reset_gctl = true;   // the device counters need zeroing before the next launch (first / after a stop)
  uint32_t n_batches = 0, posted = 0;  // this launch: batches to run, batches posted
  uint32_t base = 0;        // absolute number of batches posted over the ring's lifetime before this launch
  int wall_khz = 100000;    // the device's constant wall clock (timeout ticks)
};

int pgm_rows_ring_create(void *handle, int32_t mode, int32_t n_slots, const uint8_t *const *codes,
                         const int64_t *ld_codes, const int64_t *row0, int64_t n_rows, double *const *marg,
                         int64_t ld_out, int32_t *const *map, double *const *gap, int32_t *err_flag, void *stream,
                         void **ring) {
  STALE_PROBE();
  if (!ring) return pgmi_failf(PGM_EINVAL, "rows_ring_create: null output pointer");
  *ring = nullptr;
  RowsHandle *h = (RowsHandle *)handle;
  if (!h) return pgmi_failf(PGM_EINVAL, "rows_ring_create: null plan");
  if (n_slots < 1 || !codes || !ld_codes || !row0) return pgmi_failf(PGM_EINVAL, "rows_ring_create: no slots");
  if (n_rows < 2) return pgmi_failf(PGM_EINVAL, "rows_ring_create: n_rows %lld < 2", (long long)n_rows);
  if (mode & ~(PGM_ROWS_MARGINALS | PGM_ROWS_MAP | PGM_ROWS_MAPGAP))
    return pgmi_failf(PGM_EINVAL, "rows_ring_create: the ring runs marginals / MAP / MAP-gap outputs only");
  if (!(mode & (PGM_ROWS_MARGINALS | PGM_ROWS_MAP | PGM_ROWS_MAPGAP)))
    return pgmi_failf(PGM_EINVAL, "rows_ring_create: no output requested");
  if (!rows_jit_ready(h)) return pgmi_failf(PGM_EINVAL, "rows_ring_create: the ring needs the plan-specialised (hipRTC) kernel");
  std::vector<PgmRingSlot> slots((size_t)n_slots);
  for (int32_t i = 0; i < n_slots; ++i) {
    double *m = (mode & PGM_ROWS_MARGINALS) ? (marg ? marg[i] : nullptr) : nullptr;
    int32_t *mp = (mode & (PGM_ROWS_MAP | PGM_ROWS_MAPGAP)) && map ? map[i] : nullptr;
    double *g = (mode & PGM_ROWS_MAPGAP) && gap ? gap[i] : nullptr;
    if ((mode & PGM_ROWS_MARGINALS) && !m) return pgmi_failf(PGM_EINVAL, "rows_ring_create: slot %d has no marginal buffer", i);
    if ((mode & PGM_ROWS_MAP) && !mp) return pgmi_failf(PGM_EINVAL, "rows_ring_create: slot %d has no MAP buffer", i);
    if ((mode & PGM_ROWS_MAPGAP) && !g) return pgmi_failf(PGM_EINVAL, "rows_ring_create: slot %d has no MAP-gap buffer", i);
    if (h->max_nt > 0 && !codes[i]) return pgmi_failf(PGM_EINVAL, "rows_ring_create: slot %d has no evidence codes", i);
    if ((mode & PGM_ROWS_MARGINALS) && ld_out < n_rows)
      return pgmi_failf(PGM_EINVAL, "rows_ring_create: ld_out %lld < n_rows %lld", (long long)ld_out, (long long)n_rows);
    if (!rows2_aligned(mode, codes[i], ld_codes[i], row0[i], n_rows, m, ld_out, mp, g, h->k.n_marg))
      return pgmi_failf(PGM_EINVAL, "rows_ring_create: slot %d breaks the two-rows-per-lane contract (even rows, row0 and "
                        "leading dimensions, 16-B aligned outputs)", i);
    slots[i] = PgmRingSlot{codes[i], ld_codes[i], row0[i], m, ld_out, mp, g, 0};
  }
  RowsRing *rg = new (std::nothrow) RowsRing;
  if (!rg) return pgmi_failf(PGM_ENOMEM, "rows_ring_create: out of host memory");
  rg->h = h;
  rg->mode = mode;
  rg->n_rows = n_rows;
  rg->n_slots = (uint32_t)n_slots;
  rg->err = err_flag;
  rg->stream = S(stream);
  hipError_t e = hipMalloc((void **)&rg->d_slots, sizeof(PgmRingSlot) * slots.size());
  if (e == hipSuccess)
    e = hipMemcpy(rg->d_slots, slots.data(), sizeof(PgmRingSlot) * slots.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipHostMalloc((void **)&rg->ctl, 64, hipHostMallocCoherent | hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&rg->ctl_dev, rg->ctl, 0);
  if (e == hipSuccess) e = hipMalloc((void **)&rg->gctl, 64);
  int dev = 0, cus = 0, per_cu = 0;
  if (e == hipSuccess) e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess)
    e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rows_prog(h, n_rows)->fn_ring, ring_wg(), 0);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (rg->d_slots) (void)hipFree(rg->d_slots);
    if (rg->gctl) (void)hipFree(rg->gctl);
    if (rg->ctl) (void)hipHostFree(rg->ctl);
    delete rg;
    return pgmi_failf(e == hipErrorOutOfMemory ? PGM_ENOMEM : PGM_EDEVICE, "rows_ring_create: %s", hipGetErrorString(e));
  }
  memset(rg->ctl, 0, 64);
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0) rg->wall_khz = khz;
  (void)hipGetLastError();
  // every workgroup resident at once (one per CU at the default 1,024 threads)
  rg->blocks = (unsigned)std::max(1, cus * std::max(1, per_cu));
  *ring = rg;
  return PGM_OK;
}

static int ring_start(RowsRing *rg, uint32_t n_batches, double timeout_s, int signal);

int pgm_rows_ring_start(void *ring, uint32_t n_batches, double timeout_s) {
  STALE_PROBE();
  return ring_start((RowsRing *)ring, n_batches, timeout_s, 0);
}

int pgm_rows_ring_start_ready(void *ring, uint32_t n_batches, double timeout_s, double ready_timeout_s) {
  STALE_PROBE();
  RowsRing *rg = (RowsRing *)ring;
  if (!(ready_timeout_s > 0.0) || ready_timeout_s > 600.0)
    return pgmi_failf(PGM_EINVAL, "rows_ring_start_ready: ready timeout must be in (0, 600] s");
  if (rg) __atomic_store_n(&rg->ctl[3], 0u, __ATOMIC_SEQ_CST);
  const int st = ring_start(rg, n_batches, timeout_s, 1);
  if (st != PGM_OK || n_batches == 0) return st;
  const auto t0 = std::chrono::steady_clock::now();
  while (__atomic_load_n(&rg->ctl[3], __ATOMIC_ACQUIRE) == 0u) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > ready_timeout_s) {
      (void)pgm_rows_ring_cancel(ring);
      return pgmi_failf(PGM_EDEVICE, "rows_ring_start_ready: the resident grid did not come up within %.3g s",
                        ready_timeout_s);
    }
  }
  return PGM_OK;
}

static int ring_start(RowsRing *rg, uint32_t n_batches, double timeout_s, int signal) {
  if (!rg) return pgmi_failf(PGM_EINVAL, "rows_ring_start: null ring");
  if (rg->running) return pgmi_failf(PGM_EINVAL, "rows_ring_start: the ring is running (finish or cancel it first)");
  if (!(timeout_s > 0.0) || timeout_s > 600.0) return pgmi_failf(PGM_EINVAL, "rows_ring_start: timeout must be in (0, 600] s");
  unsigned long long ticks = (unsigned long long)(timeout_s * (double)rg->wall_khz * 1000.0);
  // ctl[0] counts batches posted over the ring's lifetime (never reset: a launch's batch b is
  // absolute batch base + b), so no device-side reset is needed between launches
  __atomic_store_n(&rg->ctl[1], 0u, __ATOMIC_SEQ_CST);
  __atomic_store_n(&rg->ctl[2], 0u, __ATOMIC_SEQ_CST);
  rg->base = __atomic_load_n(&rg->ctl[0], __ATOMIC_SEQ_CST);
  if (rg->base > 0xF0000000u) return pgmi_failf(PGM_EINVAL, "rows_ring_start: batch counter exhausted (recreate the ring)");
  rg->n_batches = n_batches;
  rg->posted = 0;
  if (n_batches == 0) return PGM_OK;
  const double *v = rg->h->d_values;
  const PgmRingSlot *d = rg->d_slots;
  unsigned ns = rg->n_slots, nb = n_batches;
  unsigned *ctl = rg->ctl_dev, *gc = rg->gctl;
  unsigned base = rg->base;
  long long n = rg->n_rows;
  int32_t *ef = rg->err;
  int32_t md = rg->mode;
  int sg = signal;
  void *args[] = {(void *)&v, (void *)&d, &ns, (void *)&ctl, (void *)&gc, &nb, &base, &n, (void *)&ef, &md, &ticks, &sg};
  if (rg->reset_gctl) {  // mirror = base, token free, stop clear, readiness count 0
    unsigned init[16] = {base, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(rg->gctl, init, sizeof init, hipMemcpyHostToDevice, rg->stream));
    HIP_TRY(hipStreamSynchronize(rg->stream));
    rg->reset_gctl = false;
  }
  HIP_TRY(hipModuleLaunchKernel(rows_prog(rg->h, rg->n_rows)->fn_ring, rg->blocks, 1, 1, (unsigned)ring_wg(), 1, 1, 0, rg->stream, args,
                                nullptr));
  rg->running = true;
  return PGM_OK;
}

int pgm_rows_ring_post(void *ring, uint32_t n_posted) {
  RowsRing *rg = (RowsRing *)ring;
  if (!rg) return pgmi_failf(PGM_EINVAL, "rows_ring_post: null ring");
  if (!rg->running) return pgmi_failf(PGM_EINVAL, "rows_ring_post: the ring is not running");
  rg->posted = std::max(rg->posted, __atomic_load_n(&rg->ctl[0], __ATOMIC_SEQ_CST) - rg->base);  // direct stores
  if (n_posted < rg->posted || n_posted > rg->n_batches)
    return pgmi_failf(PGM_EINVAL, "rows_ring_post: %u batches posted, %u started, asked for %u", rg->posted, rg->n_batches,
                      n_posted);
  rg->posted = n_posted;
  // a sequentially consistent store: drained from the store buffer before this call returns
  __atomic_store_n(&rg->ctl[0], rg->base + n_posted, __ATOMIC_SEQ_CST);
  return PGM_OK;
}

static int ring_wait(RowsRing *rg) {
  HIP_TRY(hipStreamSynchronize(rg->stream));
  rg->running = false;
  return PGM_OK;
}

int pgm_rows_ring_finish(void *ring) {
  STALE_PROBE();
  RowsRing *rg = (RowsRing *)ring;
  if (!rg) return pgmi_failf(PGM_EINVAL, "rows_ring_finish: null ring");
  if (!rg->running) return PGM_OK;
  rg->posted = std::max(rg->posted, __atomic_load_n(&rg->ctl[0], __ATOMIC_SEQ_CST) - rg->base);  // direct stores
  if (rg->posted < rg->n_batches)
    return pgmi_failf(PGM_EINVAL, "rows_ring_finish: only %u of %u batches posted (post them or cancel)", rg->posted,
                      rg->n_batches);
  const int st = ring_wait(rg);
  if (st != PGM_OK) return st;
  if (__atomic_load_n(&rg->ctl[2], __ATOMIC_SEQ_CST) & 2u) {
    rg->reset_gctl = true;
    return pgmi_failf(PGM_EDEVICE, "rows_ring_finish: the resident kernel timed out waiting for a batch");
  }
  return PGM_OK;
}

int pgm_rows_ring_cancel(void *ring) {
  STALE_PROBE();
  RowsRing *rg = (RowsRing *)ring;
  if (!rg) return pgmi_failf(PGM_EINVAL, "rows_ring_cancel: null ring");
  if (!rg->running) return PGM_OK;
  __atomic_store_n(&rg->ctl[1], 1u, __ATOMIC_SEQ_CST);
  rg->reset_gctl = true;
  return ring_wait(rg);
}

int pgm_rows_ring_counter(void *ring, uint32_t **counter, uint32_t *base) {
  RowsRing *rg = (RowsRing *)ring;
  if (!rg || !counter || !base) return pgmi_failf(PGM_EINVAL, "rows_ring_counter: null argument");
  *counter = rg->ctl;
  *base = rg->base;
  return PGM_OK;
}

int pgm_rows_ring_kernel(void *ring, char *name, size_t cap, uint32_t *blocks, uint32_t *wg) {
  RowsRing *rg = (RowsRing *)ring;
  if (!rg || !name || cap == 0) return pgmi_failf(PGM_EINVAL, "rows_ring_kernel: null argument");
  snprintf(name, cap, "%s", "pgm_rows_ring");
  if (blocks) *blocks = rg->blocks;
  if (wg) *wg = (uint32_t)ring_wg();
  return PGM_OK;
}

int pgm_rows_ring_destroy(void *ring) {
  STALE_PROBE();
  RowsRing *rg = (RowsRing *)ring;
  if (!rg) return PGM_OK;
  int st = PGM_OK;
  if (rg->running) st = pgm_rows_ring_cancel(rg);
  if (rg->d_slots) (void)hipFree(rg->d_slots);
  if (rg->gctl) (void)hipFree(rg->gctl);
  if (rg->ctl) (void)hipHostFree(rg->ctl);
  delete rg;
  return st;
}

// internal (pgm_internal.h): what the direct AQL path (pgmdq.cpp) needs to dispatch a bound
// specialised launch on its own queue; PGM_EINVAL when the bound launch is not the hipRTC kernel
int pgmi_rows_bound_jit(void *bound, pgmi_jit_launch *out) {
  RowsBound *b = (RowsBound *)bound;
  if (!b || !out) return pgmi_failf(PGM_EINVAL, "rows_bound_jit: null argument");
  if (!b->fn) return pgmi_failf(PGM_EINVAL, "direct launch needs the plan-specialised kernel (hipRTC), not an AOT kernel");
  RowsHandle *h = (RowsHandle *)b->handle;
  if (b->prog->code.empty()) return pgmi_failf(PGM_EINVAL, "direct launch: no code object kept for this plan");
  out->code = b->prog->code.data();
  out->code_size = b->prog->code.size();
  out->kernel = b->prog->name_of(b->fn);
  out->args = &b->args;
  out->args_size = b->args_size;
  out->blocks = b->blocks;
  out->wg = (unsigned)jit_wg();
  out->owner = h;
  out->write_through = h->jit_write_through ? 1 : 0;
  return PGM_OK;
}

}  // extern "C"

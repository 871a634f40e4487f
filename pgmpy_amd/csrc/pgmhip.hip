// pgmhip.hip — gfx950 (MI355X / CDNA4) primitive factor kernels + their C-ABI.
//
// Built for gfx950 only:  hipcc --offload-arch=gfx950 -O3 -fPIC -shared
// (pgmpy_amd/build.py).  Declarations and the reference call site each entry
// point replaces: include/pgmhip.h.  Design, data layout and the roofline of
// every kernel: DESIGN.md.  The fused row plan (k_rows, pgm_rows_*) is pgmrows.hip.
// The host arithmetic that decides which kernel a descriptor runs and with what
// geometry (plan_contract, plan_prodn, plan_gather, plan_contract_n, the batch job
// assembly) and the entry points that never touch the device are pgmprim_plan.cpp
// (pgm_prim.h); an entry point here calls the planner, returns its status, launches.
//
// Kernels
//   k_contract / k_contract_final  generic strided broadcast-combine + axis reduce (HBM-bound)
//   k_gather                       batched evidence reduce (gather by per-row state codes)
//   k_indicator                    0/1 evidence indicators (BP findings)
//   k_argmax                       first-index argmax per row
// also: n-ary product (+ marginal), batched small jobs, the dense pairwise step (gemm), evidence
// ingestion (codes_*), and the library's one error string (pgm_last_error, pgmi_fail / pgmi_failf)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pgmhip.h"
#include "pgm_internal.h"
#include "pgm_prim.h"
#include "pgm_hip_common.h"

using namespace pgmprim;

#define PGM_ABI_VERSION 25  // 25: pgm_rows_launch_info (host-only query of the row-plan launch: kernel family, template arguments, row groups, grid, LDS; pgm_rows_plan_run takes its choice from the same function); 24: pgm_contract_info (host-only query of the planned contraction kernel; the launcher takes its choice from the same function); 23: pgm_batch_add_contract_n (n-ary contraction jobs), pgm_dq_timer_dispatch_times, pgm_host_scan_* / pgm_host_lut_map_u8; 22: pgm_dq_bind_pm / pgm_dq_run_chain / pgm_dq_profiling; 21: pgm_batch_specialise; 20: pgm_batch_info and the grid-barrier levelled batch removed (levels: single-workgroup mode only); 19: pgm_stream_sync_spin; 18: pgm_batch_set_mode (single-workgroup levelled batch), pgm_batch_blocks; 17: pgm_rows_shard_run (rows sharded over several GPUs from host buffers); 16: pgm_rows_ring_start_ready; 15: pgm_batch_add_level / pgm_batch_info (levelled batch), pgm_memcpy_d2h_async; 14: pgm_rows_ring_* (resident ring of row batches); 13: pgm_dq_timer_dispatch_stats, pgm_rows_bound_kernel; 12: pgm_dq_launch_group, pgm_dq_timer_stop_ticks, PGM_ROWS_FLOOR; 11: pgm_product_n_marginal_bind / pgm_pm_bound_*; 10: pgm_dq_* direct AQL dispatch, pgm_codes_remap; 9: gemm lane_order, batch product_n / indicator

// ----------------------------------------------------------------------------- errors
static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// debugging aid (PGM_STALE_PROBE=1): report a pending HIP error left by an earlier call when a C-ABI
// entry point starts, so a launch check is not blamed for someone else's error
void pgmi_stale_probe(const char *fn) {
  static const bool on = getenv("PGM_STALE_PROBE") != nullptr;
  if (!on) return;
  const hipError_t e = hipPeekAtLastError();
  if (e != hipSuccess) fprintf(stderr, "pgmhip: pending HIP error at entry of %s: %s\n", fn, hipGetErrorString(e));
}

// ----------------------------------------------------------------------------- fast division
// n / d for n < 2^31 with one mul-hi and one shift (Granlund-Montgomery round-up method; make_fdiv:
// pgm_internal.h).

__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FDiv &f) {
  uint32_t t = __umulhi(n, f.m);
  return (t + n) >> f.s;
}

__device__ __forceinline__ double max_nan(double a, double b) {
  // np.max semantics: NaN propagates
  return (a > b || a != a) ? a : b;
}

// ----------------------------------------------------------------------------- contract

// ContractK (the planned flat / row-mode contraction): pgm_internal.h

template <int CMB>
__device__ __forceinline__ double combine(double a, double b) {
  if constexpr (CMB == PGM_COMBINE_MUL) return a * b;
  if constexpr (CMB == PGM_COMBINE_ADD) return a + b;
  if constexpr (CMB == PGM_COMBINE_DIV) {
    double r = a / b;
    return (r != r) ? 0.0 : r;  // DiscreteFactor.py:863 values[isnan] = 0
  }
  if constexpr (CMB == PGM_COMBINE_DIV_RAW) return a / b;
  return a;  // COPY
}

template <int RED>
__device__ __forceinline__ double red_init() {
  if constexpr (RED == PGM_RED_MAX) return -__builtin_inf();
  return 0.0;
}

template <int RED>
__device__ __forceinline__ double red_op(double acc, double v) {
  if constexpr (RED == PGM_RED_SUM) return acc + v;
  if constexpr (RED == PGM_RED_MAX) return max_nan(acc, v);
  return v;
}

// reduction-outer index -> offsets (wave-uniform when ro is)
__device__ __forceinline__ void decode_ro(const ContractK &p, uint32_t ro, int64_t &ra, int64_t &rb) {
  ra = 0;
  rb = 0;
  for (int k = p.nr - 2; k >= 0; --k) {
    const uint32_t q = fdiv(ro, p.rdiv[k]);
    const uint32_t dg = ro - q * p.rdiv[k].d;
    ra += (int64_t)dg * p.rsa[k];
    rb += (int64_t)dg * p.rsb[k];
    ro = q;
  }
}

// Flat mode: G lanes cooperate on one output (any keep layout); lanes stride the innermost
// reduction dim, the reduction-outer index is walked wave-uniformly.  `tid` / `nthreads` are the
// thread's index and the thread count of the launch (or of its job in a batched launch).
template <int CMB, int RED>
__device__ __forceinline__ void contract_flat(const ContractK &p, const double *__restrict__ A,
                                              const double *__restrict__ B, double *__restrict__ C,
                                              double *__restrict__ ws, uint64_t tid, uint64_t nthreads,
                                              uint32_t split) {
  const uint32_t G = 1u << p.g_log2;
  const uint32_t lane_g = (uint32_t)tid & (G - 1);
  const uint64_t ngroups = nthreads >> p.g_log2;
  const uint32_t r0 = split * p.red_chunk;
  const uint32_t r1 = min(p.n_ro, r0 + p.red_chunk);
  for (uint64_t out = tid >> p.g_log2; out < p.n_out; out += ngroups) {
    int64_t oa = 0, ob = 0, oc = 0;
    uint32_t idx = (uint32_t)out;
    for (int k = p.nk - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - q * p.kdiv[k].d;
      oa += (int64_t)dg * p.ksa[k];
      if constexpr (CMB != PGM_COMBINE_COPY) ob += (int64_t)dg * p.ksb[k];
      oc += (int64_t)dg * p.ksc[k];
      idx = q;
    }
    double acc = red_init<RED>();
    if (G == 1) {
      // one lane per output: the reduction entries (reduction-outer major, innermost minor — the
      // summation order of the loop below) UNR at a time, every operand load of a group issued before
      // the group is summed, so a long reduction is not one memory round trip per entry (the entry
      // walk is wave-uniform: scalar offsets and branches)
      constexpr int UNR = 8;
      const uint32_t total = (r1 > r0 ? r1 - r0 : 0u) * p.ri_card;
      uint32_t ro = r0, ri = 0;
      int64_t ra = 0, rb = 0;
      if (total) decode_ro(p, ro, ra, rb);
      for (uint32_t e = 0; e < total; e += UNR) {
        double xa[UNR], xb[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if (e + u < total) {
            xa[u] = A[oa + ra + (int64_t)ri * p.ri_sa];
            if constexpr (CMB != PGM_COMBINE_COPY) xb[u] = B[ob + rb + (int64_t)ri * p.ri_sb];
            if (++ri == p.ri_card) {
              ri = 0;
              if (++ro < r1) decode_ro(p, ro, ra, rb);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if (e + u < total) {
            if constexpr (CMB == PGM_COMBINE_COPY)
              acc = red_op<RED>(acc, xa[u]);
            else
              acc = red_op<RED>(acc, combine<CMB>(xa[u], xb[u]));
          }
        }
      }
    } else {
      // G lanes per output, each striding the innermost reduction dim from its lane; this lane's entries
      // (reduction-outer major, its innermost indices minor — the summation order of the r03 loop) are
      // walked UNR at a time with every operand load of a group issued before the group is summed (r04:
      // the r03 loop waited for each load before the next, one memory round trip per entry — C2's levels
      // with long reduction-outer walks; same order, bit-identical sums).  G <= ri_card (host plan), so
      // every lane has at least one entry per reduction-outer index.
      constexpr int UNR = 8;
      uint32_t ro = r0, ri = lane_g;
      int64_t ra = 0, rb = 0;
      bool live = ro < r1;
      if (live) decode_ro(p, ro, ra, rb);
      while (live) {
        double xa[UNR], xb[UNR];
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if (live) {
            xa[u] = A[oa + ra + (int64_t)ri * p.ri_sa];
            if constexpr (CMB != PGM_COMBINE_COPY) xb[u] = B[ob + rb + (int64_t)ri * p.ri_sb];
            cnt = u + 1;
            ri += G;
            if (ri >= p.ri_card) {
              ri = lane_g;
              if (++ro < r1) decode_ro(p, ro, ra, rb);
              else live = false;
            }
          }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if (u < cnt) {
            if constexpr (CMB == PGM_COMBINE_COPY)
              acc = red_op<RED>(acc, xa[u]);
            else
              acc = red_op<RED>(acc, combine<CMB>(xa[u], xb[u]));
          }
        }
      }
    }
    if constexpr (RED != PGM_RED_NONE) {
      for (uint32_t off = G >> 1; off > 0; off >>= 1) acc = red_op<RED>(acc, __shfl_xor(acc, (int)off, 64));
    }
    if (lane_g == 0) {
      if (p.n_split == 1)
        C[oc] = acc;
      else
        ws[(uint64_t)split * p.n_out + out] = acc;
    }
  }
}

// Flat mode over output PAIRS along the innermost kept dim, one lane per pair, 16-B accesses (batched
// BP separator marginals: rows innermost).  Host-checked (pgm_batch_add_contract): even innermost kept
// extent, output innermost stride 1, each operand's innermost kept stride 0 or 1, every other stride
// of a 16-B-read operand even, bases 16-B aligned.  Same summation order as contract_flat with G = 1.
template <int CMB, int RED>
__device__ __forceinline__ void contract_flat2(const ContractK &p, const double *__restrict__ A,
                                               const double *__restrict__ B, double *__restrict__ C, uint64_t tid,
                                               uint64_t nthreads) {
  const int kx = p.nk - 1;
  const bool va = p.ksa[kx] != 0, vb = p.ksb[kx] != 0;
  const uint32_t n_pairs = p.n_out >> 1;
  for (uint64_t q = tid; q < n_pairs; q += nthreads) {
    int64_t oa = 0, ob = 0, oc = 0;
    uint32_t idx = (uint32_t)q << 1;
    for (int k = kx; k >= 0; --k) {
      const uint32_t qq = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - qq * p.kdiv[k].d;
      oa += (int64_t)dg * p.ksa[k];
      if constexpr (CMB != PGM_COMBINE_COPY) ob += (int64_t)dg * p.ksb[k];
      oc += (int64_t)dg * p.ksc[k];
      idx = qq;
    }
    double lo = red_init<RED>(), hi = red_init<RED>();
    // the reduction entries in order (reduction-outer major), UNR at a time with every load of a group
    // issued before it is summed (see contract_flat)
    constexpr int UNR = 4;
    const uint32_t total = p.n_ro * p.ri_card;
    uint32_t ro = 0, ri = 0;
    int64_t ra = 0, rb = 0;
    if (total) decode_ro(p, ro, ra, rb);
    for (uint32_t e = 0; e < total; e += UNR) {
      double2 xa[UNR], xb[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (e + u < total) {
          const double *a = A + oa + ra + (int64_t)ri * p.ri_sa;
          if (va) {
            xa[u] = *(const double2 *)a;
          } else {
            xa[u].x = xa[u].y = *a;
          }
          if constexpr (CMB != PGM_COMBINE_COPY) {
            const double *b = B + ob + rb + (int64_t)ri * p.ri_sb;
            if (vb) {
              xb[u] = *(const double2 *)b;
            } else {
              xb[u].x = xb[u].y = *b;
            }
          }
          if (++ri == p.ri_card) {
            ri = 0;
            if (++ro < p.n_ro) decode_ro(p, ro, ra, rb);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (e + u < total) {
          double xl = xa[u].x, xh = xa[u].y;
          if constexpr (CMB != PGM_COMBINE_COPY) {
            xl = combine<CMB>(xl, xb[u].x);
            xh = combine<CMB>(xh, xb[u].y);
          }
          lo = red_op<RED>(lo, xl);
          hi = red_op<RED>(hi, xh);
        }
      }
    }
    *(double2 *)(C + oc) = make_double2(lo, hi);
  }
}

template <int CMB, int RED>
__global__ __launch_bounds__(256) void k_contract(const ContractK p, const double *__restrict__ A,
                                                  const double *__restrict__ B, double *__restrict__ C,
                                                  double *__restrict__ ws) {
  contract_flat<CMB, RED>(p, A, B, C, ws, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x,
                          (uint64_t)gridDim.x * blockDim.x, blockIdx.y);
}

// Row mode: the innermost keep dim runs across the lanes (coalesced when it is innermost in the
// operands, e.g. the evidence-row axis), the outer keep index and the reduction-outer index are
// wave-uniform (scalar decode), the innermost reduction dim is walked by increments.
template <int CMB>
__device__ __forceinline__ double ld_combine(const double *a, const double *b, int64_t ia, int64_t ib) {
  if constexpr (CMB == PGM_COMBINE_COPY)
    return a[ia];
  else
    return combine<CMB>(a[ia], b[ib]);
}

// Row mode: the innermost keep dim runs across the lanes (coalesced when it is innermost in the
// operands, e.g. the evidence-row axis), the outer keep index and the reduction-outer index are
// wave-uniform (scalar decode), the innermost reduction dim is walked by increments.  Loops are
// unrolled 4-wide with independent accumulators so each lane keeps 4-8 loads in flight.
template <int CMB, int RED>
__global__ __launch_bounds__(256) void k_contract_rows(const ContractK p, const double *__restrict__ A,
                                                       const double *__restrict__ B, double *__restrict__ C,
                                                       double *__restrict__ ws) {
  // grid: x-blocks stride the innermost keep dim, y-blocks stride the outer keep index, z = split.
  // A block decodes an outer index once (wave-uniform, scalar) and reuses it for all its rows.
  const int kx = p.nk - 1;
  const uint32_t NX = p.kdiv[kx].d;
  const int64_t sxa = p.ksa[kx], sxb = p.ksb[kx], sxc = p.ksc[kx];
  const uint32_t n_outer = p.n_out / NX;
  const uint32_t xstep = gridDim.x * blockDim.x;
  auto decode_o = [&](uint32_t idx, int64_t &oa, int64_t &ob, int64_t &oc) {
    oa = ob = oc = 0;
    for (int k = kx - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - q * p.kdiv[k].d;
      oa += (int64_t)dg * p.ksa[k];
      if constexpr (CMB != PGM_COMBINE_COPY) ob += (int64_t)dg * p.ksb[k];
      oc += (int64_t)dg * p.ksc[k];
      idx = q;
    }
  };
  if constexpr (RED == PGM_RED_NONE) {
    for (uint32_t o = blockIdx.y; o < n_outer; o += gridDim.y) {
      int64_t oa, ob, oc;
      decode_o(o, oa, ob, oc);
      uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
      for (; x + 3 * xstep < NX; x += 4 * xstep) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t xx = x + u * xstep;
          v[u] = ld_combine<CMB>(A, B, oa + xx * sxa, ob + xx * sxb);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) C[oc + (int64_t)(x + u * xstep) * sxc] = v[u];
      }
      for (; x < NX; x += xstep) C[oc + (int64_t)x * sxc] = ld_combine<CMB>(A, B, oa + (int64_t)x * sxa, ob + (int64_t)x * sxb);
    }
    return;
  }
  const uint32_t split = blockIdx.z;
  const uint32_t v0 = split * p.red_chunk;
  const uint32_t v1 = min(p.n_v, v0 + p.red_chunk);
  const uint32_t nb = p.ri_nb, CH = p.ri_chunk, RI = p.ri_card;
  for (uint32_t o = blockIdx.y; o < n_outer; o += gridDim.y) {
    int64_t oa, ob, oc;
    decode_o(o, oa, ob, oc);
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < NX; x += xstep) {
      const double *a = A + oa + (int64_t)x * sxa;
      const double *b = B + ob + (int64_t)x * sxb;
      double acc0 = red_init<RED>(), acc1 = acc0, acc2 = acc0, acc3 = acc0;
      for (uint32_t v = v0; v < v1; ++v) {
        const uint32_t ro = nb == 1 ? v : v / nb;
        const uint32_t bk = v - ro * nb;
        int64_t ra, rb;
        decode_ro(p, ro, ra, rb);
        const uint32_t ri1 = min(RI, (bk + 1) * CH);
        uint32_t ri = bk * CH;
        for (; ri + 4 <= ri1; ri += 4) {
          const double w0 = ld_combine<CMB>(a, b, ra + (int64_t)ri * p.ri_sa, rb + (int64_t)ri * p.ri_sb);
          const double w1 = ld_combine<CMB>(a, b, ra + (int64_t)(ri + 1) * p.ri_sa, rb + (int64_t)(ri + 1) * p.ri_sb);
          const double w2 = ld_combine<CMB>(a, b, ra + (int64_t)(ri + 2) * p.ri_sa, rb + (int64_t)(ri + 2) * p.ri_sb);
          const double w3 = ld_combine<CMB>(a, b, ra + (int64_t)(ri + 3) * p.ri_sa, rb + (int64_t)(ri + 3) * p.ri_sb);
          acc0 = red_op<RED>(acc0, w0);
          acc1 = red_op<RED>(acc1, w1);
          acc2 = red_op<RED>(acc2, w2);
          acc3 = red_op<RED>(acc3, w3);
        }
        for (; ri < ri1; ++ri) acc0 = red_op<RED>(acc0, ld_combine<CMB>(a, b, ra + (int64_t)ri * p.ri_sa, rb + (int64_t)ri * p.ri_sb));
      }
      const double acc = red_op<RED>(red_op<RED>(acc0, acc1), red_op<RED>(acc2, acc3));
      if (p.n_split == 1)
        C[oc + (int64_t)x * sxc] = acc;
      else
        ws[(uint64_t)split * p.n_out + (uint64_t)o * NX + x] = acc;
    }
  }
}

// Row mode, short reduction (n_red <= 512, no split): every reduction offset is decoded once per
// block into LDS, then each row sums flat over them with 8 loads and 8 accumulators in flight
// (a BP separator marginal: a few clique variables summed for every (separator state, row)).
// (RTAB_MAX: pgm_prim.h)
template <int CMB, int RED>
__global__ __launch_bounds__(256) void k_contract_rows_tab(const ContractK p, const double *__restrict__ A,
                                                           const double *__restrict__ B, double *__restrict__ C) {
  __shared__ int64_t sra[RTAB_MAX], srb[RTAB_MAX];
  const uint32_t NR = p.n_red;
  for (uint32_t j = threadIdx.x; j < NR; j += blockDim.x) {
    const uint32_t ro = j / p.ri_card, ri = j - ro * p.ri_card;
    int64_t ra, rb;
    decode_ro(p, ro, ra, rb);
    sra[j] = ra + (int64_t)ri * p.ri_sa;
    srb[j] = rb + (int64_t)ri * p.ri_sb;
  }
  __syncthreads();
  const int kx = p.nk - 1;
  const uint32_t NX = p.kdiv[kx].d;
  const int64_t sxa = p.ksa[kx], sxb = p.ksb[kx], sxc = p.ksc[kx];
  const uint32_t n_outer = p.n_out / NX;
  const uint32_t xstep = gridDim.x * blockDim.x;
  for (uint32_t o = blockIdx.y; o < n_outer; o += gridDim.y) {
    int64_t oa = 0, ob = 0, oc = 0;
    uint32_t idx = o;
    for (int k = kx - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - q * p.kdiv[k].d;
      oa += (int64_t)dg * p.ksa[k];
      if constexpr (CMB != PGM_COMBINE_COPY) ob += (int64_t)dg * p.ksb[k];
      oc += (int64_t)dg * p.ksc[k];
      idx = q;
    }
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < NX; x += xstep) {
      const double *a = A + oa + (int64_t)x * sxa;
      const double *b = B + ob + (int64_t)x * sxb;
      double acc[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = red_init<RED>();
      uint32_t j = 0;
      for (; j + 8 <= NR; j += 8) {
        double w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = ld_combine<CMB>(a, b, sra[j + u], srb[j + u]);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = red_op<RED>(acc[u], w[u]);
      }
      for (; j < NR; ++j) acc[0] = red_op<RED>(acc[0], ld_combine<CMB>(a, b, sra[j], srb[j]));
#pragma unroll
      for (int u = 1; u < 8; ++u) acc[0] = red_op<RED>(acc[0], acc[u]);
      C[oc + (int64_t)x * sxc] = acc[0];
    }
  }
}

// k_contract_rows_tab for a plain marginal (COPY), two rows per lane with 16-B loads/stores.
// Host-checked: even row count, row stride 1 in A and C, every other A/C stride even, bases 16-B aligned.
template <int RED>
__global__ __launch_bounds__(256) void k_contract_rows_tab2(const ContractK p, const double *__restrict__ A,
                                                            double *__restrict__ C) {
  __shared__ int64_t sra[RTAB_MAX];
  const uint32_t NR = p.n_red;
  for (uint32_t j = threadIdx.x; j < NR; j += blockDim.x) {
    const uint32_t ro = j / p.ri_card, ri = j - ro * p.ri_card;
    int64_t ra, rb;
    decode_ro(p, ro, ra, rb);
    sra[j] = (ra + (int64_t)ri * p.ri_sa) >> 1;  // in double2 units
  }
  __syncthreads();
  const int kx = p.nk - 1;
  const uint32_t NP = p.kdiv[kx].d >> 1;
  const uint32_t n_outer = p.n_out / p.kdiv[kx].d;
  const uint32_t xstep = gridDim.x * blockDim.x;
  for (uint32_t o = blockIdx.y; o < n_outer; o += gridDim.y) {
    int64_t oa = 0, oc = 0;
    uint32_t idx = o;
    for (int k = kx - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - q * p.kdiv[k].d;
      oa += (int64_t)dg * p.ksa[k];
      oc += (int64_t)dg * p.ksc[k];
      idx = q;
    }
    const double2 *a2 = (const double2 *)(A + oa);
    double2 *c2 = (double2 *)(C + oc);
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < NP; x += xstep) {
      const double2 *a = a2 + x;
      double2 acc[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] = make_double2(red_init<RED>(), red_init<RED>());
      uint32_t j = 0;
      for (; j + 8 <= NR; j += 8) {
        double2 w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = a[sra[j + u]];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          acc[u].x = red_op<RED>(acc[u].x, w[u].x);
          acc[u].y = red_op<RED>(acc[u].y, w[u].y);
        }
      }
      for (; j < NR; ++j) {
        const double2 w = a[sra[j]];
        acc[0].x = red_op<RED>(acc[0].x, w.x);
        acc[0].y = red_op<RED>(acc[0].y, w.y);
      }
#pragma unroll
      for (int u = 1; u < 8; ++u) {
        acc[0].x = red_op<RED>(acc[0].x, acc[u].x);
        acc[0].y = red_op<RED>(acc[0].y, acc[u].y);
      }
      c2[x] = acc[0];
    }
  }
}

template <int RED>
__global__ __launch_bounds__(256) void k_contract_final(const ContractK p, const double *__restrict__ ws,
                                                        double *__restrict__ C) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t out = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; out < p.n_out; out += stride) {
    int64_t oc = 0;
    uint32_t idx = (uint32_t)out;
    for (int k = p.nk - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      oc += (int64_t)(idx - q * p.kdiv[k].d) * p.ksc[k];
      idx = q;
    }
    double acc = ws[out];
    for (int s = 1; s < p.n_split; ++s) acc = red_op<RED>(acc, ws[(uint64_t)s * p.n_out + out]);
    C[oc] = acc;
  }
}

// the plan of a contraction (plan_contract) and the kernel it runs (contract_kernel): pgmprim_plan.cpp

template <int CMB, int RED>
static void launch_contract_t(const ContractLaunch &L, const double *A, const double *B, double *C, double *ws,
                              hipStream_t s) {
  uint32_t grid[3];
  const int kernel = contract_kernel(L, CMB, RED, A, C, grid);
  const dim3 g(grid[0], grid[1], grid[2]);
  switch (kernel) {
    case PGM_CK_ROWS_TAB2: hipLaunchKernelGGL((k_contract_rows_tab2<RED>), g, dim3(256), 0, s, L.k, A, C); break;
    case PGM_CK_ROWS_TAB: hipLaunchKernelGGL((k_contract_rows_tab<CMB, RED>), g, dim3(256), 0, s, L.k, A, B, C); break;
    case PGM_CK_ROWS: hipLaunchKernelGGL((k_contract_rows<CMB, RED>), g, dim3(256), 0, s, L.k, A, B, C, ws); break;
    default: hipLaunchKernelGGL((k_contract<CMB, RED>), g, dim3(256), 0, s, L.k, A, B, C, ws); break;
  }
  if (L.k.n_split > 1) {
    uint64_t blocks = std::min<uint64_t>((L.k.n_out + 255) / 256, 65535);
    hipLaunchKernelGGL((k_contract_final<RED>), dim3((unsigned)std::max<uint64_t>(blocks, 1)), dim3(256), 0, s,
                       L.k, (const double *)ws, C);
  }
}

template <int CMB>
static void launch_contract_c(int red, const ContractLaunch &L, const double *A, const double *B, double *C,
                              double *ws, hipStream_t s) {
  switch (red) {
    case PGM_RED_NONE: launch_contract_t<CMB, PGM_RED_NONE>(L, A, B, C, ws, s); break;
    case PGM_RED_SUM: launch_contract_t<CMB, PGM_RED_SUM>(L, A, B, C, ws, s); break;
    default: launch_contract_t<CMB, PGM_RED_MAX>(L, A, B, C, ws, s); break;
  }
}

// ----------------------------------------------------------------------------- n-ary product
// ProdNK (a planned n-ary product): pgm_prim.h

// all operand values first (unused slots alias operand 0 with stride 0, so every load is valid and
// no load sits behind a branch), then the product with the per-operand kinds (uniform branches)
template <int NOPS>
__device__ __forceinline__ double prodn_combine(const ProdNK &p, const double (&v)[NOPS]) {
  double prod = 1.0;
#pragma unroll
  for (int i = 0; i < NOPS; ++i) {
    if (i < p.n_ops) {
      if (p.kind[i] == PGM_PRODN_MUL) {
        prod *= v[i];
      } else if (p.kind[i] == PGM_PRODN_RATIO && i + 1 < NOPS) {
        const double r = v[i] / v[i + 1];
        prod *= (r != r) ? 0.0 : r;
      }
    }
  }
  return prod;
}

// flat mode: every output decoded on its own (grid-stride over tid / nthreads); also the body of a
// batched product_n job (k_batch)
template <int NOPS>
__device__ __forceinline__ void prodn_flat(const ProdNK &p, double *__restrict__ C, uint64_t tid, uint64_t nthreads) {
  for (uint64_t out = tid; out < p.n_out; out += nthreads) {
    uint32_t idx = (uint32_t)out;
    int64_t off[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) off[i] = 0;
    int64_t oc = 0;
    for (int k = p.nk - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - q * p.kdiv[k].d;
#pragma unroll
      for (int i = 0; i < NOPS; ++i) off[i] += (int64_t)dg * p.ks[i][k];
      oc += (int64_t)dg * p.ksc[k];
      idx = q;
    }
    double v[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) v[i] = p.ops[i][off[i]];
    C[oc] = prodn_combine<NOPS>(p, v);
  }
}

// flat mode over element PAIRS along the innermost dim (host-checked: even innermost card, output
// innermost stride 1, every operand's innermost stride 0 or 1, all other strides of 16-B accessed
// arrays even, bases 16-B aligned): 16-B loads/stores for batched jobs
template <int NOPS>
__device__ __forceinline__ void prodn_flat2(const ProdNK &p, double *__restrict__ C, uint64_t tid, uint64_t nthreads) {
  const int kx = p.nk - 1;
  bool vec[NOPS];
#pragma unroll
  for (int i = 0; i < NOPS; ++i) vec[i] = p.ks[i][kx] != 0;
  const uint32_t n_pairs = p.n_out >> 1;
  for (uint64_t q = tid; q < n_pairs; q += nthreads) {
    uint32_t idx = (uint32_t)q << 1;
    int64_t off[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) off[i] = 0;
    int64_t oc = 0;
    for (int k = kx; k >= 0; --k) {
      const uint32_t qq = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - qq * p.kdiv[k].d;
#pragma unroll
      for (int i = 0; i < NOPS; ++i) off[i] += (int64_t)dg * p.ks[i][k];
      oc += (int64_t)dg * p.ksc[k];
      idx = qq;
    }
    double lo[NOPS], hi[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) {
      if (vec[i]) {
        const double2 w = *(const double2 *)(p.ops[i] + off[i]);
        lo[i] = w.x;
        hi[i] = w.y;
      } else {
        lo[i] = hi[i] = p.ops[i][off[i]];
      }
    }
    *(double2 *)(C + oc) = make_double2(prodn_combine<NOPS>(p, lo), prodn_combine<NOPS>(p, hi));
  }
}

template <int NOPS>
__global__ __launch_bounds__(256) void k_productn(const ProdNK p, double *__restrict__ C) {
  if (p.row_mode) {
    constexpr int U = NOPS <= 4 ? 4 : 2;  // rows in flight per thread
    const int kx = p.nk - 1;
    const uint32_t NX = p.kdiv[kx].d;
    const uint32_t n_outer = p.n_out / NX;
    const uint32_t xstep = gridDim.x * blockDim.x;
    int64_t sx[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) sx[i] = p.ks[i][kx];
    const int64_t scx = p.ksc[kx];
    for (uint32_t o = blockIdx.y; o < n_outer; o += gridDim.y) {
      // outer decode once per block and outer index (wave-uniform), reused for all rows
      int64_t off[NOPS];
#pragma unroll
      for (int i = 0; i < NOPS; ++i) off[i] = 0;
      int64_t oc = 0;
      uint32_t idx = o;
      for (int k = kx - 1; k >= 0; --k) {
        const uint32_t q = fdiv(idx, p.kdiv[k]);
        const uint32_t dg = idx - q * p.kdiv[k].d;
#pragma unroll
        for (int i = 0; i < NOPS; ++i) off[i] += (int64_t)dg * p.ks[i][k];
        oc += (int64_t)dg * p.ksc[k];
        idx = q;
      }
      const double *op[NOPS];
#pragma unroll
      for (int i = 0; i < NOPS; ++i) op[i] = p.ops[i] + off[i];
      for (uint32_t x0 = blockIdx.x * blockDim.x + threadIdx.x; x0 < NX; x0 += U * xstep) {
        double v[U][NOPS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t x = x0 + u * xstep;
          const int64_t xc = x < NX ? x : NX - 1;
#pragma unroll
          for (int i = 0; i < NOPS; ++i) v[u][i] = op[i][xc * sx[i]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t x = x0 + u * xstep;
          if (x < NX) C[oc + (int64_t)x * scx] = prodn_combine<NOPS>(p, v[u]);
        }
      }
    }
    return;
  }
  prodn_flat<NOPS>(p, C, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
}

// Row mode, two rows per lane (16-B loads/stores; the 8-B form runs at 0.54-0.70x the 16-B rate on
// gfx950).  Host-checked: even row count, output row stride 1, every operand's row stride 0 (broadcast,
// one scalar per outer index) or 1, every base 16-B aligned (all outer strides even).
template <int NOPS>
__global__ __launch_bounds__(256) void k_productn_rows2(const ProdNK p, double *__restrict__ C) {
  constexpr int U = NOPS <= 4 ? 2 : 1;  // row pairs in flight per thread
  const int kx = p.nk - 1;
  const uint32_t NP = p.kdiv[kx].d >> 1;
  const uint32_t n_outer = p.n_out / p.kdiv[kx].d;
  const uint32_t xstep = gridDim.x * blockDim.x;
  bool vec[NOPS];
#pragma unroll
  for (int i = 0; i < NOPS; ++i) vec[i] = p.ks[i][kx] != 0;
  for (uint32_t o = blockIdx.y; o < n_outer; o += gridDim.y) {
    int64_t off[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) off[i] = 0;
    int64_t oc = 0;
    uint32_t idx = o;
    for (int k = kx - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - q * p.kdiv[k].d;
#pragma unroll
      for (int i = 0; i < NOPS; ++i) off[i] += (int64_t)dg * p.ks[i][k];
      oc += (int64_t)dg * p.ksc[k];
      idx = q;
    }
    const double *op[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) op[i] = p.ops[i] + off[i];
    double2 *c2 = (double2 *)(C + oc);
    for (uint32_t x0 = blockIdx.x * blockDim.x + threadIdx.x; x0 < NP; x0 += U * xstep) {
      double2 v[U][NOPS];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t x = x0 + u * xstep;
        const uint32_t xc = x < NP ? x : NP - 1;
#pragma unroll
        for (int i = 0; i < NOPS; ++i) {
          if (vec[i]) {
            v[u][i] = ((const double2 *)op[i])[xc];
          } else {
            const double b = op[i][0];
            v[u][i] = make_double2(b, b);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t x = x0 + u * xstep;
        double lo[NOPS], hi[NOPS];
#pragma unroll
        for (int i = 0; i < NOPS; ++i) {
          lo[i] = v[u][i].x;
          hi[i] = v[u][i].y;
        }
        if (x < NP) c2[x] = make_double2(prodn_combine<NOPS>(p, lo), prodn_combine<NOPS>(p, hi));
      }
    }
  }
}

// ----------------------------------------------------------------------------- n-ary product + marginal
// C = prod_i X_i (as pgm_product_n) and, in the same pass, M = SUM/MAX of C over the keep dims M
// does not have: a batched-BP clique belief written together with its separator message (collect)
// or updated in place together with the marginal onto its children's separator (distribute), so
// the belief is not read again.  Rows (the last keep dim) two per lane with 16-B accesses as in
// k_productn_rows2.  A block owns one kept outer index (separator state); the reduction (the
// clique's other states) is walked from an LDS offset table with the next entry's operands in
// flight while the current product is stored and accumulated.

template <int NOPS>
__device__ __forceinline__ double prodm_combine(const ProdMK &p, const double (&v)[NOPS]) {
  double prod = 1.0;
#pragma unroll
  for (int i = 0; i < NOPS; ++i) {
    if (i < p.n_ops) {
      if (p.kind[i] == PGM_PRODN_MUL) {
        prod *= v[i];
      } else if (p.kind[i] == PGM_PRODN_RATIO && i + 1 < NOPS) {
        const double r = v[i] / v[i + 1];
        prod *= (r != r) ? 0.0 : r;
      }
    }
  }
  return prod;
}


// j-outer form: for each reduced entry j the block sweeps its x range (XI row pairs per lane,
// x = x0 + i*256), so every store instruction of the block lands in one contiguous run of the
// belief and XI x NOPS 16-B operand loads are in flight per lane; the marginal stays in XI
// register accumulators until the last j.  Block = (kept outer index, 256*XI row pairs).
template <int NOPS, int RED, int XI>
__global__ __launch_bounds__(256) void k_productn_marg_jx(const ProdMK p, double *C, double *__restrict__ M) {
  __shared__ int64_t tc[RMAX_MARG];
  __shared__ int64_t to[NOPS][RMAX_MARG];
  const uint32_t NR = p.n_red;
  for (uint32_t j = threadIdx.x; j < NR; j += blockDim.x) {
    uint32_t idx = j;
    int64_t oc = 0, oo[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) oo[i] = 0;
    for (int k = p.nr - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.rdiv[k]);
      const uint32_t dg = idx - q * p.rdiv[k].d;
      oc += (int64_t)dg * p.rsc[k];
#pragma unroll
      for (int i = 0; i < NOPS; ++i) oo[i] += (int64_t)dg * p.rs[i][k];
      idx = q;
    }
    tc[j] = oc;
#pragma unroll
    for (int i = 0; i < NOPS; ++i) to[i][j] = oo[i];
  }
  __syncthreads();
  const int kx = p.nk - 1;
  for (uint32_t o = blockIdx.y; o < p.n_outer; o += gridDim.y) {
    int64_t oc = 0, om = 0, off[NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) off[i] = 0;
    uint32_t idx = o;
    for (int k = kx - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - q * p.kdiv[k].d;
      oc += (int64_t)dg * p.ksc[k];
      om += (int64_t)dg * p.ksm[k];
#pragma unroll
      for (int i = 0; i < NOPS; ++i) off[i] += (int64_t)dg * p.ks[i][k];
      idx = q;
    }
    const uint32_t x0 = blockIdx.x * (256u * XI) + threadIdx.x;
    uint32_t xs[XI];
#pragma unroll
    for (int u = 0; u < XI; ++u) {
      const uint32_t x = x0 + 256u * u;
      xs[u] = x < p.NP ? x : p.NP - 1;
    }
    double2 acc[XI];
#pragma unroll
    for (int u = 0; u < XI; ++u) acc[u] = make_double2(red_init<RED>(), red_init<RED>());
    // operands that do not vary over the reduced entries: loaded once per outer index
    double2 h[XI][NOPS];
#pragma unroll
    for (int i = 0; i < NOPS; ++i) {
      if (p.jvar[i]) continue;
      const double *b = p.ops[i] + off[i];
      if (p.vec[i]) {
#pragma unroll
        for (int u = 0; u < XI; ++u) h[u][i] = ((const double2 *)b)[xs[u]];
      } else {
        const double sv = b[0];
#pragma unroll
        for (int u = 0; u < XI; ++u) h[u][i] = make_double2(sv, sv);
      }
    }
    for (uint32_t j = 0; j < NR; ++j) {
      double2 v[XI][NOPS];
#pragma unroll
      for (int i = 0; i < NOPS; ++i) {
        const double *b = p.ops[i] + off[i] + to[i][j];
        if (!p.jvar[i]) {
#pragma unroll
          for (int u = 0; u < XI; ++u) v[u][i] = h[u][i];
        } else if (p.vec[i]) {
#pragma unroll
          for (int u = 0; u < XI; ++u) v[u][i] = ((const double2 *)b)[xs[u]];
        } else {
          const double sv = b[0];
#pragma unroll
          for (int u = 0; u < XI; ++u) v[u][i] = make_double2(sv, sv);
        }
      }
      double2 *cj = (double2 *)(C + oc + tc[j]);
#pragma unroll
      for (int u = 0; u < XI; ++u) {
        double lo[NOPS], hi[NOPS];
#pragma unroll
        for (int i = 0; i < NOPS; ++i) {
          lo[i] = v[u][i].x;
          hi[i] = v[u][i].y;
        }
        const double2 pr = make_double2(prodm_combine<NOPS>(p, lo), prodm_combine<NOPS>(p, hi));
        if (C && x0 + 256u * u < p.NP) cj[x0 + 256u * u] = pr;  // C == nullptr: the marginal only
        acc[u].x = red_op<RED>(acc[u].x, pr.x);
        acc[u].y = red_op<RED>(acc[u].y, pr.y);
      }
    }
#pragma unroll
    for (int u = 0; u < XI; ++u) {
      if (p.mdiv >= 0) {  // the marginal over the operand that does not vary over the summed entries
        double2 dv = h[u][0];
#pragma unroll
        for (int i = 1; i < NOPS; ++i)
          if (i == p.mdiv) dv = h[u][i];
        const double rx = acc[u].x / dv.x, ry = acc[u].y / dv.y;
        acc[u] = make_double2(rx != rx ? 0.0 : rx, ry != ry ? 0.0 : ry);
      }
      if (x0 + 256u * u < p.NP) ((double2 *)(M + om))[x0 + 256u * u] = acc[u];
    }
  }
}

// its plan: pgmi_plan_product_marg (pgmpm_gen.cpp)

// ----------------------------------------------------------------------------- gather
// GatherK (a planned per-row evidence gather): pgm_internal.h

__device__ __forceinline__ void gather_body(const GatherK &p, const double *__restrict__ A,
                                            const uint8_t *__restrict__ codes, double *__restrict__ C,
                                            int32_t *__restrict__ err, uint64_t tid, uint64_t nthreads) {
  for (uint64_t out = tid; out < p.n_out; out += nthreads) {
    int64_t oa = 0, oc = 0, row = 0;
    uint32_t idx = (uint32_t)out;
    for (int k = p.nk - 1; k >= 0; --k) {
      const uint32_t q = fdiv(idx, p.kdiv[k]);
      const uint32_t dg = idx - q * p.kdiv[k].d;
      oa += (int64_t)dg * p.ksa[k];
      oc += (int64_t)dg * p.ksc[k];
      if (k == p.batch_dim) row = dg;
      idx = q;
    }
    for (int j = 0; j < p.n_ev; ++j) {
      uint32_t c = codes[p.ev_col[j] * p.ld + p.row0 + row];
      if (c >= (uint32_t)p.ev_card[j]) {
        if (err) atomicOr(err, 1);
        c = 0;
      }
      oa += (int64_t)c * p.ev_stride[j];
    }
    C[oc] = A[oa];
  }
}

__global__ __launch_bounds__(256) void k_gather(const GatherK p, const double *__restrict__ A,
                                                const uint8_t *__restrict__ codes, double *__restrict__ C,
                                                int32_t *__restrict__ err) {
  gather_body(p, A, codes, C, err, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
}

// findings as 0/1 indicators (BP): out[k, r] = (codes[r] == k), 1 for a missing code (PGM_EV_MISSING)
__device__ __forceinline__ void indicator_body(const uint8_t *__restrict__ codes, int64_t n_rows, int64_t card,
                                               double *__restrict__ out, int64_t s_state, int64_t s_row,
                                               int32_t *__restrict__ err, int64_t tid, int64_t stride) {
  const int64_t n = n_rows * card;
  for (int64_t i = tid; i < n; i += stride) {
    const int64_t r = i % n_rows, k = i / n_rows;
    const uint32_t c = codes[r];
    double v;
    if (c == PGM_EV_MISSING)
      v = 1.0;
    else {
      if (c >= (uint64_t)card && err) atomicOr(err, 1);
      v = (c == (uint64_t)k) ? 1.0 : 0.0;
    }
    out[k * s_state + r * s_row] = v;
  }
}

// ----------------------------------------------------------------------------- batched small jobs
// Many independent small contractions / evidence gathers in ONE launch: workgroup -> job through a
// block map, each job runs the flat-mode contraction (or the gather) over its own blocks.  One
// level of a compiled contraction path (all steps whose inputs are ready) is one launch instead
// of one launch per step.
// BatchJob: pgm_prim.h

template <int CMB>
__device__ __forceinline__ void batch_contract_c(const BatchJob &J, uint64_t tid, uint64_t n) {
  if (J.c.row_mode == 2) {  // output pairs, 16-B accesses
    switch (J.red) {
      case PGM_RED_NONE: contract_flat2<CMB, PGM_RED_NONE>(J.c, J.A, J.B, J.C, tid, n); break;
      case PGM_RED_SUM: contract_flat2<CMB, PGM_RED_SUM>(J.c, J.A, J.B, J.C, tid, n); break;
      default: contract_flat2<CMB, PGM_RED_MAX>(J.c, J.A, J.B, J.C, tid, n); break;
    }
    return;
  }
  switch (J.red) {
    case PGM_RED_NONE: contract_flat<CMB, PGM_RED_NONE>(J.c, J.A, J.B, J.C, nullptr, tid, n, 0); break;
    case PGM_RED_SUM: contract_flat<CMB, PGM_RED_SUM>(J.c, J.A, J.B, J.C, nullptr, tid, n, 0); break;
    default: contract_flat<CMB, PGM_RED_MAX>(J.c, J.A, J.B, J.C, nullptr, tid, n, 0); break;
  }
}

__device__ __forceinline__ void batch_block(const BatchJob *__restrict__ jobs, const uint32_t *__restrict__ block_job,
                                            uint32_t b);

__global__ __launch_bounds__(256) void k_batch(const BatchJob *__restrict__ jobs,
                                               const uint32_t *__restrict__ block_job) {
  batch_block(jobs, block_job, blockIdx.x);
}

// ChainJob (a job of a single-workgroup levelled batch of contractions, staged in LDS): pgm_prim.h

template <int CMB>
__device__ __forceinline__ void chain_contract_c(const ChainJob &J, uint64_t tid, uint64_t n) {
  if (J.c.row_mode == 2) {
    switch (J.red) {
      case PGM_RED_NONE: contract_flat2<CMB, PGM_RED_NONE>(J.c, J.A, J.B, J.C, tid, n); break;
      case PGM_RED_SUM: contract_flat2<CMB, PGM_RED_SUM>(J.c, J.A, J.B, J.C, tid, n); break;
      default: contract_flat2<CMB, PGM_RED_MAX>(J.c, J.A, J.B, J.C, tid, n); break;
    }
    return;
  }
  switch (J.red) {
    case PGM_RED_NONE: contract_flat<CMB, PGM_RED_NONE>(J.c, J.A, J.B, J.C, nullptr, tid, n, 0); break;
    case PGM_RED_SUM: contract_flat<CMB, PGM_RED_SUM>(J.c, J.A, J.B, J.C, nullptr, tid, n, 0); break;
    default: contract_flat<CMB, PGM_RED_MAX>(J.c, J.A, J.B, J.C, nullptr, tid, n, 0); break;
  }
}

// 1,024 threads = kChainVB virtual 256-thread blocks: a level's blocks run kChainVB at a time (each
// virtual block's 4 waves as one block of k_batch), one workgroup barrier per level.
static constexpr uint32_t kChainVB = 4;

__global__ __launch_bounds__(256 * kChainVB) void k_batch_wg_c(const ChainJob *__restrict__ jobs,
                                                    const uint32_t *__restrict__ block_job,
                                                    const uint32_t *__restrict__ level_off, uint32_t n_levels,
                                                    uint32_t n_jobs, uint32_t n_blocks) {
  extern __shared__ uint4 chain_lds[];
  const uint32_t jq = n_jobs * (uint32_t)(sizeof(ChainJob) / 16);
  const uint4 *src = reinterpret_cast<const uint4 *>(jobs);
  for (uint32_t i = threadIdx.x; i < jq; i += blockDim.x) chain_lds[i] = src[i];  // all loads independent
  uint32_t *lmap = reinterpret_cast<uint32_t *>(chain_lds + jq);
  for (uint32_t i = threadIdx.x; i < n_blocks; i += blockDim.x) lmap[i] = block_job[i];
  uint32_t *llev = lmap + n_blocks;
  for (uint32_t i = threadIdx.x; i <= n_levels; i += blockDim.x) llev[i] = level_off[i];
  __syncthreads();
  const ChainJob *sj = reinterpret_cast<const ChainJob *>(chain_lds);
  const uint32_t vb = threadIdx.x / 256, lt = threadIdx.x % 256;
  for (uint32_t l = 0; l < n_levels; ++l) {
    const uint32_t e = llev[l + 1];
    for (uint32_t b = llev[l] + vb; b < e; b += kChainVB) {
      const ChainJob &J = sj[lmap[b]];
      const uint64_t tid = (uint64_t)(b - J.block0) * 256 + lt;
      const uint64_t n = (uint64_t)J.nblocks * 256;
      switch (J.cmb) {
        case PGM_COMBINE_MUL: chain_contract_c<PGM_COMBINE_MUL>(J, tid, n); break;
        case PGM_COMBINE_ADD: chain_contract_c<PGM_COMBINE_ADD>(J, tid, n); break;
        case PGM_COMBINE_DIV: chain_contract_c<PGM_COMBINE_DIV>(J, tid, n); break;
        case PGM_COMBINE_DIV_RAW: chain_contract_c<PGM_COMBINE_DIV_RAW>(J, tid, n); break;
        default: chain_contract_c<PGM_COMBINE_COPY>(J, tid, n); break;
      }
    }
    __syncthreads();  // the level's outputs are complete before the next level reads them
  }
}

// A batch whose jobs are all contractions with one (combine, reduce) pair — every C2 / C1 path level —
// runs this instead of k_batch: k_batch carries every job kind's code (167 KB of instructions, 123
// VGPRs), this one only the two contraction bodies.  Same per-job code, so bit-identical results
// (r04: C2 0.175 / 0.178 against 0.179 / 0.180 ms with k_batch, profiles/r04k/).
template <int CMB, int RED>
__global__ __launch_bounds__(256) void k_batch_c(const BatchJob *__restrict__ jobs,
                                                 const uint32_t *__restrict__ block_job) {
  const uint32_t b = blockIdx.x;
  const uint32_t j = __builtin_amdgcn_readfirstlane(block_job[b]);
  const BatchJob &J = jobs[j];
  const uint64_t tid = (uint64_t)(b - J.block0) * blockDim.x + threadIdx.x;
  const uint64_t n = (uint64_t)J.nblocks * blockDim.x;
  if (J.c.row_mode == 2)
    contract_flat2<CMB, RED>(J.c, J.A, J.B, J.C, tid, n);
  else
    contract_flat<CMB, RED>(J.c, J.A, J.B, J.C, nullptr, tid, n, 0);
}

// The same for a batch of n-ary products only (C4's levelled BP sweep: the separator-sized products).
__global__ __launch_bounds__(256) void k_batch_p(const BatchJob *__restrict__ jobs,
                                                 const uint32_t *__restrict__ block_job) {
  const uint32_t b = blockIdx.x;
  const uint32_t j = __builtin_amdgcn_readfirstlane(block_job[b]);
  const BatchJob &J = jobs[j];
  const uint64_t tid = (uint64_t)(b - J.block0) * blockDim.x + threadIdx.x;
  const uint64_t n = (uint64_t)J.nblocks * blockDim.x;
  if (J.pn.pairs) {
    if (J.pn.n_ops <= 2) prodn_flat2<2>(J.pn, J.C, tid, n);
    else if (J.pn.n_ops <= 4) prodn_flat2<4>(J.pn, J.C, tid, n);
    else prodn_flat2<PMAX>(J.pn, J.C, tid, n);
    return;
  }
  if (J.pn.n_ops <= 2) prodn_flat<2>(J.pn, J.C, tid, n);
  else if (J.pn.n_ops <= 4) prodn_flat<4>(J.pn, J.C, tid, n);
  else prodn_flat<PMAX>(J.pn, J.C, tid, n);
}

__device__ __forceinline__ void batch_block(const BatchJob *__restrict__ jobs, const uint32_t *__restrict__ block_job,
                                            uint32_t b) {
  const uint32_t j = __builtin_amdgcn_readfirstlane(block_job[b]);
  const BatchJob &J = jobs[j];
  const uint64_t tid = (uint64_t)(b - J.block0) * blockDim.x + threadIdx.x;
  const uint64_t n = (uint64_t)J.nblocks * blockDim.x;
  if (J.kind == 1) {
    gather_body(J.g, J.A, J.codes, J.C, J.err, tid, n);
    return;
  }
  if (J.kind == 3) {
    indicator_body(J.codes, J.ind_rows, J.ind_card, J.C, J.ind_s_state, J.ind_s_row, J.err, (int64_t)tid, (int64_t)n);
    return;
  }
  if (J.kind == 2) {
    if (J.pn.pairs) {
      if (J.pn.n_ops <= 2) prodn_flat2<2>(J.pn, J.C, tid, n);
      else if (J.pn.n_ops <= 4) prodn_flat2<4>(J.pn, J.C, tid, n);
      else prodn_flat2<PMAX>(J.pn, J.C, tid, n);
      return;
    }
    if (J.pn.n_ops <= 2) prodn_flat<2>(J.pn, J.C, tid, n);
    else if (J.pn.n_ops <= 4) prodn_flat<4>(J.pn, J.C, tid, n);
    else prodn_flat<PMAX>(J.pn, J.C, tid, n);
    return;
  }
  switch (J.cmb) {
    case PGM_COMBINE_MUL: batch_contract_c<PGM_COMBINE_MUL>(J, tid, n); break;
    case PGM_COMBINE_ADD: batch_contract_c<PGM_COMBINE_ADD>(J, tid, n); break;
    case PGM_COMBINE_DIV: batch_contract_c<PGM_COMBINE_DIV>(J, tid, n); break;
    case PGM_COMBINE_DIV_RAW: batch_contract_c<PGM_COMBINE_DIV_RAW>(J, tid, n); break;
    default: batch_contract_c<PGM_COMBINE_COPY>(J, tid, n); break;
  }
}

__global__ __launch_bounds__(256) void k_indicator(const uint8_t *__restrict__ codes, int64_t n_rows, int64_t card,
                                                   double *__restrict__ out, int64_t s_state, int64_t s_row,
                                                   int32_t *__restrict__ err) {
  indicator_body(codes, n_rows, card, out, s_state, s_row, err, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                 (int64_t)gridDim.x * blockDim.x);
}

// ----------------------------------------------------------------------------- argmax
__device__ __forceinline__ bool am_better(double v, uint32_t i, double bv, uint32_t bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn) return !bn || i < bi;  // np.argmax: first NaN wins
  if (bn) return false;
  return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(256) void k_argmax(const double *__restrict__ X, uint64_t n_rows, uint32_t row_len,
                                                int64_t s_row, int64_t s_elem, int g_log2,
                                                int64_t *__restrict__ out, int32_t *__restrict__ out32) {
  const uint32_t G = 1u << g_log2;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane_g = (uint32_t)tid & (G - 1);
  const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) >> g_log2;
  for (uint64_t r = tid >> g_log2; r < n_rows; r += ngroups) {
    double bv = -__builtin_inf();
    uint32_t bi = 0xffffffffu;
    for (uint32_t i = lane_g; i < row_len; i += G) {
      const double v = X[(int64_t)r * s_row + (int64_t)i * s_elem];
      if (am_better(v, i, bv, bi)) {
        bv = v;
        bi = i;
      }
    }
    for (uint32_t off = G >> 1; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, (int)off, 64);
      const uint32_t oi = (uint32_t)__shfl_xor((int)bi, (int)off, 64);
      if (am_better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane_g == 0) {
      const int64_t v = (bi == 0xffffffffu) ? 0 : (int64_t)bi;
      if (out) out[r] = v;
      if (out32) out32[r] = (int32_t)v;
    }
  }
}

// ----------------------------------------------------------------------------- dense pairwise step
// C[b, m, n] = sum_k A[b, m, k] B[b, k, n], FP64 MFMA (v_mfma_f64_16x16x4_f64), every index a
// group of variables addressed through a per-index offset table (any label interleaving, no
// packing copies; C written directly in the planner's label order).  A 64x64 output tile per
// workgroup, 4 waves in 2x2, each wave a 32x32 block = 2x2 MFMA tiles (4 independent
// accumulators).  K advances 16 at a time through LDS, A staged transposed (As[k][m]) so each
// operand read is 16 consecutive doubles per k row; the next K tile's global loads are issued
// before the current tile's MFMAs (register prefetch).  Operand maps (gfx950 f64): lane l holds
// A[l&15][k=l>>4], B[k=l>>4][l&15]; D[reg r] is row (l>>4)+4r, col l&15.
struct GemmK {
  int64_t batch, M, N, K;
  const int64_t *a_b, *b_b, *c_b, *a_m, *c_m, *a_k, *b_k, *b_n, *c_n;
  int64_t s_ab, s_bb, s_cb, s_am, s_cm, s_ak, s_bk, s_bn, s_cn;  // >= 0: strided group, -1: table
  uint32_t tiles_n;
  uint32_t a_mfast, b_kfast;  // tile-load lane order: A along m (else k), B along k (else n) — the unit-stride axis
};
// offset of index i of a group: the table (TAB) or a single stride (the group collapses)
template <bool TAB>
__device__ __forceinline__ int64_t goff(int64_t s, const int64_t *tab, int64_t i) {
  if constexpr (TAB) return tab[i];
  else return i * s;
}

// TA / TB / TC: operand A, B, C addressed through its offset tables (some group does not collapse).
// BM x BN block tile, 4 waves in a WY x WX grid, each wave FM x FN 16x16 f64 MFMA tiles; BK = 16.
// Tiles: 64x64 (2x2 waves of 32x32), 16x128 for M <= 16 (1x4 waves of 16x32: no MFMA rows wasted on
// a 16-row step), 128x64 for 64 < M <= 128 (2x2 waves of 64x32: B read once per batch, not twice).
template <int BM, int BN, bool TA, bool TB, bool TC>
__global__ __launch_bounds__(256) void k_gemm_f64(const GemmK p, const double *__restrict__ A,
                                                  const double *__restrict__ B, double *__restrict__ C) {
  constexpr int BK = 16;
  constexpr int WY = BM >= 32 ? 2 : 1, WX = 4 / WY;
  constexpr int FM = BM / 16 / WY, FN = BN / 16 / WX;
  constexpr int NA = BM * BK / 256, NB = BN * BK / 256;  // tile elements per thread per k tile
  static_assert(FM >= 1 && FN >= 1 && NA >= 1 && NB >= 1, "tile shape");
#ifndef PGM_GEMM_PAD
#define PGM_GEMM_PAD 1
#endif
  __shared__ double As[BK][BM + PGM_GEMM_PAD];  // +1: the k-fast tile stores (16 lanes down a column) hit 32 distinct banks
  __shared__ double Bs[BK][BN + PGM_GEMM_PAD];
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wy = wave / WX, wx = wave % WX;
  const uint32_t t = blockIdx.x;  // n fastest within an m row of tiles (A rows stay hot in L2)
  const int64_t n0 = (int64_t)(t % p.tiles_n) * BN, m0 = (int64_t)(t / p.tiles_n) * BM;
  const int64_t b = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;  // batches beyond 65,535 continue in z
  if (b >= p.batch) return;  // (whole block: uniform)
  const double *Ab = A + goff<TA>(p.s_ab, p.a_b, b);
  const double *Bb = B + goff<TB>(p.s_bb, p.b_b, b);
  // this thread's tile elements per operand and k tile (e = tid + 256 i), lanes along the operand's
  // unit-stride axis: A k-fast (k = e % 16, m = e / 16) or m-fast (m = e % BM, k = e / BM);
  // B n-fast (n = e % BN, k = e / BN) or k-fast (k = e % 16, n = e / 16)
  const bool amf = p.a_mfast, bkf = p.b_kfast;
  int am[NA], ak[NA], bk[NB], bn[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int e = tid + 256 * i;
    am[i] = amf ? (e % BM) : (e >> 4);
    ak[i] = amf ? (e / BM) : (e & 15);
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int e = tid + 256 * i;
    bk[i] = bkf ? (e & 15) : (e / BN);
    bn[i] = bkf ? (e >> 4) : (e % BN);
  }
  int64_t arow[NA], bcol[NB];
  bool aok[NA], bok[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int64_t gm = m0 + am[i];
    aok[i] = gm < p.M;
    arow[i] = aok[i] ? goff<TA>(p.s_am, p.a_m, gm) : 0;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int64_t gn = n0 + bn[i];
    bok[i] = gn < p.N;
    bcol[i] = bok[i] ? goff<TB>(p.s_bn, p.b_n, gn) : 0;
  }
  double ra[NA], rb[NB];
  // k offsets.  SR (64 x 64 tiles): strided groups keep a running offset advanced by BK strides per
  // tile (one 64-bit add instead of a multiply and a clamp per element and tile: the plain 64 x 64
  // kernel was VALU-bound on that address arithmetic, 4096^2 x 512: 35 -> 40 TF/s); tiles wholly
  // inside K take unguarded loads, the last tile guards each k.  The 128 x 64 and 16 x 128 tiles keep
  // the clamped per-tile form (the running form costs them registers: 500 x (100 x 576 x 125)
  // 307 -> 400 us, profiles/r02bo_gemm_ab.txt).  Table groups read their entries one k tile ahead of
  // the loads that use them, so a table lookup never sits in series with its data load.
  constexpr bool SR = BM == 64 && BN == 64;
  int64_t oa[NA], ob[NB];
  const int64_t dka = (int64_t)BK * p.s_ak, dkb = (int64_t)BK * p.s_bk;
  auto offs = [&](int64_t k0) {
    const bool full = SR && k0 + BK <= p.K;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      if constexpr (TA || !SR) {
        const int64_t gka = k0 + ak[i];
        oa[i] = goff<TA>(p.s_ak, p.a_k, full ? gka : (gka < p.K ? gka : p.K - 1));
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      if constexpr (TB || !SR) {
        const int64_t gkb = k0 + bk[i];
        ob[i] = goff<TB>(p.s_bk, p.b_k, full ? gkb : (gkb < p.K ? gkb : p.K - 1));
      }
    }
  };
  if constexpr (SR && !TA) {
#pragma unroll
    for (int i = 0; i < NA; ++i) oa[i] = (int64_t)ak[i] * p.s_ak;
  }
  if constexpr (SR && !TB) {
#pragma unroll
    for (int i = 0; i < NB; ++i) ob[i] = (int64_t)bk[i] * p.s_bk;
  }
  // rows / columns past M / N (and, in the clamped form, k past K) read an in-bounds element and
  // are zeroed
  auto load = [&](int64_t k0) {
    double va[NA], vb[NB];
    if (!SR || k0 + BK <= p.K) {
#pragma unroll
      for (int i = 0; i < NA; ++i) va[i] = Ab[arow[i] + oa[i]];
#pragma unroll
      for (int i = 0; i < NB; ++i) vb[i] = Bb[ob[i] + bcol[i]];
#pragma unroll
      for (int i = 0; i < NA; ++i) ra[i] = (aok[i] && (SR || k0 + ak[i] < p.K)) ? va[i] : 0.0;
#pragma unroll
      for (int i = 0; i < NB; ++i) rb[i] = (bok[i] && (SR || k0 + bk[i] < p.K)) ? vb[i] : 0.0;
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        double v = 0.0;
        if (aok[i] && k0 + ak[i] < p.K) v = Ab[arow[i] + oa[i]];
        ra[i] = v;
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        double v = 0.0;
        if (bok[i] && k0 + bk[i] < p.K) v = Bb[ob[i] + bcol[i]];
        rb[i] = v;
      }
    }
    if constexpr (SR && !TA) {
#pragma unroll
      for (int i = 0; i < NA; ++i) oa[i] += dka;
    }
    if constexpr (SR && !TB) {
#pragma unroll
      for (int i = 0; i < NB; ++i) ob[i] += dkb;
    }
  };
  d4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  offs(0);
  load(0);
  offs(BK);
  for (int64_t k0 = 0; k0 < p.K; k0 += BK) {
#pragma unroll
    for (int i = 0; i < NA; ++i) As[ak[i]][am[i]] = ra[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) Bs[bk[i]][bn[i]] = rb[i];
    __syncthreads();
    if (k0 + BK < p.K) {  // in flight during this tile's MFMAs
      load(k0 + BK);
      offs(k0 + 2 * BK);
    }
#pragma unroll
    for (int s = 0; s < BK / 4; ++s) {
      const int kq = 4 * s + (lane >> 4);
      double av[FM], bv[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) av[i] = As[kq][(wy * FM + i) * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < FN; ++j) bv[j] = Bs[kq][(wx * FN + j) * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  double *Cb = C + goff<TC>(p.s_cb, p.c_b, b);
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int64_t cn = n0 + (wx * FN + j) * 16 + (lane & 15);
    if (cn >= p.N) continue;
    const int64_t ocn = goff<TC>(p.s_cn, p.c_n, cn);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t cm = m0 + (wy * FM + i) * 16 + (lane >> 4) + 4 * r;
        if (cm < p.M) Cb[goff<TC>(p.s_cm, p.c_m, cm) + ocn] = acc[i][j][r];
      }
  }
}

template <int BM, int BN>
static void launch_gemm(int tabs, dim3 g, hipStream_t s, const GemmK &k, const double *A, const double *B, double *C) {
  const dim3 b(256);
  switch (tabs) {
    case 0: hipLaunchKernelGGL((k_gemm_f64<BM, BN, false, false, false>), g, b, 0, s, k, A, B, C); break;
    case 1: hipLaunchKernelGGL((k_gemm_f64<BM, BN, false, false, true>), g, b, 0, s, k, A, B, C); break;
    case 2: hipLaunchKernelGGL((k_gemm_f64<BM, BN, false, true, false>), g, b, 0, s, k, A, B, C); break;
    case 3: hipLaunchKernelGGL((k_gemm_f64<BM, BN, false, true, true>), g, b, 0, s, k, A, B, C); break;
    case 4: hipLaunchKernelGGL((k_gemm_f64<BM, BN, true, false, false>), g, b, 0, s, k, A, B, C); break;
    case 5: hipLaunchKernelGGL((k_gemm_f64<BM, BN, true, false, true>), g, b, 0, s, k, A, B, C); break;
    case 6: hipLaunchKernelGGL((k_gemm_f64<BM, BN, true, true, false>), g, b, 0, s, k, A, B, C); break;
    default: hipLaunchKernelGGL((k_gemm_f64<BM, BN, true, true, true>), g, b, 0, s, k, A, B, C); break;
  }
}

// ----------------------------------------------------------------------------- evidence column select
__global__ __launch_bounds__(256) void k_codes_select(const uint8_t *__restrict__ codes, int64_t ld, int64_t row0,
                                                      const int32_t *__restrict__ cols, int64_t n_rows,
                                                      uint8_t *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y;
  if (r < n_rows) out[(int64_t)j * n_rows + r] = codes[(int64_t)cols[j] * ld + row0 + r];
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// ----------------------------------------------------------------------------- evidence ingestion
// DataFrame columns -> evidence codes (the reference maps each state name with
// name_to_no per row and evidence variable, state_name.py:71-84, DiscreteFactor.py:589-597).  Input:
// per-column int8 indices into that column's categories (pandas Categorical / Arrow dictionary
// indices, -1 = NaN); a per-column LUT maps a category index to the variable's state number (254 =
// a category that is not a state name of the variable).  Output: uint8 state codes (255 = NaN) and,
// per row, the key of its missing-column pattern (XOR of the missing columns' 64-bit keys) and its
// number of missing columns, from which the host groups rows by evidence pattern.  One thread per
// row over a chunk of columns (blockIdx.y); byte accesses along the rows are coalesced.
__global__ __launch_bounds__(256) void k_codes_remap(const int8_t *__restrict__ raw, int64_t ld_raw,
                                                     const uint8_t *__restrict__ lut, int32_t lut_stride,
                                                     int32_t n_cols, int64_t n_rows, int32_t chunk,
                                                     const uint64_t *__restrict__ col_key, uint8_t *__restrict__ out,
                                                     int64_t ld_out, unsigned long long *__restrict__ row_key,
                                                     uint32_t *__restrict__ row_nmiss,
                                                     unsigned long long *__restrict__ row_hash,
                                                     int32_t *__restrict__ err) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const int c0 = blockIdx.y * chunk;
  const int c1 = min(n_cols, c0 + chunk);
  unsigned long long key = 0, h0 = 0, h1 = 0;
  uint32_t nm = 0;
  bool bad = false;
  for (int c = c0; c < c1; ++c) {
    const int v = raw[(int64_t)c * ld_raw + r];
    uint8_t st;
    if (v < 0) {
      st = 255;
      key ^= col_key[c];
      ++nm;
    } else if (v >= lut_stride) {
      st = 254;
      bad = true;
    } else {
      st = lut[(int64_t)c * lut_stride + v];
      bad |= st == 254;
    }
    out[(int64_t)c * ld_out + r] = st;
    if (row_hash) {  // row content: XOR of two independent mixes of (column, state)
      const unsigned long long x = ((unsigned long long)c << 8) | st;
      h0 ^= mix64(x ^ 0x9e3779b97f4a7c15ull);
      h1 ^= mix64(x ^ 0xc2b2ae3d27d4eb4full);
    }
  }
  if (nm && row_key) {
    atomicXor(&row_key[r], key);
    atomicAdd(&row_nmiss[r], nm);
  }
  if (row_hash) {
    atomicXor(&row_hash[2 * r], h0);
    atomicXor(&row_hash[2 * r + 1], h1);
  }
  if (bad && err) atomicOr(err, 1);
}

// numpy's float64 add.reduce of a strided run (the pairwise summation of numpy's umath loops): runs
// of < 8 summed in order; runs of <= 128 in 8 interleaved accumulators combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail in order; longer runs split in two at a
// multiple of 8 below the half, each half summed the same way.  Post-order over an explicit stack.
// numpy hands the loop at most one 8,192-element buffer at a time and adds the buffers' sums in
// order (np_sum); checked bit for bit against numpy 2.2 up to 40,000 elements (tests).
__device__ double np_block_sum(const double *a, int64_t n, int64_t s) {
  if (n < 8) {
    double res = 0.0;
    for (int64_t i = 0; i < n; ++i) res += a[i * s];
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j * s];
  int64_t i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[(i + j) * s];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i * s];
  return res;
}

__device__ double np_pairwise_sum(const double *a, int64_t n, int64_t s) {
  if (n <= 128) return np_block_sum(a, n, s);
  int64_t off[40], len[40];
  double left[40];
  int stage[40];
  int top = 0;
  off[0] = 0, len[0] = n, stage[0] = 0;
  double val = 0.0;
  bool have = false;
  for (;;) {
    if (!have) {
      if (len[top] <= 128) {
        val = np_block_sum(a + off[top] * s, len[top], s);
        have = true;
        --top;
      } else {  // descend into the left half
        int64_t n2 = len[top] / 2;
        n2 -= n2 % 8;
        stage[top] = 1;
        off[top + 1] = off[top], len[top + 1] = n2, stage[top + 1] = 0;
        ++top;
      }
    } else {
      if (top < 0) return val;
      if (stage[top] == 1) {  // left done: the right half next
        int64_t n2 = len[top] / 2;
        n2 -= n2 % 8;
        left[top] = val;
        stage[top] = 2;
        off[top + 1] = off[top] + n2, len[top + 1] = len[top] - n2, stage[top + 1] = 0;
        ++top;
        have = false;
      } else {
        val = left[top] + val;
        --top;
      }
    }
  }
}

// predict(stochastic=True) (DiscreteBayesianNetwork.py:889-892 -> DiscreteFactor.sample L868-912):
// sample() normalises the joint (values / values.sum(), DiscreteFactor.py:530: numpy's pairwise sum)
// and numpy's Generator.choice(P, p=p) then takes cdf = cumsum(p) (in order), cdf /= cdf[-1] and
// index = searchsorted(cdf, u, side="right") = the number of cdf entries <= u.  The same operations
// in the same order per output row r, so a uniform on a CDF boundary lands where numpy puts it; the
// uniforms u come from the reference's seeded stream on the host.  joint column group[r].
__global__ __launch_bounds__(256) void k_sample_joint(const double *__restrict__ joint, int64_t ld, int64_t P,
                                                      const int32_t *__restrict__ group,
                                                      const double *__restrict__ u, int64_t n,
                                                      int32_t *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const double *q = joint + group[r];
  double total = 0.0;
  for (int64_t c = 0; c < P; c += 8192) total += np_pairwise_sum(q + c * ld, P - c < 8192 ? P - c : 8192, ld);
  double last = 0.0;
  for (int64_t i = 0; i < P; ++i) last = i ? last + q[i * ld] / total : q[0] / total;
  const double x = u[r];
  double acc = 0.0;
  int64_t idx = 0;
  for (int64_t i = 0; i < P; ++i) {
    acc = i ? acc + q[i * ld] / total : q[0] / total;
    if (acc / last <= x) idx = i + 1;
  }
  out[r] = (int32_t)(idx < P ? idx : P - 1);
}

// ============================================================================= C-ABI
extern "C" {

int pgm_version(void) { return PGM_ABI_VERSION; }

int pgm_last_error(char *buf, size_t len) {
  if (!buf || len == 0) return PGM_EINVAL;
  size_t n = std::min(len - 1, g_err.size());
  memcpy(buf, g_err.data(), n);
  buf[n] = 0;
  return PGM_OK;
}

int pgm_device_count(int *n) {
  STALE_PROBE();
  if (!n) return fail(PGM_EINVAL, "null pointer");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *n = 0;
    return fail(PGM_EDEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *n = c;
  return PGM_OK;
}

int pgm_set_device(int device) {
  STALE_PROBE();
  HIP_TRY(hipSetDevice(device));
  return PGM_OK;
}

int pgm_alloc(void **ptr, size_t bytes) {
  STALE_PROBE();
  if (!ptr) return fail(PGM_EINVAL, "null pointer");
  *ptr = nullptr;
  if (bytes == 0) return PGM_OK;
  HIP_TRY(hipMalloc(ptr, bytes));
  return PGM_OK;
}

int pgm_free(void *ptr) {
  STALE_PROBE();
  if (ptr) HIP_TRY(hipFree(ptr));
  return PGM_OK;
}

int pgm_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream) {
  STALE_PROBE();
  if (bytes == 0) return PGM_OK;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream)));
  return PGM_OK;
}

int pgm_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream) {
  STALE_PROBE();
  if (bytes == 0) return PGM_OK;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream)));
  HIP_TRY(hipStreamSynchronize(S(stream)));
  return PGM_OK;
}

int pgm_memcpy_d2h_async(void *dst, const void *src, size_t bytes, void *stream) {
  STALE_PROBE();
  if (bytes == 0) return PGM_OK;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream)));
  return PGM_OK;
}

int pgm_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream) {
  STALE_PROBE();
  if (bytes == 0) return PGM_OK;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, S(stream)));
  return PGM_OK;
}

int pgm_host_alloc(void **ptr, size_t bytes) {
  STALE_PROBE();
  if (!ptr) return fail(PGM_EINVAL, "host_alloc: null pointer");
  *ptr = nullptr;
  if (bytes == 0) bytes = 1;
  const hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *ptr = nullptr;
    return fail(e == hipErrorOutOfMemory ? PGM_ENOMEM : PGM_EDEVICE, "host_alloc: %s", hipGetErrorString(e));
  }
  memset(*ptr, 0, bytes);
  return PGM_OK;
}

int pgm_host_free(void *ptr) {
  STALE_PROBE();
  if (ptr) HIP_TRY(hipHostFree(ptr));
  return PGM_OK;
}

int pgm_memset(void *dst, int value, size_t bytes, void *stream) {
  STALE_PROBE();
  if (bytes == 0) return PGM_OK;
  HIP_TRY(hipMemsetAsync(dst, value, bytes, S(stream)));
  return PGM_OK;
}

int pgm_stream_sync(void *stream) {
  STALE_PROBE();
  HIP_TRY(hipStreamSynchronize(S(stream)));
  return PGM_OK;
}

// the same wait by polling the stream (hipStreamQuery in a loop): no blocking wait's wake-up latency, one
// host core busy meanwhile — for latency-bound single queries (C2: 0.223 -> 0.210 ms/query, r03ab)
int pgm_stream_sync_spin(void *stream) {
  STALE_PROBE();
  hipError_t e;
  while ((e = hipStreamQuery(S(stream))) == hipErrorNotReady) {
  }
  HIP_TRY(e);
  return PGM_OK;
}

int pgm_event_create(void **ev) {
  STALE_PROBE();
  if (!ev) return fail(PGM_EINVAL, "null pointer");
  hipEvent_t e;
  HIP_TRY(hipEventCreate(&e));
  *ev = (void *)e;
  return PGM_OK;
}

int pgm_event_destroy(void *ev) {
  STALE_PROBE();
  if (ev) HIP_TRY(hipEventDestroy((hipEvent_t)ev));
  return PGM_OK;
}

int pgm_event_record(void *ev, void *stream) {
  STALE_PROBE();
  HIP_TRY(hipEventRecord((hipEvent_t)ev, S(stream)));
  return PGM_OK;
}

int pgm_event_elapsed_ms(void *start, void *stop, float *ms) {
  STALE_PROBE();
  HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
  HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return PGM_OK;
}

int pgm_contract(const pgm_contract_desc *d, const double *A, const double *B, double *C, void *workspace,
                 size_t workspace_bytes, void *stream) {
  STALE_PROBE();
  ContractLaunch L;
  int rc = plan_contract(d, L);
  if (rc) return rc;
  if (L.empty) return PGM_OK;
  if (!A || !C) return fail(PGM_EINVAL, "contract: null A or C");
  if (d->combine != PGM_COMBINE_COPY && !B) return fail(PGM_EINVAL, "contract: null B for a binary combine");
  if (L.ws_doubles * sizeof(double) > workspace_bytes || (L.ws_doubles && !workspace))
    return fail(PGM_EINVAL, "contract: workspace of %zu bytes needed, %zu given",
                (size_t)(L.ws_doubles * sizeof(double)), workspace_bytes);
  double *ws = (double *)workspace;
  hipStream_t s = S(stream);
  switch (d->combine) {
    case PGM_COMBINE_MUL: launch_contract_c<PGM_COMBINE_MUL>(d->reduce, L, A, B, C, ws, s); break;
    case PGM_COMBINE_ADD: launch_contract_c<PGM_COMBINE_ADD>(d->reduce, L, A, B, C, ws, s); break;
    case PGM_COMBINE_DIV: launch_contract_c<PGM_COMBINE_DIV>(d->reduce, L, A, B, C, ws, s); break;
    case PGM_COMBINE_DIV_RAW: launch_contract_c<PGM_COMBINE_DIV_RAW>(d->reduce, L, A, B, C, ws, s); break;
    default: launch_contract_c<PGM_COMBINE_COPY>(d->reduce, L, A, B, C, ws, s); break;
  }
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_product_n(const pgm_productn_desc *d, const double *const *ops, double *C, void *stream) {
  STALE_PROBE();
  if (!d || !ops || !C) return fail(PGM_EINVAL, "product_n: null argument");
  ProdNK k;
  const int prc = plan_prodn(d, ops, k);
  if (prc != PGM_OK) return prc;
  const uint64_t n_out = k.n_out;
  const uint64_t NX = k.nk > 0 ? (uint64_t)k.kdiv[k.nk - 1].d : 1;
  uint32_t g[3] = {1, 1, 1};
  // two rows per lane when every access is 16-B aligned (batched BP: rows innermost, even count)
  if (k.row_mode && prodn_pairs_ok(k, C)) {
    const uint64_t NP = NX / 2;
    const uint64_t bs = std::min<uint64_t>(256, (NP + 63) / 64 * 64);
    row_grid(n_out / NX, (NP + bs - 1) / bs, g);
    hipStream_t s = S(stream);
    const dim3 g2(g[0], g[1], 1), b2((unsigned)bs);
    switch (d->n_ops <= 2 ? 2 : d->n_ops <= 4 ? 4 : 8) {
      case 2: hipLaunchKernelGGL((k_productn_rows2<2>), g2, b2, 0, s, k, C); break;
      case 4: hipLaunchKernelGGL((k_productn_rows2<4>), g2, b2, 0, s, k, C); break;
      default: hipLaunchKernelGGL((k_productn_rows2<8>), g2, b2, 0, s, k, C); break;
    }
    HIP_TRY(hipGetLastError());
    return PGM_OK;
  }
  if (k.row_mode)
    row_grid(n_out / NX, (NX + 255) / 256, g);
  else
    g[0] = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_out + 255) / 256, 1), 65535);
  const dim3 grid(g[0], g[1], 1);
  hipStream_t s = S(stream);
  switch (d->n_ops <= 2 ? 2 : d->n_ops <= 4 ? 4 : 8) {
    case 2: hipLaunchKernelGGL((k_productn<2>), grid, dim3(256), 0, s, k, C); break;
    case 4: hipLaunchKernelGGL((k_productn<4>), grid, dim3(256), 0, s, k, C); break;
    default: hipLaunchKernelGGL((k_productn<8>), grid, dim3(256), 0, s, k, C); break;
  }
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_product_n_marginal_ok(const pgm_productn_desc *d, const double *const *ops, const double *C,
                              const int64_t *marg_s, const double *M) {
  STALE_PROBE();
  ProdMK k;
  uint32_t g[3];
  return pgmi_plan_product_marg(d, ops, C, marg_s, M, k, g) == 1 ? 1 : 0;
}

int pgm_product_n_marginal(const pgm_productn_desc *d, const double *const *ops, double *C, const int64_t *marg_s,
                           int32_t reduce, double *M, void *stream) {
  STALE_PROBE();
  if (reduce != PGM_RED_SUM && reduce != PGM_RED_MAX)
    return fail(PGM_EINVAL, "product_n_marginal: reduce must be PGM_RED_SUM or PGM_RED_MAX");
  ProdMK k;
  uint32_t g[3];
  const int r = pgmi_plan_product_marg(d, ops, C, marg_s, M, k, g);
  if (r < 0) return r;
  if (r == 0)
    return fail(PGM_EINVAL, "product_n_marginal: shape not supported by the fused kernel "
                            "(pgm_product_n_marginal_ok is 0: run pgm_product_n + pgm_contract)");
  hipStream_t s = S(stream);
  const bool two = k.n_ops <= 2;
  // j-outer form: 2 row pairs per lane from 1,024 row pairs up, else 1 (MI355X, pathfinder's largest
  // clique: collect 413 -> 272 us at 4,000 rows, 94 -> 80 us at 1,000, against r02's j-inner kernel)
  const int XI = k.NP >= 1024 ? 2 : 1;
  const uint64_t gxj = (k.NP + 256ull * XI - 1) / (256ull * XI);
  const dim3 gj((unsigned)gxj, g[1], 1);
#define PGM_MARGJ_NOPS(NO, XX)                                                                               \
  if (reduce == PGM_RED_SUM) hipLaunchKernelGGL((k_productn_marg_jx<NO, PGM_RED_SUM, XX>), gj, dim3(256), 0, s, k, C, M); \
  else hipLaunchKernelGGL((k_productn_marg_jx<NO, PGM_RED_MAX, XX>), gj, dim3(256), 0, s, k, C, M);
#define PGM_MARGJ_LAUNCH(XX)                                                                                 \
  if (two) {                                                                                                 \
    PGM_MARGJ_NOPS(2, XX)                                                                                    \
  } else if (k.n_ops <= 4) {                                                                                 \
    PGM_MARGJ_NOPS(4, XX)                                                                                    \
  } else {                                                                                                   \
    PGM_MARGJ_NOPS(MOPS, XX)                                                                                 \
  }
  if (XI == 2) {
    PGM_MARGJ_LAUNCH(2)
  } else {
    PGM_MARGJ_LAUNCH(1)
  }
#undef PGM_MARGJ_LAUNCH
#undef PGM_MARGJ_NOPS
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_graph_capture_begin(void *stream) {
  STALE_PROBE();
  if (!stream) return fail(PGM_EINVAL, "graph capture needs a non-default stream");
  HIP_TRY(hipStreamBeginCapture(S(stream), hipStreamCaptureModeRelaxed));
  return PGM_OK;
}

int pgm_graph_capture_end(void *stream, void **graph_exec) {
  STALE_PROBE();
  if (!graph_exec) return fail(PGM_EINVAL, "null pointer");
  hipGraph_t g = nullptr;
  HIP_TRY(hipStreamEndCapture(S(stream), &g));
  hipGraphExec_t e = nullptr;
  hipError_t err = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (err != hipSuccess) {
    (void)hipGetLastError();
    return fail(PGM_EDEVICE, "hipGraphInstantiate: %s", hipGetErrorString(err));
  }
  *graph_exec = (void *)e;
  return PGM_OK;
}

int pgm_graph_launch(void *graph_exec, void *stream) {
  STALE_PROBE();
  if (!graph_exec) return fail(PGM_EINVAL, "null graph");
  HIP_TRY(hipGraphLaunch((hipGraphExec_t)graph_exec, S(stream)));
  return PGM_OK;
}

int pgm_graph_destroy(void *graph_exec) {
  STALE_PROBE();
  if (graph_exec) HIP_TRY(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
  return PGM_OK;
}

}  // extern "C"

// plan_gather, BatchHandle and the batch caps: pgm_prim.h / pgmprim_plan.cpp

template <int CMB>
static void launch_batch_cr(int red, dim3 g, hipStream_t s, const BatchJob *jobs, const uint32_t *map) {
  switch (red) {
    case PGM_RED_NONE: hipLaunchKernelGGL((k_batch_c<CMB, PGM_RED_NONE>), g, dim3(256), 0, s, jobs, map); break;
    case PGM_RED_SUM: hipLaunchKernelGGL((k_batch_c<CMB, PGM_RED_SUM>), g, dim3(256), 0, s, jobs, map); break;
    default: hipLaunchKernelGGL((k_batch_c<CMB, PGM_RED_MAX>), g, dim3(256), 0, s, jobs, map); break;
  }
}

static void launch_batch_c(int spec, dim3 g, hipStream_t s, const BatchJob *jobs, const uint32_t *map) {
  const int red = spec % 3;
  switch (spec / 3) {
    case PGM_COMBINE_MUL: launch_batch_cr<PGM_COMBINE_MUL>(red, g, s, jobs, map); break;
    case PGM_COMBINE_ADD: launch_batch_cr<PGM_COMBINE_ADD>(red, g, s, jobs, map); break;
    case PGM_COMBINE_DIV: launch_batch_cr<PGM_COMBINE_DIV>(red, g, s, jobs, map); break;
    case PGM_COMBINE_DIV_RAW: launch_batch_cr<PGM_COMBINE_DIV_RAW>(red, g, s, jobs, map); break;
    default: launch_batch_cr<PGM_COMBINE_COPY>(red, g, s, jobs, map); break;
  }
}

extern "C" {

int pgm_gather(const pgm_gather_desc *d, const double *A, const uint8_t *codes, double *C, int32_t *err_flag,
               void *stream) {
  STALE_PROBE();
  if (!d || !A || !C) return fail(PGM_EINVAL, "gather: null argument");
  if (d->n_ev > 0 && !codes) return fail(PGM_EINVAL, "gather: null codes");
  GatherK k;
  int rc = plan_gather(d, k);
  if (rc != PGM_OK) return rc;
  if (k.n_out == 0) return PGM_OK;
  uint64_t blocks = std::min<uint64_t>((k.n_out + 255) / 256, 65535);
  hipLaunchKernelGGL(k_gather, dim3((unsigned)blocks), dim3(256), 0, S(stream), k, A, codes, C, err_flag);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_batch_create(void **handle) {
  STALE_PROBE();
  if (!handle) return fail(PGM_EINVAL, "batch_create: null handle");
  *handle = new (std::nothrow) BatchHandle;
  return *handle ? PGM_OK : fail(PGM_ENOMEM, "batch_create: host allocation");
}

static void batch_free(BatchHandle *h) {
  if (h->d_jobs) (void)hipFree(h->d_jobs);
  if (h->d_map) (void)hipFree(h->d_map);
  if (h->d_level) (void)hipFree(h->d_level);
  if (h->d_chain) (void)hipFree(h->d_chain);
  h->d_chain = nullptr;
  h->chain_lds = 0;
  h->d_jobs = nullptr;
  h->d_map = nullptr;
  h->d_level = nullptr;
}

int pgm_batch_finalize(void *handle) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h) return fail(PGM_EINVAL, "batch_finalize: null handle");
  if (h->d_jobs || h->jobs.empty()) return PGM_OK;
  std::vector<ChainJob> cj;
  size_t lds = 0;
  const int rc = batch_close(h, cj, lds);
  if (rc != PGM_OK) return rc;
  hipError_t e = hipMalloc((void **)&h->d_jobs, sizeof(BatchJob) * h->jobs.size());
  if (e == hipSuccess) e = hipMalloc((void **)&h->d_map, sizeof(uint32_t) * h->block_job.size());
  if (e == hipSuccess)
    e = hipMemcpy(h->d_jobs, h->jobs.data(), sizeof(BatchJob) * h->jobs.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_map, h->block_job.data(), sizeof(uint32_t) * h->block_job.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess && h->mode == PGM_BATCH_ONE_WORKGROUP) {  // k_batch_wg_c: staged descriptors + level table
    e = hipMalloc((void **)&h->d_level, sizeof(uint32_t) * h->level_off.size());
    if (e == hipSuccess)
      e = hipMemcpy(h->d_level, h->level_off.data(), sizeof(uint32_t) * h->level_off.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_chain, sizeof(ChainJob) * cj.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_chain, cj.data(), sizeof(ChainJob) * cj.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) h->chain_lds = lds;
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    batch_free(h);
    return fail(e == hipErrorOutOfMemory ? PGM_ENOMEM : PGM_EDEVICE, "batch_finalize: %s", hipGetErrorString(e));
  }
  return PGM_OK;
}

int pgm_batch_run(void *handle, void *stream) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h) return fail(PGM_EINVAL, "batch_run: null handle");
  if (h->jobs.empty()) return PGM_OK;
  if (!h->d_jobs) return fail(PGM_EINVAL, "batch_run: not finalized");
  if (!h->njobs.empty())
    return fail(PGM_EINVAL, "batch_run: n-ary contraction jobs run only in the batch's specialised kernel (pgm_batch_specialise)");
  if (h->mode == PGM_BATCH_ONE_WORKGROUP) {
    const uint32_t n_levels = (uint32_t)h->level_off.size() - 1;
    hipLaunchKernelGGL(k_batch_wg_c, dim3(1), dim3(256 * kChainVB), h->chain_lds, S(stream), (const ChainJob *)h->d_chain,
                       h->d_map, h->d_level, n_levels, (uint32_t)h->jobs.size(), (uint32_t)h->block_job.size());
  } else if (h->spec == kBatchSpecProducts) {
    hipLaunchKernelGGL(k_batch_p, dim3((unsigned)h->block_job.size()), dim3(256), 0, S(stream), h->d_jobs, h->d_map);
  } else if (h->spec >= 0) {
    launch_batch_c(h->spec, dim3((unsigned)h->block_job.size()), S(stream), h->d_jobs, h->d_map);
  } else {
    hipLaunchKernelGGL(k_batch, dim3((unsigned)h->block_job.size()), dim3(256), 0, S(stream), h->d_jobs, h->d_map);
  }
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_batch_specialise(void *handle, void **bound) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h || !bound) return fail(PGM_EINVAL, "batch_specialise: null argument");
  *bound = nullptr;
  if (!h->d_jobs) return fail(PGM_EINVAL, "batch_specialise: not finalized");
  std::vector<pgmi_cs_job> jobs;
  for (const BatchJob &J : h->jobs) {
    if ((J.kind > 1 && J.kind != 4) || (J.kind == 0 && J.c.n_split != 1)) return PGM_OK;  // contractions and gathers only
    pgmi_cs_job c;
    memset(&c, 0, sizeof c);
    if (J.kind == 4) {  // n-ary contraction
      c.kind = 2;
      c.red = J.red;
      c.block0 = J.block0;
      c.nblocks = J.nblocks;
      c.C = J.C;
      c.n = h->njobs[J._pad];
      for (int t = 0; t < c.n.n_ops; ++t) c.ops[t] = h->nops[J._pad][t];
      jobs.push_back(c);
      continue;
    }
    c.kind = J.kind;
    c.cmb = J.cmb;
    c.red = J.red;
    c.block0 = J.block0;
    c.nblocks = J.nblocks;
    c.A = J.A;
    c.B = J.B;
    c.C = J.C;
    c.codes = J.codes;
    c.err = J.err;
    if (J.kind == 0) c.k = J.c;
    else c.g = J.g;
    jobs.push_back(c);
  }
  if (jobs.empty()) return PGM_OK;
  return pgmi_cs_bind(jobs.data(), (int)jobs.size(), h->level_off.data(), (int)h->level_off.size() - 1,
                      h->mode == PGM_BATCH_ONE_WORKGROUP ? 1 : 0, bound);
}

int pgm_batch_destroy(void *handle) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h) return PGM_OK;
  batch_free(h);
  delete h;
  return PGM_OK;
}

int pgm_indicator(const uint8_t *codes, int64_t n_rows, int64_t card, double *out, int64_t s_state, int64_t s_row,
                  int32_t *err_flag, void *stream) {
  STALE_PROBE();
  if (!codes || !out) return fail(PGM_EINVAL, "indicator: null argument");
  if (n_rows <= 0 || card <= 0) return PGM_OK;
  uint64_t blocks = std::min<uint64_t>((uint64_t)(n_rows * card + 255) / 256, 65535);
  hipLaunchKernelGGL(k_indicator, dim3((unsigned)blocks), dim3(256), 0, S(stream), codes, n_rows, card, out, s_state,
                     s_row, err_flag);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_argmax(const double *X, int64_t n_rows, int64_t row_len, int64_t s_row, int64_t s_elem, int64_t *out_idx,
               int32_t *out_idx32, void *stream) {
  STALE_PROBE();
  if (!X || (!out_idx && !out_idx32)) return fail(PGM_EINVAL, "argmax: null argument");
  if (n_rows <= 0) return PGM_OK;
  if (row_len <= 0) return fail(PGM_EINVAL, "argmax: empty rows (np.argmax of an empty sequence)");
  if (row_len >= (1ll << 31)) return fail(PGM_EINVAL, "argmax: row too long");
  const int g = lanes_log2((uint64_t)n_rows, kTargetThreads, (uint64_t)row_len);
  uint64_t threads = (uint64_t)n_rows << g;
  uint64_t blocks = std::min<uint64_t>((threads + 255) / 256, 65535);
  hipLaunchKernelGGL(k_argmax, dim3((unsigned)blocks), dim3(256), 0, S(stream), X, (uint64_t)n_rows,
                     (uint32_t)row_len, s_row, s_elem, g, out_idx, out_idx32);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_gemm(const pgm_gemm_desc *d, const double *A, const double *B, double *C, void *stream) {
  STALE_PROBE();
  if (!d || !A || !B || !C || !d->offsets) return fail(PGM_EINVAL, "gemm: null argument");
  if (d->batch < 0 || d->m < 0 || d->n < 0 || d->k < 0) return fail(PGM_EINVAL, "gemm: negative extent");
  if (d->batch == 0 || d->m == 0 || d->n == 0) return PGM_OK;
  GemmK k;
  k.batch = d->batch;
  k.M = d->m;
  k.N = d->n;
  k.K = d->k;
  const int64_t *o = d->offsets;
  k.a_b = o;
  k.b_b = o + d->batch;
  k.c_b = o + 2 * d->batch;
  k.a_m = o + 3 * d->batch;
  k.c_m = k.a_m + d->m;
  k.a_k = k.c_m + d->m;
  k.b_k = k.a_k + d->k;
  k.b_n = k.b_k + d->k;
  k.c_n = k.b_n + d->n;
  k.s_ab = d->stride[0];
  k.s_bb = d->stride[1];
  k.s_cb = d->stride[2];
  k.s_am = d->stride[3];
  k.s_cm = d->stride[4];
  k.s_ak = d->stride[5];
  k.s_bk = d->stride[6];
  k.s_bn = d->stride[7];
  k.s_cn = d->stride[8];
  // block tile by M
  // 128-row tile only while it still gives >= 4 blocks per CU (it halves the blocks of a 65..128-row
  // step; it pays when B is large and would be read twice: C2's 500 x (100 x 576 x 125) step 495 -> 396 us)
  const bool tall_ok = d->m > 64 && d->m <= 128 && (uint64_t)d->batch * (((uint64_t)d->n + 63) / 64) >= 1024;
  const int cfg = d->m <= 16 ? 1 : tall_ok ? 2 : 0;
  const uint64_t BM = cfg == 1 ? 16 : cfg == 2 ? 128 : 64, BN = cfg == 1 ? 128 : 64;
  const uint64_t tn = ((uint64_t)d->n + BN - 1) / BN, tm = ((uint64_t)d->m + BM - 1) / BM;
  if (tn * tm > 0x7fffffffull || d->batch > 65535ll * 65535ll) return fail(PGM_EINVAL, "gemm: grid too large");
  k.tiles_n = (uint32_t)tn;
  if (d->k == 0) return fail(PGM_EINVAL, "gemm: k == 0 (nothing to sum; use the generic contraction)");
  // tile-load lane order along each operand's unit-stride axis (r01: 28.7 -> 32.6 TF/s on plain layouts)
  const bool am_unit = d->stride[3] == 1 || (d->stride[3] < 0 && (d->lane_order & 1));
  const bool bk_unit = d->stride[6] == 1 || (d->stride[6] < 0 && (d->lane_order & 2));
  k.a_mfast = (am_unit && d->stride[5] != 1) ? 1u : 0u;
  k.b_kfast = (bk_unit && d->stride[7] != 1) ? 1u : 0u;
  const bool ta = d->stride[0] < 0 || d->stride[3] < 0 || d->stride[5] < 0;
  const bool tb = d->stride[1] < 0 || d->stride[6] < 0 || d->stride[7] < 0;
  const bool tc = d->stride[2] < 0 || d->stride[4] < 0 || d->stride[8] < 0;
  const int tabs = (ta ? 4 : 0) | (tb ? 2 : 0) | (tc ? 1 : 0);
  const uint64_t gy = std::min<int64_t>(d->batch, 65535), gz = ((uint64_t)d->batch + gy - 1) / gy;
  const dim3 g((unsigned)(tn * tm), (unsigned)gy, (unsigned)gz);
  hipStream_t s = S(stream);
  if (cfg == 1) launch_gemm<16, 128>(tabs, g, s, k, A, B, C);
  else if (cfg == 2) launch_gemm<128, 64>(tabs, g, s, k, A, B, C);
  else launch_gemm<64, 64>(tabs, g, s, k, A, B, C);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_codes_select(const uint8_t *codes, int64_t ld, int64_t row0, const int32_t *cols, int32_t n_cols,
                     int64_t n_rows, uint8_t *out, void *stream) {
  STALE_PROBE();
  if (n_cols <= 0 || n_rows <= 0) return PGM_OK;
  if (!codes || !cols || !out) return fail(PGM_EINVAL, "codes_select: null argument");
  if (n_cols > 65535) return fail(PGM_EINVAL, "codes_select: too many columns");
  const uint64_t bx = ((uint64_t)n_rows + 255) / 256;
  if (bx > 0x7fffffffull) return fail(PGM_EINVAL, "codes_select: too many rows");
  hipLaunchKernelGGL(k_codes_select, dim3((unsigned)bx, (unsigned)n_cols), dim3(256), 0, S(stream), codes, ld, row0,
                     cols, n_rows, out);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgm_codes_remap(const int8_t *raw, int64_t ld_raw, int32_t n_cols, int64_t n_rows, const uint8_t *lut,
                    int32_t lut_stride, const uint64_t *col_key, uint8_t *out, int64_t ld_out, uint64_t *row_key,
                    uint32_t *row_nmiss, uint64_t *row_hash, int32_t *err_flag, void *stream) {
  STALE_PROBE();
  if (n_cols <= 0 || n_rows <= 0) return PGM_OK;
  if (!raw || !lut || !out || (row_key && (!row_nmiss || !col_key)))
    return fail(PGM_EINVAL, "codes_remap: null argument");
  if (ld_raw < n_rows || ld_out < n_rows || lut_stride < 1 || lut_stride > 256)
    return fail(PGM_EINVAL, "codes_remap: bad leading dimension or LUT stride");
  const uint64_t bx = ((uint64_t)n_rows + 255) / 256;
  if (bx > 0x7fffffffull) return fail(PGM_EINVAL, "codes_remap: too many rows");
  // enough (row block x column chunk) workgroups to fill the chip, each chunk >= 16 columns
  int chunks = 1;
  while (chunks < 64 && bx * chunks < 2048 && n_cols / (chunks * 2) >= 16) chunks *= 2;
  const int chunk = (n_cols + chunks - 1) / chunks;
  hipLaunchKernelGGL(k_codes_remap, dim3((unsigned)bx, (unsigned)chunks), dim3(256), 0, S(stream), raw, ld_raw, lut,
                     lut_stride, n_cols, n_rows, chunk, col_key, out, ld_out, (unsigned long long *)row_key, row_nmiss,
                     (unsigned long long *)row_hash, err_flag);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

// host-side scan (no device): for each of n_cols int8 code columns (n cells each), whether any cell is
// negative (pandas Categorical NaN = -1).  Columns are split over up to `threads` host threads; each
// column is OR-reduced 8 cells per 64-bit word and tested on the sign bits.
// pgm_host_any_negative_i8: pgmhost.cpp (r06: one persistent host thread pool)

int pgm_sample_joint(const double *joint, int64_t ld, int64_t P, const int32_t *group, const double *u, int64_t n,
                     int32_t *out_idx, void *stream) {
  STALE_PROBE();
  if (n <= 0) return PGM_OK;
  if (!joint || !group || !u || !out_idx || P <= 0 || P > 0x7fffffff) return fail(PGM_EINVAL, "sample_joint: bad argument");
  const uint64_t bx = ((uint64_t)n + 255) / 256;
  if (bx > 0x7fffffffull) return fail(PGM_EINVAL, "sample_joint: too many rows");
  hipLaunchKernelGGL(k_sample_joint, dim3((unsigned)bx), dim3(256), 0, S(stream), joint, ld, P, group, u, n, out_idx);
  HIP_TRY(hipGetLastError());
  return PGM_OK;
}

int pgmi_fail(int code, const char *msg) { return fail(code, "%s", msg); }

int pgmi_failf(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return fail(code, "%s", buf);
}

}  // extern "C"

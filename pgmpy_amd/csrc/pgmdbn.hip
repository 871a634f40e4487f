// pgmdbn.hip — the dynamic-network filter on the device (include/pgmhip.h "dynamic Bayesian networks"):
// k_dbn runs the scaled forward recursion and, when asked, the backward one for a batch of evidence
// sequences in one launch.  One wave per workgroup; a sequence owns P lanes of it (P a power of two) and
// its alpha, message and beta vectors in LDS.  The plan (pgmdbn_plan.cpp) turned every table index into
// three added offsets: what the clamped codes give (cl, per sequence, slice and family), what the free
// nodes of x' give (xoff) and what the interface state gives (ioff).  k_dbn_viterbi, further down, is the
// max-product recursion on the same plan with backpointers and a backtrack: the most probable sequence.
// k_dbn_estep, last, is the smoother with every term of gamma added to fp64 count tables: Baum-Welch's E-step.
#include <math.h>

#include <algorithm>

#include "pgm_dbn.h"
#include "pgm_hip_common.h"

struct DbnArgs {
  DbnLayout L;
  const int32_t *tab;
  const uint8_t *codes;
  int64_t ld, row0, B;
  int32_t T1;  // slices
  const double *val0, *val1;
  double *filter, *smooth, *loglik, *scratch;
  uint8_t *impossible;
  int32_t *err;
};

namespace {

// everything a lane needs of its sequence; the LDS pointers are the sequence's own
struct Seq {
  const DbnArgs &a;
  double *A, *msg, *beta;
  int32_t *cl;
  uint8_t *ev;  // [0, n): the codes of the slice before, [n, 2n): of the slice itself
  int64_t seq, row;
  int xl;
  bool live;
};

__device__ __forceinline__ double seg_sum(double v, int P) {
  for (int m = P >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the codes of slices t - 1 and t, checked: a clamped code that is no state reads as state 0, a free one
// as missing, and either raises the flag
__device__ void load_ev(const Seq &s, int t) {
  const DbnLayout &L = s.a.L;
  const int32_t *card = s.a.tab + L.o_card, *clamp = s.a.tab + L.o_clamp;
  bool bad = false;
  for (int v = s.xl; v < L.n; v += L.P)
    for (int h = 0; h < 2; ++h) {
      const int ts = t - 1 + h;
      int code = 0;
      if (ts >= 0) {
        code = s.a.codes[((int64_t)ts * L.n + v) * s.a.ld + s.row];
        if (code >= card[v]) {
          if (clamp[v])
            bad = true, code = 0;
          else if (code != PGM_EV_MISSING)
            bad = true, code = PGM_EV_MISSING;
        }
      }
      if (s.live) s.ev[h * L.n + v] = (uint8_t)code;
    }
  if (bad && s.live) atomicOr(s.a.err, 1);
}

__device__ void compute_cl(const Seq &s, int k) {
  const DbnLayout &L = s.a.L;
  const int32_t *ctoff = s.a.tab + L.o_ctoff[k], *ctidx = s.a.tab + L.o_ctidx[k], *ctstr = s.a.tab + L.o_ctstr[k];
  for (int f = s.xl; f < L.n; f += L.P) {
    int32_t o = 0;
    for (int e = ctoff[f]; e < ctoff[f + 1]; ++e) o += (int32_t)s.ev[ctidx[e]] * ctstr[e];
    if (s.live) s.cl[f] = o;
  }
}

__device__ __forceinline__ bool consistent(const Seq &s, int x) {
  const DbnLayout &L = s.a.L;
  const int32_t *card = s.a.tab + L.o_card, *xstride = s.a.tab + L.o_xstride, *fr = s.a.tab + L.o_free;
  for (int j = 0; j < L.n_free; ++j) {
    const int v = fr[j];
    const int code = s.ev[L.n + v];
    if (code != PGM_EV_MISSING && code != x / xstride[v] % card[v]) return false;
  }
  return true;
}

// the factor of x that does not depend on the interface state: every slice-0 family at t = 0, the
// transition families without a free slice-t parent after it
__device__ __forceinline__ double local_factor(const Seq &s, int x, bool first) {
  const DbnLayout &L = s.a.L;
  double p = 1.0;
  if (first) {
    const int32_t *voff = s.a.tab + L.o_voff[0], *xoff = s.a.tab + L.o_xoff[0];
    for (int f = 0; f < L.n; ++f) p *= s.a.val0[voff[f] + s.cl[f] + xoff[f * L.J + x]];
  } else {
    const int32_t *voff = s.a.tab + L.o_voff[1], *xoff = s.a.tab + L.o_xoff[1], *cur = s.a.tab + L.o_cur;
    for (int l = 0; l < L.n_cur; ++l) {
      const int f = cur[l];
      p *= s.a.val1[voff[f] + s.cl[f] + xoff[f * L.J + x]];
    }
  }
  return p;
}

// prod over the transition families with a free slice-t parent, at interface state i and slice state x
__device__ __forceinline__ double trans_factor(const Seq &s, int i, int x, double p) {
  const DbnLayout &L = s.a.L;
  const int32_t *voff = s.a.tab + L.o_voff[1], *xoff = s.a.tab + L.o_xoff[1], *prev = s.a.tab + L.o_prev,
                *ioff = s.a.tab + L.o_ioff;
  for (int l = 0; l < L.n_prev; ++l) {
    const int f = prev[l];
    p *= s.a.val1[voff[f] + s.cl[f] + xoff[f * L.J + x] + ioff[l * L.S + i]];
  }
  return p;
}

// sum_i msg(i) prod(i, x), i ascending.  With few families the part of a family's offset that x fixes is taken
// once, outside the loop over i; the products are the same operations in the same order either way.
static constexpr int kDbnHoist = 8;
__device__ __forceinline__ double carried(const Seq &s, int x) {
  const DbnLayout &L = s.a.L;
  double acc = 0.0;
  if (L.n_prev > kDbnHoist) {
    for (int i = 0; i < L.S; ++i) acc += trans_factor(s, i, x, s.msg[i]);
    return acc;
  }
  const int32_t *voff = s.a.tab + L.o_voff[1], *xoff = s.a.tab + L.o_xoff[1], *prev = s.a.tab + L.o_prev,
                *ioff = s.a.tab + L.o_ioff;
  int32_t base[kDbnHoist];
#pragma unroll
  for (int l = 0; l < kDbnHoist; ++l) {
    base[l] = 0;
    if (l < L.n_prev) {
      const int f = prev[l];
      base[l] = voff[f] + s.cl[f] + xoff[f * L.J + x];
    }
  }
  for (int i = 0; i < L.S; ++i) {
    double p = s.msg[i];
#pragma unroll
    for (int l = 0; l < kDbnHoist; ++l)
      if (l < L.n_prev) p *= s.a.val1[base[l] + ioff[l * L.S + i]];
    acc += p;
  }
  return acc;
}

// the marginals of the queried nodes from A (divided by den), the states of a node in x order
__device__ void marginals(const Seq &s, double *out, int t, double den, bool nan) {
  const DbnLayout &L = s.a.L;
  const int32_t *card = s.a.tab + L.o_card, *clamp = s.a.tab + L.o_clamp, *xstride = s.a.tab + L.o_xstride,
                *qnode = s.a.tab + L.o_qnode, *qstate = s.a.tab + L.o_qstate;
  for (int q = s.xl; q < L.Q; q += L.P) {
    const int v = qnode[q], k = qstate[q];
    double m = 0.0;
    if (clamp[v]) {
      m = s.ev[L.n + v] == k ? 1.0 : 0.0;
    } else {
      const int st = xstride[v], blk = st * card[v];
      for (int hi = 0; hi < L.J; hi += blk)
        for (int lo = 0; lo < st; ++lo) m += s.A[hi + k * st + lo];
      m /= den;
    }
    if (s.live) out[(s.seq * s.a.T1 + t) * L.Q + q] = nan ? NAN : m;
  }
}

}  // namespace

__global__ __launch_bounds__(kDbnBlock) void k_dbn(const DbnArgs a) {
  extern __shared__ double lds[];
  const DbnLayout &L = a.L;
  const int lane = (int)threadIdx.x, P = L.P, J = L.J, S = L.S, n = L.n;
  const int seg = lane / P;
  const int64_t seq = (int64_t)blockIdx.x * L.spw + seg;
  // a lane without a sequence computes on the first one's data and stores nothing
  const bool live = seg < L.spw && seq < a.B;
  const int sg = live ? seg : 0;
  int32_t *cl_all = reinterpret_cast<int32_t *>(lds + (size_t)L.spw * (J + 2 * S));
  uint8_t *ev_all = reinterpret_cast<uint8_t *>(cl_all + (size_t)L.spw * n);
  const Seq s = {a,
                 lds + (size_t)sg * J,
                 lds + (size_t)L.spw * J + (size_t)sg * S,
                 lds + (size_t)L.spw * (J + S) + (size_t)sg * S,
                 cl_all + (size_t)sg * n,
                 ev_all + (size_t)sg * 2 * n,
                 live ? seq : 0,
                 a.row0 + (live ? seq : 0),
                 lane % P,
                 live};
  const int xl = s.xl, T1 = a.T1;
  const int32_t *ix = a.tab + L.o_ix, *xperm = a.tab + L.o_xperm;
  double *scr = a.smooth ? a.scratch + s.seq * T1 * (S + 1) : nullptr;

  // ------------------------------------------------------------------ forward
  double ll = 0.0;
  bool dead = false;
  for (int t = 0; t < T1; ++t) {
    load_ev(s, t);
    __syncthreads();
    compute_cl(s, t ? 1 : 0);
    if (t)
      for (int i = xl; i < S; i += P) {
        double m = 0.0;
        for (int r = 0; r < L.R; ++r) m += s.A[xperm[i * L.R + r]];
        if (live) {
          s.msg[i] = m;
          if (scr) scr[(t - 1) * (S + 1) + i] = m;
        }
      }
    __syncthreads();
    double part = 0.0;
    for (int x = xl; x < J; x += P) {
      double v = 0.0;
      if (consistent(s, x)) {
        v = local_factor(s, x, t == 0);
        if (t) v *= carried(s, x);
      }
      if (live) s.A[x] = v;
      part += v;
    }
    const double c = seg_sum(part, P);
    if (live)
      for (int x = xl; x < J; x += P) s.A[x] /= c;
    if (!(c > 0.0)) dead = true;
    ll += log(c);
    if (scr && live && xl == 0) scr[t * (S + 1) + S] = c;
    __syncthreads();
    if (a.filter) marginals(s, a.filter, t, 1.0, dead);
    __syncthreads();
  }
  if (live && xl == 0) {
    if (a.loglik) a.loglik[seq] = dead ? -INFINITY : ll;
    if (a.impossible) a.impossible[seq] = dead ? 1 : 0;
  }
  if (!a.smooth) return;

  // ------------------------------------------------------------------ backward
  if (live)
    for (int i = xl; i < S; i += P) s.beta[i] = 1.0;
  for (int t = T1 - 1; t >= 0; --t) {
    load_ev(s, t);
    if (t && live)
      for (int i = xl; i < S; i += P) s.msg[i] = scr[(t - 1) * (S + 1) + i];
    const double c = scr[t * (S + 1) + S];
    __syncthreads();
    compute_cl(s, t ? 1 : 0);
    __syncthreads();
    // gamma_t = alpha_t beta_t(I(x)), alpha_t rebuilt from the message of the slice before
    double part = 0.0;
    for (int x = xl; x < J; x += P) {
      double g = 0.0;
      if (consistent(s, x)) {
        g = local_factor(s, x, t == 0);
        if (t) g *= carried(s, x);
        g = g / c * s.beta[ix[x]];
      }
      if (live) s.A[x] = g;
      part += g;
    }
    const double gs = seg_sum(part, P);
    __syncthreads();
    marginals(s, a.smooth, t, gs, dead);
    __syncthreads();
    if (!t) break;
    // beta_t-1(i) = sum_x' w(x') prod(i, x'), w = 1[e] local(x') beta_t(I(x')) / c_t, x' ascending
    for (int x = xl; x < J; x += P) {
      const double w = consistent(s, x) ? local_factor(s, x, false) * s.beta[ix[x]] / c : 0.0;
      if (live) s.A[x] = w;
    }
    __syncthreads();
    for (int i = xl; i < S; i += P) {
      double b = 0.0;
      for (int x = 0; x < J; ++x) {
        const double w = s.A[x];
        if (w != 0.0) b += trans_factor(s, i, x, w);
      }
      if (live) s.beta[i] = b;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- Viterbi
// k_dbn_viterbi — the max-product form of the forward pass and the backtrack, one launch (include/pgmhip.h
// "dynamic Bayesian networks: MAP sequences").  The plan, the mapping and the LDS layout are k_dbn's: delta_t
// lies where alpha_t does, m_t where the message does, and argx_t (S int32) in the beta region.
// Backpointers: bp, uint16 (J <= 4096), [t - 1][sequence of the launch][J] for t = 1 .. T: the state of
// slice t - 1 that the best path into state x of slice t comes from.  The sequences of a wave write
// neighbouring runs of J entries per slice; the backtrack is one dependent load per slice, the same
// address in every lane of the sequence.  The layout is private to this kernel.
struct DbnVitArgs {
  DbnArgs a;  // filter, smooth and scratch unused; loglik is logmap
  uint8_t *path;
  int64_t ld_out, row0_out;
  uint16_t *bp;
};

namespace {

// max_i msg(i) prod(i, x), i ascending, the first maximum kept (strict >); *psi: that i.  The products are
// carried()'s: the same operations in the same order.
__device__ __forceinline__ double carried_max(const Seq &s, int x, int *psi) {
  const DbnLayout &L = s.a.L;
  double best = -1.0;
  int at = 0;
  if (L.n_prev > kDbnHoist) {
    for (int i = 0; i < L.S; ++i) {
      const double p = trans_factor(s, i, x, s.msg[i]);
      if (p > best) best = p, at = i;
    }
    *psi = at;
    return best;
  }
  const int32_t *voff = s.a.tab + L.o_voff[1], *xoff = s.a.tab + L.o_xoff[1], *prev = s.a.tab + L.o_prev,
                *ioff = s.a.tab + L.o_ioff;
  int32_t base[kDbnHoist];
#pragma unroll
  for (int l = 0; l < kDbnHoist; ++l) {
    base[l] = 0;
    if (l < L.n_prev) {
      const int f = prev[l];
      base[l] = voff[f] + s.cl[f] + xoff[f * L.J + x];
    }
  }
  for (int i = 0; i < L.S; ++i) {
    double p = s.msg[i];
#pragma unroll
    for (int l = 0; l < kDbnHoist; ++l)
      if (l < L.n_prev) p *= s.a.val1[base[l] + ioff[l * L.S + i]];
    if (p > best) best = p, at = i;
  }
  *psi = at;
  return best;
}

// the maximum over the sequence's lanes and the lowest index that attains it: the larger value wins, the
// lower index on equality; the operation commutes, so every lane ends with the same pair
__device__ __forceinline__ void seg_argmax(double &v, int &at, int P) {
  for (int m = P >> 1; m > 0; m >>= 1) {
    const double ov = __shfl_xor(v, m, 64);
    const int oat = __shfl_xor(at, m, 64);
    if (ov > v || (ov == v && oat < at)) v = ov, at = oat;
  }
}

}  // namespace

__global__ __launch_bounds__(kDbnBlock) void k_dbn_viterbi(const DbnVitArgs va) {
  extern __shared__ double lds[];
  const DbnArgs &a = va.a;
  const DbnLayout &L = a.L;
  const int lane = (int)threadIdx.x, P = L.P, J = L.J, S = L.S, n = L.n;
  const int seg = lane / P;
  const int64_t seq = (int64_t)blockIdx.x * L.spw + seg;
  // a lane without a sequence computes on the first one's data and stores nothing
  const bool live = seg < L.spw && seq < a.B;
  const int sg = live ? seg : 0;
  int32_t *cl_all = reinterpret_cast<int32_t *>(lds + (size_t)L.spw * (J + 2 * S));
  uint8_t *ev_all = reinterpret_cast<uint8_t *>(cl_all + (size_t)L.spw * n);
  const Seq s = {a,
                 lds + (size_t)sg * J,
                 lds + (size_t)L.spw * J + (size_t)sg * S,
                 lds + (size_t)L.spw * (J + S) + (size_t)sg * S,
                 cl_all + (size_t)sg * n,
                 ev_all + (size_t)sg * 2 * n,
                 live ? seq : 0,
                 a.row0 + (live ? seq : 0),
                 lane % P,
                 live};
  int32_t *argx = reinterpret_cast<int32_t *>(s.beta);
  const int xl = s.xl, T1 = a.T1;
  const int32_t *card = a.tab + L.o_card, *clamp = a.tab + L.o_clamp, *xstride = a.tab + L.o_xstride,
                *fr = a.tab + L.o_free, *xperm = a.tab + L.o_xperm;
  const int64_t orow = va.row0_out + s.seq;

  // ------------------------------------------------------------------ forward
  double lm = 0.0;
  bool dead = false;
  int xbest = 0;
  for (int t = 0; t < T1; ++t) {
    load_ev(s, t);
    __syncthreads();
    compute_cl(s, t ? 1 : 0);
    if (live)
      for (int v = xl; v < n; v += P)
        if (clamp[v]) va.path[((int64_t)t * n + v) * va.ld_out + orow] = s.ev[n + v];
    if (t)
      for (int i = xl; i < S; i += P) {
        // the x of a group ascend along r: the first maximum is the lowest x
        int at = xperm[i * L.R];
        double m = s.A[at];
        for (int r = 1; r < L.R; ++r) {
          const int x = xperm[i * L.R + r];
          const double v = s.A[x];
          if (v > m) m = v, at = x;
        }
        if (live) s.msg[i] = m, argx[i] = at;
      }
    __syncthreads();
    uint16_t *bp = t ? va.bp + ((int64_t)(t - 1) * a.B + s.seq) * J : nullptr;
    double best = -1.0;
    int at = 0x7fffffff;
    for (int x = xl; x < J; x += P) {
      double v = 0.0;
      int from = 0;
      if (consistent(s, x)) {
        v = local_factor(s, x, t == 0);
        if (t) {
          int psi;
          v *= carried_max(s, x, &psi);
          from = argx[psi];
        }
      }
      if (live) {
        s.A[x] = v;
        if (t) bp[x] = (uint16_t)from;
      }
      if (v > best) best = v, at = x;
    }
    seg_argmax(best, at, P);
    const double c = best;
    if (live)
      for (int x = xl; x < J; x += P) s.A[x] /= c;
    if (!(c > 0.0)) dead = true;
    lm += log(c);
    xbest = at;
    __syncthreads();
  }
  if (!live) return;
  if (xl == 0) {
    if (a.loglik) a.loglik[seq] = dead ? -INFINITY : lm;
    if (a.impossible) a.impossible[seq] = dead ? 1 : 0;
  }

  // ------------------------------------------------------------------ backtrack
  // (no barrier and no LDS from here on: the lanes of a sequence walk the same states)
  int x = xbest;
  for (int t = T1 - 1; t >= 0; --t) {
    for (int j = xl; j < L.n_free; j += P) {
      const int v = fr[j];
      va.path[((int64_t)t * n + v) * va.ld_out + orow] = dead ? (uint8_t)PGM_EV_MISSING : (uint8_t)(x / xstride[v] % card[v]);
    }
    if (t && !dead) x = va.bp[((int64_t)(t - 1) * a.B + seq) * J + x];
  }
}

// ---------------------------------------------------------------------------------------------- expected counts
// k_dbn_estep — the E-step of Baum-Welch (include/pgmhip.h "dynamic Bayesian networks: expected counts").  The
// plan, the mapping and a sequence's LDS are k_dbn's; the forward pass is k_dbn's smoother's, statement by
// statement (loglik and impossible are the same bits), and so are gamma and the beta update of the backward
// pass.  What is new is between them: every term of gamma, and of the carried sum inside it, is added to the
// entry of the count tables that the factor was read from.  tile: the fp64 copy of both table sets in LDS
// (tables0, then tables1), or null: every add goes to global memory.
struct DbnEstepArgs {
  DbnArgs a;  // filter and smooth unused; scratch as for a smoother
  double *tab0, *tab1;
  int64_t groups;   // groups of spw sequences
  int64_t tile_at;  // doubles into LDS where the tile begins; < 0: no tile
  int32_t total0, total1;
};

namespace {

// TILE is a template argument so that the tile's adds are LDS instructions, not flat ones
template <bool TILE>
struct Counts {
  double *tile, *tab0, *tab1;
  int32_t total0;
  __device__ __forceinline__ void add(int set, int32_t at, double w) const {
    if constexpr (TILE)
      atomicAdd(&tile[(set ? total0 : 0) + at], w);
    else
      atomicAdd(&(set ? tab1 : tab0)[at], w);
  }
};

// the adds of slice t >= 1 at x' for the families with a free slice-t parent: xi(i, x') / gs, a term of xi
// built as the matching term of carried() and then as gamma is (local, / c, * beta)
template <bool TILE>
__device__ __forceinline__ void add_prev(const Seq &s, const Counts<TILE> &k, int x, double local, double c, double beta, double gs) {
  const DbnLayout &L = s.a.L;
  const int32_t *voff = s.a.tab + L.o_voff[1], *xoff = s.a.tab + L.o_xoff[1], *prev = s.a.tab + L.o_prev,
                *ioff = s.a.tab + L.o_ioff;
  if (L.n_prev > kDbnHoist) {
    for (int i = 0; i < L.S; ++i) {
      const double m = s.msg[i];
      if (m == 0.0) continue;
      const double xi = local * trans_factor(s, i, x, m) / c * beta;
      if (xi == 0.0) continue;
      const double w = xi / gs;
      for (int l = 0; l < L.n_prev; ++l) {
        const int f = prev[l];
        k.add(1, voff[f] + s.cl[f] + xoff[f * L.J + x] + ioff[l * L.S + i], w);
      }
    }
    return;
  }
  int32_t base[kDbnHoist];
#pragma unroll
  for (int l = 0; l < kDbnHoist; ++l) {
    base[l] = 0;
    if (l < L.n_prev) {
      const int f = prev[l];
      base[l] = voff[f] + s.cl[f] + xoff[f * L.J + x];
    }
  }
  for (int i = 0; i < L.S; ++i) {
    double p = s.msg[i];
    if (p == 0.0) continue;
#pragma unroll
    for (int l = 0; l < kDbnHoist; ++l)
      if (l < L.n_prev) p *= s.a.val1[base[l] + ioff[l * L.S + i]];
    const double xi = local * p / c * beta;
    if (xi == 0.0) continue;
    const double w = xi / gs;
#pragma unroll
    for (int l = 0; l < kDbnHoist; ++l)
      if (l < L.n_prev) k.add(1, base[l] + ioff[l * L.S + i], w);
  }
}

}  // namespace

template <bool TILE>
__global__ __launch_bounds__(kDbnBlock) void k_dbn_estep(const DbnEstepArgs ea) {
  extern __shared__ double lds[];
  const DbnArgs &a = ea.a;
  const DbnLayout &L = a.L;
  const int lane = (int)threadIdx.x, P = L.P, J = L.J, S = L.S, n = L.n;
  const int seg = lane / P;
  const int32_t total = ea.total0 + ea.total1;
  const Counts<TILE> k = {TILE ? lds + ea.tile_at : nullptr, ea.tab0, ea.tab1, ea.total0};
  if constexpr (TILE) {
    for (int32_t e = lane; e < total; e += kDbnBlock) k.tile[e] = 0.0;
    __syncthreads();
  }
  int32_t *cl_all = reinterpret_cast<int32_t *>(lds + (size_t)L.spw * (J + 2 * S));
  uint8_t *ev_all = reinterpret_cast<uint8_t *>(cl_all + (size_t)L.spw * n);
  const int32_t *ix = a.tab + L.o_ix, *xperm = a.tab + L.o_xperm;
  const int T1 = a.T1;

  for (int64_t grp = blockIdx.x; grp < ea.groups; grp += gridDim.x) {
    const int64_t seq = grp * L.spw + seg;
    // a lane without a sequence computes on the first one's data and stores nothing
    const bool live = seg < L.spw && seq < a.B;
    const int sg = live ? seg : 0;
    const Seq s = {a,
                   lds + (size_t)sg * J,
                   lds + (size_t)L.spw * J + (size_t)sg * S,
                   lds + (size_t)L.spw * (J + S) + (size_t)sg * S,
                   cl_all + (size_t)sg * n,
                   ev_all + (size_t)sg * 2 * n,
                   live ? seq : grp * L.spw,
                   a.row0 + (live ? seq : grp * L.spw),
                   lane % P,
                   live};
    const int xl = s.xl;
    double *scr = a.scratch + s.seq * T1 * (S + 1);

    // ---------------------------------------------------------------- forward (k_dbn's, with scratch)
    double ll = 0.0;
    bool dead = false;
    for (int t = 0; t < T1; ++t) {
      load_ev(s, t);
      __syncthreads();
      compute_cl(s, t ? 1 : 0);
      if (t)
        for (int i = xl; i < S; i += P) {
          double m = 0.0;
          for (int r = 0; r < L.R; ++r) m += s.A[xperm[i * L.R + r]];
          if (live) {
            s.msg[i] = m;
            scr[(t - 1) * (S + 1) + i] = m;
          }
        }
      __syncthreads();
      double part = 0.0;
      for (int x = xl; x < J; x += P) {
        double v = 0.0;
        if (consistent(s, x)) {
          v = local_factor(s, x, t == 0);
          if (t) v *= carried(s, x);
        }
        if (live) s.A[x] = v;
        part += v;
      }
      const double c = seg_sum(part, P);
      if (live)
        for (int x = xl; x < J; x += P) s.A[x] /= c;
      if (!(c > 0.0)) dead = true;
      ll += log(c);
      if (live && xl == 0) scr[t * (S + 1) + S] = c;
      __syncthreads();
    }
    if (live && xl == 0) {
      if (a.loglik) a.loglik[seq] = dead ? -INFINITY : ll;
      if (a.impossible) a.impossible[seq] = dead ? 1 : 0;
    }

    // ---------------------------------------------------------------- backward
    const bool counted = live && !dead;  // an impossible sequence adds nothing
    if (live)
      for (int i = xl; i < S; i += P) s.beta[i] = 1.0;
    for (int t = T1 - 1; t >= 0; --t) {
      load_ev(s, t);
      if (t && live)
        for (int i = xl; i < S; i += P) s.msg[i] = scr[(t - 1) * (S + 1) + i];
      const double c = scr[t * (S + 1) + S];
      __syncthreads();
      compute_cl(s, t ? 1 : 0);
      __syncthreads();
      // gamma_t, as k_dbn builds it
      double part = 0.0;
      for (int x = xl; x < J; x += P) {
        double g = 0.0;
        if (consistent(s, x)) {
          g = local_factor(s, x, t == 0);
          if (t) g *= carried(s, x);
          g = g / c * s.beta[ix[x]];
        }
        if (live) s.A[x] = g;
        part += g;
      }
      const double gs = seg_sum(part, P);
      // the adds: a lane's own x; g = 0 is an x that contradicts the evidence, or has no mass (then every term
      // of its carried sum is 0 too: the terms are not negative)
      if (counted)
        for (int x = xl; x < J; x += P) {
          const double g = s.A[x];
          if (g == 0.0) continue;
          const double w = g / gs;
          if (!t) {
            const int32_t *voff = a.tab + L.o_voff[0], *xoff = a.tab + L.o_xoff[0];
            for (int f = 0; f < n; ++f) k.add(0, voff[f] + s.cl[f] + xoff[f * J + x], w);
          } else {
            const int32_t *voff = a.tab + L.o_voff[1], *xoff = a.tab + L.o_xoff[1], *cur = a.tab + L.o_cur;
            for (int l = 0; l < L.n_cur; ++l) {
              const int f = cur[l];
              k.add(1, voff[f] + s.cl[f] + xoff[f * J + x], w);
            }
            if (L.n_prev) add_prev(s, k, x, local_factor(s, x, false), c, s.beta[ix[x]], gs);
          }
        }
      if (!t) break;
      // beta_t-1, as k_dbn builds it (a lane rewrites the A[x] it has just read: no barrier between)
      for (int x = xl; x < J; x += P) {
        const double w = consistent(s, x) ? local_factor(s, x, false) * s.beta[ix[x]] / c : 0.0;
        if (live) s.A[x] = w;
      }
      __syncthreads();
      for (int i = xl; i < S; i += P) {
        double b = 0.0;
        for (int x = 0; x < J; ++x) {
          const double w = s.A[x];
          if (w != 0.0) b += trans_factor(s, i, x, w);
        }
        if (live) s.beta[i] = b;
      }
      __syncthreads();
    }
    __syncthreads();  // the next group's codes go where this one's adds have read
  }
  if constexpr (TILE) {
    __syncthreads();
    for (int32_t e = lane; e < total; e += kDbnBlock) {
      const double v = k.tile[e];
      if (v != 0.0) atomicAdd(e < ea.total0 ? &ea.tab0[e] : &ea.tab1[e - ea.total0], v);
    }
  }
}

extern "C" {

int pgm_dbn_plan_destroy(void *plan) { return pgm_plan_destroy<DbnHandle>(plan); }

int pgm_dbn_run(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int32_t n_slices,
                const double *values0, const double *values1, double *filter, double *smooth, double *loglik,
                uint8_t *impossible, double *scratch, int64_t scratch_bytes, void *stream) {
  DbnHandle *h = static_cast<DbnHandle *>(plan);
  bool launch = false;
  const int st = dbn_run_check(h, codes, n_cols, ld, row0, n_rows, n_slices, values0, values1, filter, smooth, loglik, scratch,
                               scratch_bytes, &launch);
  if (st != PGM_OK || !launch) return st;
  const DbnPlan &p = h->p;
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_tab, p.tab)};
  int up = h->dev.use(kHipDevOps, base);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  // above 64 KiB of dynamic LDS a kernel has to be told so before the launch
  if (p.lds_bytes > 65536)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dbn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)p.lds_bytes));
  DbnArgs a = {};
  a.L = p.L, a.tab = h->d_tab, a.codes = codes, a.ld = ld, a.row0 = row0, a.B = n_rows, a.T1 = n_slices;
  a.val0 = values0, a.val1 = values1, a.filter = filter, a.smooth = smooth, a.loglik = loglik, a.scratch = scratch;
  a.impossible = impossible, a.err = h->dev.flag();
  const int64_t blocks = (n_rows + p.L.spw - 1) / p.L.spw;
  hipLaunchKernelGGL(k_dbn, dim3((unsigned)blocks), dim3(kDbnBlock), (size_t)p.lds_bytes, S(stream), a);
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad)
    return pgmi_fail(PGM_EINVAL, "dbn_run: a clamped cell is missing, or a code is >= its node's cardinality");
  return PGM_OK;
}

int pgm_dbn_viterbi(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int32_t n_slices,
                    const double *values0, const double *values1, uint8_t *path, int64_t ld_out, int64_t row0_out,
                    double *logmap, uint8_t *impossible, void *scratch, int64_t scratch_bytes, void *stream) {
  DbnHandle *h = static_cast<DbnHandle *>(plan);
  bool launch = false;
  const int st = dbn_viterbi_check(h, codes, n_cols, ld, row0, n_rows, n_slices, values0, values1, path, ld_out, row0_out, logmap,
                                   scratch, scratch_bytes, &launch);
  if (st != PGM_OK || !launch) return st;
  const DbnPlan &p = h->p;
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_tab, p.tab)};
  int up = h->dev.use(kHipDevOps, base);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  // the attribute is a kernel's own: k_dbn having been told does not cover this one
  if (p.lds_bytes > 65536)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dbn_viterbi), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)p.lds_bytes));
  DbnVitArgs va = {};
  DbnArgs &a = va.a;
  a.L = p.L, a.tab = h->d_tab, a.codes = codes, a.ld = ld, a.row0 = row0, a.B = n_rows, a.T1 = n_slices;
  a.val0 = values0, a.val1 = values1, a.loglik = logmap, a.impossible = impossible, a.err = h->dev.flag();
  va.path = path, va.ld_out = ld_out, va.row0_out = row0_out, va.bp = static_cast<uint16_t *>(scratch);
  const int64_t blocks = (n_rows + p.L.spw - 1) / p.L.spw;
  hipLaunchKernelGGL(k_dbn_viterbi, dim3((unsigned)blocks), dim3(kDbnBlock), (size_t)p.lds_bytes, S(stream), va);
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad)
    return pgmi_fail(PGM_EINVAL, "dbn_viterbi: a clamped cell is missing, or a code is >= its node's cardinality");
  return PGM_OK;
}

int pgm_dbn_estep(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int32_t n_slices,
                  const double *values0, const double *values1, double *tables0, double *tables1, double *loglik,
                  uint8_t *impossible, double *scratch, int64_t scratch_bytes, uint32_t flags, void *stream) {
  DbnHandle *h = static_cast<DbnHandle *>(plan);
  bool launch = false;
  const int st = dbn_estep_check(h, codes, n_cols, ld, row0, n_rows, n_slices, values0, values1, tables0, tables1, loglik, scratch,
                                 scratch_bytes, flags, &launch);
  if (st != PGM_OK || !launch) return st;
  const DbnPlan &p = h->p;
  const DbnEstepGeom g = dbn_estep_geom(p, flags);
  const pgmdev::Slot base[] = {pgmdev::upload(h->d_tab, p.tab)};
  int up = h->dev.use(kHipDevOps, base);
  if (up == PGM_OK) up = flag_reset(h->dev, stream);
  if (up != PGM_OK) return up;
  // the attribute is a kernel's own, and this one's LDS is the plan's plus the tile
  void (*const kernel)(DbnEstepArgs) = g.tile ? k_dbn_estep<true> : k_dbn_estep<false>;
  if (g.lds_bytes > 65536)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)g.lds_bytes));
  DbnEstepArgs ea = {};
  DbnArgs &a = ea.a;
  a.L = p.L, a.tab = h->d_tab, a.codes = codes, a.ld = ld, a.row0 = row0, a.B = n_rows, a.T1 = n_slices;
  a.val0 = values0, a.val1 = values1, a.loglik = loglik, a.scratch = scratch, a.impossible = impossible, a.err = h->dev.flag();
  ea.tab0 = tables0, ea.tab1 = tables1, ea.total0 = (int32_t)p.total[0], ea.total1 = (int32_t)p.total[1];
  ea.groups = (n_rows + p.L.spw - 1) / p.L.spw;
  ea.tile_at = g.tile ? g.tile_at : -1;
  const int64_t blocks = g.tile ? std::min(ea.groups, g.max_blocks) : ea.groups;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kDbnBlock), (size_t)g.lds_bytes, S(stream), ea);
  int32_t bad = 0;
  const int rd = flag_read(h->dev, stream, &bad);
  if (rd != PGM_OK) return rd;
  if (bad)
    return pgmi_fail(PGM_EINVAL, "dbn_estep: a clamped cell is missing, or a code is >= its node's cardinality");
  return PGM_OK;
}
}

// pgmxs.hip — the highest-scoring DAG under a decomposable score by dynamic programming over the subset lattice
// (Silander and Myllymaki), on the device (gfx950): k_xs_fill / k_xs_scatter (the family scores into their cells),
// k_xs_zeta (the max-zeta transform of every node's row: butterfly passes through an LDS tile, the low bits in one
// launch, the high bits several to a launch on a strided tile), k_xs_sink (the best-sink recurrence: a workgroup owns
// the sets that share their high bits, walks the popcount layers of the low bits in LDS and is launched by the popcount
// of the high bits), k_xs_readback (one wave follows the sinks down from the full set) and the C-ABI (pgm_xs_run,
// pgm_xs_set_tiling, pgm_xs_destroy).  The contract is include/pgmhip.h "Exact structure search"; the host side
// (tiling, lists, launch counts, checks, pgm_xs_create, pgm_xs_info) is pgmxs_plan.cpp.  Compares and single fp64
// adds only: no matrix instruction has anything to multiply, no atomic, and launch order alone carries the
// dependencies (no grid-wide barrier, no waiting on memory).
//
// On the same handle, lists and tiling, the exact edge posteriors (include/pgmhip.h "Exact edge posteriors";
// pgm_xs_posterior): the lattice with a log-sum-exp where the search has a maximum.  k_xsp_zeta (subset and superset
// sums of 8-byte cells through the same LDS tiles), k_xsp_paths (the forward and backward path sums F and B by popcount
// layers), k_xsp_gamma and k_xsp_edges (a few rows of gamma at a time, and a fixed-order reduction of the listed
// families into a column of the n x n matrix).  fp64 exp and log1p; still no matrix instruction and no atomic.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pgm_hip_common.h"
#include "pgm_xs.h"

// a set with bit v squeezed out: the index of S (v not in S) in node v's row
__device__ __forceinline__ uint32_t xs_squeeze(uint32_t S, uint32_t v) {
  return (S & ((1u << v) - 1u)) | ((S >> (v + 1u)) << v);
}

// The total order of step 1: the larger score, then the fewer parents, then the smaller mask.  A cell without a
// family holds (-inf, PGM_XS_NONE): 32 bits set, so it loses every tie but the one with itself.
__device__ __forceinline__ bool xs_better(double sa, uint32_t ma, double sb, uint32_t mb) {
  if (sa != sb) return sa > sb;
  const int pa = __popc(ma), pb = __popc(mb);
  return pa != pb ? pa < pb : ma < mb;
}

__global__ __launch_bounds__(kXsBlock) void k_xs_fill(double *q, uint32_t *a, int64_t cells) {
  const int64_t step = (int64_t)gridDim.x * kXsBlock;
  for (int64_t i = (int64_t)blockIdx.x * kXsBlock + threadIdx.x; i < cells; i += step) q[i] = -INFINITY, a[i] = kXsNone;
}

// a family has one cell and a cell one family (the host rejected duplicates): plain stores
__global__ __launch_bounds__(kXsBlock) void k_xs_scatter(double *q, uint32_t *a, const uint32_t *cell,
                                                         const uint32_t *mask, const double *score, int32_t n_fam) {
  const int32_t f = (int32_t)(blockIdx.x * kXsBlock + threadIdx.x);
  if (f < n_fam) q[cell[f]] = score[f], a[cell[f]] = mask[f];
}

struct XsZetaArgs {
  double *q;
  uint32_t *a;
  int32_t W, Lz;  // bits of a row's index; log2 of the tile
  XsTrip t;
};

// Workgroup b: tile b mod 2^(W - Lz) of row b >> (W - Lz).  LDS cell i is row cell base | (i >> c) << b0 | (i mod 2^c):
// the tile's bits c .. Lz - 1 stand for the row's bits b0 .. b0 + hh - 1.  The bits that number the tile are the row's
// other bits, c .. b0 - 1 and b0 + hh .. W - 1.  A pass over LDS bit j pairs cell lo (bit j clear) with lo | 2^j; the
// pairs of a pass are disjoint, so one barrier between passes is all the order there is.
__global__ __launch_bounds__(kXsBlock) void k_xs_zeta(XsZetaArgs z) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *val = reinterpret_cast<double *>(smem);
  uint32_t *msk = reinterpret_cast<uint32_t *>(val + (1u << z.Lz));
  const uint32_t tid = threadIdx.x, cells = 1u << z.Lz, tile_bits = (uint32_t)(z.W - z.Lz);
  const uint32_t v = blockIdx.x >> tile_bits, f = blockIdx.x & ((1u << tile_bits) - 1u);
  const uint32_t c = (uint32_t)z.t.c, b0 = (uint32_t)z.t.b0, mid = b0 - c;
  const uint32_t base = ((f & ((1u << mid) - 1u)) << c) | ((f >> mid) << (b0 + (uint32_t)z.t.hh));
  double *q = z.q + ((size_t)v << z.W);
  uint32_t *a = z.a + ((size_t)v << z.W);
  for (uint32_t i = tid; i < cells; i += kXsBlock) {
    const uint32_t T = base | ((i >> c) << b0) | (i & ((1u << c) - 1u));
    val[i] = q[T], msk[i] = a[T];
  }
  __syncthreads();
  for (uint32_t j = (uint32_t)z.t.p0; j < (uint32_t)z.t.p1; ++j) {
    for (uint32_t p = tid; p < cells >> 1; p += kXsBlock) {
      const uint32_t lo = ((p >> j) << (j + 1u)) | (p & ((1u << j) - 1u)), hi = lo | (1u << j);
      const double s = val[lo];
      const uint32_t m = msk[lo];
      if (xs_better(s, m, val[hi], msk[hi])) val[hi] = s, msk[hi] = m;
    }
    __syncthreads();
  }
  for (uint32_t i = tid; i < cells; i += kXsBlock) {
    const uint32_t T = base | ((i >> c) << b0) | (i & ((1u << c) - 1u));
    q[T] = val[i], a[T] = msk[i];
  }
}

struct XsSinkArgs {
  const double *q;
  double *r;
  uint32_t *k;
  const uint32_t *hi_list;
  const uint16_t *lo_list;
  int32_t W, Ls, hi0;  // hi0: where this launch's popcount starts in hi_list
  int32_t lo_off[kXsMaxTile + 2];
};

// Workgroup b owns the 2^Ls sets whose high part is hi_list[hi0 + b] and keeps their R in LDS.  Layer by layer of
// the low part's popcount: a set's candidates are its members v in ascending order, R[S \ v] from LDS for a low v
// and from memory for a high one (an earlier launch wrote it), plus Q[v][S \ v]: one add, and a strict compare so the
// smaller v keeps a tie.  A set whose candidates are all -inf keeps its smallest member.
__global__ __launch_bounds__(kXsBlock) void k_xs_sink(XsSinkArgs s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *R = reinterpret_cast<double *>(smem);
  uint8_t *K = reinterpret_cast<uint8_t *>(R + (1u << s.Ls));
  const uint32_t tid = threadIdx.x, Ls = (uint32_t)s.Ls;
  const uint32_t base = s.hi_list[s.hi0 + (int32_t)blockIdx.x] << Ls;
  for (uint32_t layer = 0; layer <= Ls; ++layer) {
    for (int32_t e = s.lo_off[layer] + (int32_t)tid; e < s.lo_off[layer + 1]; e += kXsBlock) {
      const uint32_t l = s.lo_list[e], S = base | l;
      if (S == 0) {
        R[0] = 0.0, K[0] = 0xff;
        continue;
      }
      double best = -INFINITY;
      uint32_t win = (uint32_t)__ffs((int)S) - 1u;
      for (uint32_t rem = S; rem; rem &= rem - 1u) {
        const uint32_t v = (uint32_t)__ffs((int)rem) - 1u, prev = S ^ (1u << v);
        const double before = v < Ls ? R[l ^ (1u << v)] : s.r[prev];
        const double cand = before + s.q[((size_t)v << s.W) + xs_squeeze(prev, v)];
        if (cand > best) best = cand, win = v;
      }
      R[l] = best, K[l] = (uint8_t)win;
    }
    __syncthreads();
  }
  for (uint32_t i = tid; i < (1u << Ls); i += kXsBlock) {
    s.r[base + i] = R[i];
    s.k[base + i] = K[i] == 0xff ? kXsNone : (uint32_t)K[i];
  }
}

// One wave; its first lane walks the n steps of step 3.  *flag: R[V] = -inf, no DAG meets the constraints (the
// record is then the walk along the smallest members, and holds PGM_XS_NONE where a node has no family).
__global__ __launch_bounds__(64) void k_xs_readback(const uint32_t *a, const double *r, const uint32_t *k, int32_t n,
                                                    XsRecord *rec, int32_t *flag) {
  if (threadIdx.x != 0) return;
  uint32_t S = (1u << n) - 1u;
  rec->score = r[S];
  if (r[S] == -INFINITY) *flag = 1;
  for (int32_t i = 0; i < n; ++i) {
    const uint32_t v = k[S];
    S ^= 1u << v;
    rec->parents[v] = a[((size_t)v << (n - 1)) + xs_squeeze(S, v)];
    rec->order[i] = (int32_t)v;
  }
  for (int32_t i = n; i < PGM_XS_MAX_NODES; ++i) rec->parents[i] = kXsNone, rec->order[i] = -1;
}

// ---------------------------------------------------------------------------- the handle's device side
// The base serves both entry points (the value tables, the lists, the staging of a chunk); stage 0 is the winners of a
// search, stage 1 what only a posterior needs.
static int xs_use(XsHandle *h, bool posterior) {
  const XsPlan &p = h->p;
  const pgmdev::Slot base[] = {pgmdev::scratch(h->d_q, (size_t)p.q_cells),     pgmdev::scratch(h->d_r, (size_t)p.r_cells),
                               pgmdev::upload(h->d_hi_list, p.hi_list),        pgmdev::upload(h->d_lo_list, p.lo_list),
                               pgmdev::scratch(h->d_fam_cell, (size_t)kXsChunk), pgmdev::scratch(h->d_fam_mask, (size_t)kXsChunk),
                               pgmdev::scratch(h->d_fam_score, (size_t)kXsChunk), pgmdev::scratch(h->d_rec, 1)};
  if (posterior) {
    const pgmdev::Slot post[] = {pgmdev::scratch(h->d_b, (size_t)p.r_cells), pgmdev::scratch(h->d_g, (size_t)p.post_rows << p.W),
                                 pgmdev::scratch(h->d_post, (size_t)(p.n * p.n + p.n + 2))};
    return h->dev.use(kHipDevOps, base, 1, post);
  }
  const pgmdev::Slot search[] = {pgmdev::scratch(h->d_a, (size_t)p.q_cells), pgmdev::scratch(h->d_k, (size_t)p.r_cells)};
  return h->dev.use(kHipDevOps, base, 0, search);
}

// the events of a run (start, then the end of each phase), made on the handle's device by the first run there
static int xs_events(XsHandle *h) {
  if (h->ev_device == h->dev.device()) return PGM_OK;
  for (void *&e : h->ev) {
    if (e) (void)hipEventDestroy(static_cast<hipEvent_t>(e));
    e = nullptr;
    hipEvent_t made;
    HIP_TRY(hipEventCreate(&made));
    e = made;
  }
  h->ev_device = h->dev.device();
  return PGM_OK;
}
static int xs_mark(XsHandle *h, int i, void *stream) {
  HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(h->ev[i]), S(stream)));
  return PGM_OK;
}

// Everything a run puts on the stream, in order.  Nothing here waits: the caller synchronises the stream whatever
// this returns, so the host vectors and *rec outlive every copy that was enqueued.
static int xs_enqueue(XsHandle *h, const std::vector<uint32_t> &cell, const std::vector<uint32_t> &mask,
                      const std::vector<double> &score, double *values, uint32_t *winners, XsRecord *rec, void *stream) {
  const XsPlan &p = h->p;
  if (const int e = flag_reset(h->dev, stream)) return e;
  if (const int e = xs_mark(h, 0, stream)) return e;

  // the scatter: every cell to (-inf, none), then the families a chunk at a time through the staging buffers (the
  // copies and the launches are in stream order)
  const unsigned fill_blocks = (unsigned)std::min<int64_t>((p.q_cells + kXsBlock - 1) / kXsBlock, 65536);
  hipLaunchKernelGGL(k_xs_fill, dim3(fill_blocks), dim3(kXsBlock), 0, S(stream), h->d_q, h->d_a, p.q_cells);
  HIP_TRY(hipGetLastError());
  for (size_t f0 = 0; f0 < cell.size(); f0 += kXsChunk) {
    const size_t m = std::min<size_t>(kXsChunk, cell.size() - f0);
    HIP_TRY(hipMemcpyAsync(h->d_fam_cell, cell.data() + f0, 4 * m, hipMemcpyHostToDevice, S(stream)));
    HIP_TRY(hipMemcpyAsync(h->d_fam_mask, mask.data() + f0, 4 * m, hipMemcpyHostToDevice, S(stream)));
    HIP_TRY(hipMemcpyAsync(h->d_fam_score, score.data() + f0, 8 * m, hipMemcpyHostToDevice, S(stream)));
    hipLaunchKernelGGL(k_xs_scatter, dim3((unsigned)((m + kXsBlock - 1) / kXsBlock)), dim3(kXsBlock), 0, S(stream), h->d_q,
                       h->d_a, h->d_fam_cell, h->d_fam_mask, h->d_fam_score, (int32_t)m);
    HIP_TRY(hipGetLastError());
  }
  if (const int e = xs_mark(h, 1, stream)) return e;

  // the max-zeta transform: the low bits, then the high bits h at a time
  for (const XsTrip &t : p.trips) {
    XsZetaArgs z = {h->d_q, h->d_a, p.W, p.Lz, t};
    hipLaunchKernelGGL(k_xs_zeta, dim3((unsigned)(p.q_cells >> p.Lz)), dim3(kXsBlock), (size_t)xs_zeta_lds(p), S(stream), z);
    HIP_TRY(hipGetLastError());
  }
  if (const int e = xs_mark(h, 2, stream)) return e;

  // the sinks, by the popcount of the high part
  XsSinkArgs s = {};
  s.q = h->d_q, s.r = h->d_r, s.k = h->d_k, s.hi_list = h->d_hi_list, s.lo_list = h->d_lo_list, s.W = p.W, s.Ls = p.Ls;
  std::copy(p.lo_off, p.lo_off + kXsMaxTile + 2, s.lo_off);
  for (int32_t c = 0; c + 1 < (int32_t)p.hi_off.size(); ++c) {
    s.hi0 = p.hi_off[(size_t)c];
    const unsigned blocks = (unsigned)(p.hi_off[(size_t)c + 1] - s.hi0);
    hipLaunchKernelGGL(k_xs_sink, dim3(blocks), dim3(kXsBlock), (size_t)xs_sink_lds(p), S(stream), s);
    HIP_TRY(hipGetLastError());
  }
  if (const int e = xs_mark(h, 3, stream)) return e;

  hipLaunchKernelGGL(k_xs_readback, dim3(1), dim3(64), 0, S(stream), h->d_a, h->d_r, h->d_k, p.n, h->d_rec, h->dev.flag());
  HIP_TRY(hipGetLastError());
  if (values) {
    HIP_TRY(hipMemcpyAsync(values, h->d_q, 8 * (size_t)p.q_cells, hipMemcpyDeviceToDevice, S(stream)));
    HIP_TRY(hipMemcpyAsync(values + p.q_cells, h->d_r, 8 * (size_t)p.r_cells, hipMemcpyDeviceToDevice, S(stream)));
  }
  if (winners) {
    HIP_TRY(hipMemcpyAsync(winners, h->d_a, 4 * (size_t)p.q_cells, hipMemcpyDeviceToDevice, S(stream)));
    HIP_TRY(hipMemcpyAsync(winners + p.q_cells, h->d_k, 4 * (size_t)p.r_cells, hipMemcpyDeviceToDevice, S(stream)));
  }
  HIP_TRY(hipMemcpyAsync(rec, h->d_rec, sizeof *rec, hipMemcpyDeviceToHost, S(stream)));
  return PGM_OK;
}

// ---------------------------------------------------------------------------- edge posteriors: the same lattice in log space
// include/pgmhip.h "Exact edge posteriors".  log(e^a + e^b).  |a - b| is +inf when one operand is -inf and NaN when
// both are: either way the larger operand is the answer, and no NaN leaves.  Scores are finite or -inf (the host
// rejected +inf and NaN), so +inf never enters.
__device__ __forceinline__ double xsp_lse2(double a, double b) {
  const double m = fmax(a, b), d = fabs(a - b);
  if (!(d < INFINITY)) return m;
  return m + log1p(exp(-d));
}

__global__ __launch_bounds__(kXsBlock) void k_xsp_fill(double *q, int64_t cells) {
  const int64_t step = (int64_t)gridDim.x * kXsBlock;
  for (int64_t i = (int64_t)blockIdx.x * kXsBlock + threadIdx.x; i < cells; i += step) q[i] = -INFINITY;
}

__global__ __launch_bounds__(kXsBlock) void k_xsp_scatter(double *q, const uint32_t *cell, const double *score, uint32_t n_fam) {
  const uint32_t step = gridDim.x * kXsBlock;
  for (uint32_t f = blockIdx.x * kXsBlock + threadIdx.x; f < n_fam; f += step) q[cell[f]] = score[f];
}

struct XspZetaArgs {
  double *g;      // rows of 2^W cells; the grid covers whole rows
  int32_t W, Lz;  // bits of a row's index; log2 of the tile
  int32_t up;     // 0: subset sums, hi = lse2(hi, lo); 1: superset sums, lo = lse2(lo, hi)
  XsTrip t;
};

// k_xs_zeta's tile and passes (the comment there) on a value alone, 8 bytes a cell.  A pass reads both cells of a pair
// and writes one of them; pairs are disjoint, and the passes over the row's bits come in ascending order whatever the
// tiling, so a cell sees the same operands in the same order under every tiling.
__global__ __launch_bounds__(kXsBlock) void k_xsp_zeta(XspZetaArgs z) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *val = reinterpret_cast<double *>(smem);
  const uint32_t tid = threadIdx.x, cells = 1u << z.Lz, tile_bits = (uint32_t)(z.W - z.Lz);
  const uint32_t v = blockIdx.x >> tile_bits, f = blockIdx.x & ((1u << tile_bits) - 1u);
  const uint32_t c = (uint32_t)z.t.c, b0 = (uint32_t)z.t.b0, mid = b0 - c;
  const uint32_t base = ((f & ((1u << mid) - 1u)) << c) | ((f >> mid) << (b0 + (uint32_t)z.t.hh));
  double *g = z.g + ((size_t)v << z.W);
  for (uint32_t i = tid; i < cells; i += kXsBlock) val[i] = g[base | ((i >> c) << b0) | (i & ((1u << c) - 1u))];
  __syncthreads();
  for (uint32_t j = (uint32_t)z.t.p0; j < (uint32_t)z.t.p1; ++j) {
    for (uint32_t p = tid; p < cells >> 1; p += kXsBlock) {
      const uint32_t lo = ((p >> j) << (j + 1u)) | (p & ((1u << j) - 1u)), hi = lo | (1u << j);
      const double x = xsp_lse2(val[lo], val[hi]);
      val[z.up ? lo : hi] = x;
    }
    __syncthreads();
  }
  for (uint32_t i = tid; i < cells; i += kXsBlock) g[base | ((i >> c) << b0) | (i & ((1u << c) - 1u))] = val[i];
}

struct XspPathArgs {
  const double *alpha;
  double *f, *b;
  const uint32_t *hi_list;
  const uint16_t *lo_list;
  int32_t W, Ls, hi0;
  uint32_t all;  // V
  int32_t lo_off[kXsMaxTile + 2];
};

// k_xs_sink's ownership and layers; blockIdx.y = 0 walks F and 1 walks B, which differ in the alpha cell a candidate
// reads: F takes alpha[v] at S \ v, B at V \ S.  The candidates come in ascending v under a running lse2 that starts
// at -inf, so a cell does not depend on the tile.  F and B of the sets one smaller come from LDS for a low v and
// from the table an earlier launch wrote for a high one.
__global__ __launch_bounds__(kXsBlock) void k_xsp_paths(XspPathArgs s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *R = reinterpret_cast<double *>(smem);
  const bool back = blockIdx.y != 0;
  double *tab = back ? s.b : s.f;
  const uint32_t tid = threadIdx.x, Ls = (uint32_t)s.Ls;
  const uint32_t base = s.hi_list[s.hi0 + (int32_t)blockIdx.x] << Ls;
  for (uint32_t layer = 0; layer <= Ls; ++layer) {
    for (int32_t e = s.lo_off[layer] + (int32_t)tid; e < s.lo_off[layer + 1]; e += kXsBlock) {
      const uint32_t l = s.lo_list[e], S = base | l;
      if (S == 0) {
        R[0] = 0.0;
        continue;
      }
      double acc = -INFINITY;
      for (uint32_t rem = S; rem; rem &= rem - 1u) {
        const uint32_t v = (uint32_t)__ffs((int)rem) - 1u, prev = S ^ (1u << v);
        const double before = v < Ls ? R[l ^ (1u << v)] : tab[prev];
        acc = xsp_lse2(acc, s.alpha[((size_t)v << s.W) + xs_squeeze(back ? s.all ^ S : prev, v)] + before);
      }
      R[l] = acc;
    }
    __syncthreads();
  }
  for (uint32_t i = tid; i < (1u << Ls); i += kXsBlock) tab[base + i] = R[i];
}

// gamma of the rows v0 .. v0 + rows - 1: cell (r, T) is F[S] + B[V \ S \ v] for v = v0 + r and S = T with a clear bit
// put in at v.  -inf + -inf is -inf; +inf does not occur.
__global__ __launch_bounds__(kXsBlock) void k_xsp_gamma(const double *f, const double *b, double *g, int32_t W, int32_t v0,
                                                       uint32_t all, int64_t cells) {
  const int64_t step = (int64_t)gridDim.x * kXsBlock;
  for (int64_t i = (int64_t)blockIdx.x * kXsBlock + threadIdx.x; i < cells; i += step) {
    const uint32_t v = (uint32_t)v0 + (uint32_t)(i >> W), T = (uint32_t)i & ((1u << W) - 1u);
    const uint32_t S = (T & ((1u << v) - 1u)) | ((T >> v) << (v + 1u));
    g[i] = f[S] + b[all ^ S ^ (1u << v)];
  }
}

struct XspEdgeArgs {
  const double *g, *f, *b;  // Gamma of the rows v0 ..; F and B
  const uint32_t *cell, *mask;
  const double *score;
  double *out;  // edge_post [n][n], mass [n], log_z [2]
  int32_t *flag;
  int32_t n, W, v0;
  uint32_t off[PGM_XS_MAX_NODES + 1];  // where each node's families start
};

// Workgroup b: column v = v0 + b of edge_post and mass[v].  Work-item l adds the terms of v's families l, l + 256, ...
// into one sum per possible parent and one for the mass (a family adds +0.0 to the parents it does not hold, which
// changes nothing); the indices are compile-time constants, so the 25 sums stay in registers.  A butterfly adds the
// 64 lanes of a wave, then the four wave totals are added in wave order: one fixed order, no atomic.
__global__ __launch_bounds__(kXsBlock) void k_xsp_edges(XspEdgeArgs e) {
  constexpr int kSums = PGM_XS_MAX_NODES + 1;
  __shared__ double part[kXsBlock / 64][kSums];
  const uint32_t tid = threadIdx.x, v = (uint32_t)e.v0 + blockIdx.x, all = (1u << e.n) - 1u;
  const double *g = e.g + ((size_t)blockIdx.x << e.W);
  const double log_z = e.f[all];
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (uint32_t i = e.off[v] + tid; i < e.off[v + 1]; i += kXsBlock) {
    const uint32_t m = e.mask[i];
    const double term = exp(e.score[i] + g[e.cell[i] - (v << e.W)] - log_z);
#pragma unroll
    for (int u = 0; u < PGM_XS_MAX_NODES; ++u) acc[u] += (m >> u & 1u) ? term : 0.0;
    acc[PGM_XS_MAX_NODES] += term;
  }
#pragma unroll
  for (int k = 0; k < kSums; ++k)
    for (int o = 32; o; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
  if ((tid & 63u) == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) part[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < (uint32_t)kSums) {
    double t = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    if (log_z == -INFINITY) t = NAN;  // no order admits a DAG
    if (tid < (uint32_t)e.n) e.out[tid * (uint32_t)e.n + v] = t;
    if (tid == PGM_XS_MAX_NODES) e.out[e.n * e.n + (int32_t)v] = t;
  }
  if (v == 0 && tid == 0) {
    e.out[e.n * e.n + e.n] = log_z, e.out[e.n * e.n + e.n + 1] = e.b[all];
    if (log_z == -INFINITY) *e.flag = 1;
  }
}

// Everything a posterior puts on the stream, in order; nothing here waits (xs_enqueue's rule).  `fam` is the call's
// device allocation of 16 bytes a family; `got` receives the outputs as k_xsp_edges lays them out.
static int xsp_enqueue(XsHandle *h, XspEdgeArgs e, char *fam, const std::vector<uint32_t> &cell,
                       const std::vector<uint32_t> &mask, const std::vector<double> &score, double *values, double *got,
                       void *stream) {
  const XsPlan &p = h->p;
  const size_t m = cell.size();
  const uint32_t all = (uint32_t)(p.r_cells - 1);
  auto blocks_for = [](int64_t items) { return (unsigned)std::min<int64_t>((items + kXsBlock - 1) / kXsBlock, 65536); };
  if (const int st = flag_reset(h->dev, stream)) return st;
  if (const int st = xs_mark(h, 0, stream)) return st;

  double *d_score = reinterpret_cast<double *>(fam);
  uint32_t *d_cell = reinterpret_cast<uint32_t *>(fam + 8 * m), *d_mask = d_cell + m;
  hipLaunchKernelGGL(k_xsp_fill, dim3(blocks_for(p.q_cells)), dim3(kXsBlock), 0, S(stream), h->d_q, p.q_cells);
  HIP_TRY(hipGetLastError());
  if (m) {
    HIP_TRY(hipMemcpyAsync(d_score, score.data(), 8 * m, hipMemcpyHostToDevice, S(stream)));
    HIP_TRY(hipMemcpyAsync(d_cell, cell.data(), 4 * m, hipMemcpyHostToDevice, S(stream)));
    HIP_TRY(hipMemcpyAsync(d_mask, mask.data(), 4 * m, hipMemcpyHostToDevice, S(stream)));
    hipLaunchKernelGGL(k_xsp_scatter, dim3(blocks_for((int64_t)m)), dim3(kXsBlock), 0, S(stream), h->d_q, d_cell, d_score, (uint32_t)m);
    HIP_TRY(hipGetLastError());
  }
  if (const int st = xs_mark(h, 1, stream)) return st;

  // alpha: the subset sums of every node's row
  const size_t lds = (size_t)xs_post_lds(p.Lz);
  for (const XsTrip &t : p.trips) {
    XspZetaArgs z = {h->d_q, p.W, p.Lz, 0, t};
    hipLaunchKernelGGL(k_xsp_zeta, dim3((unsigned)(p.q_cells >> p.Lz)), dim3(kXsBlock), lds, S(stream), z);
    HIP_TRY(hipGetLastError());
  }
  if (const int st = xs_mark(h, 2, stream)) return st;

  // F and B, by the popcount of the high part
  XspPathArgs s = {};
  s.alpha = h->d_q, s.f = h->d_r, s.b = h->d_b, s.hi_list = h->d_hi_list, s.lo_list = h->d_lo_list;
  s.W = p.W, s.Ls = p.Ls, s.all = all;
  std::copy(p.lo_off, p.lo_off + kXsMaxTile + 2, s.lo_off);
  for (int32_t c = 0; c + 1 < (int32_t)p.hi_off.size(); ++c) {
    s.hi0 = p.hi_off[(size_t)c];
    const unsigned blocks = (unsigned)(p.hi_off[(size_t)c + 1] - s.hi0);
    hipLaunchKernelGGL(k_xsp_paths, dim3(blocks, 2), dim3(kXsBlock), (size_t)xs_post_lds(p.Ls), S(stream), s);
    HIP_TRY(hipGetLastError());
  }
  if (const int st = xs_mark(h, 3, stream)) return st;

  // gamma, its superset sums and the edge sums, post_rows rows at a time through the one workspace
  e.g = h->d_g, e.f = h->d_r, e.b = h->d_b, e.cell = d_cell, e.mask = d_mask, e.score = d_score, e.out = h->d_post;
  e.flag = h->dev.flag(), e.n = p.n, e.W = p.W;
  for (int32_t v0 = 0; v0 < p.n; v0 += p.post_rows) {
    const int32_t rows = std::min(p.post_rows, p.n - v0);
    const int64_t cells = (int64_t)rows << p.W;
    hipLaunchKernelGGL(k_xsp_gamma, dim3(blocks_for(cells)), dim3(kXsBlock), 0, S(stream), h->d_r, h->d_b, h->d_g, p.W, v0, all, cells);
    HIP_TRY(hipGetLastError());
    for (const XsTrip &t : p.trips) {
      XspZetaArgs z = {h->d_g, p.W, p.Lz, 1, t};
      hipLaunchKernelGGL(k_xsp_zeta, dim3((unsigned)(cells >> p.Lz)), dim3(kXsBlock), lds, S(stream), z);
      HIP_TRY(hipGetLastError());
    }
    e.v0 = v0;
    hipLaunchKernelGGL(k_xsp_edges, dim3((unsigned)rows), dim3(kXsBlock), 0, S(stream), e);
    HIP_TRY(hipGetLastError());
  }
  if (const int st = xs_mark(h, 4, stream)) return st;

  if (values) {
    HIP_TRY(hipMemcpyAsync(values, h->d_q, 8 * (size_t)p.q_cells, hipMemcpyDeviceToDevice, S(stream)));
    HIP_TRY(hipMemcpyAsync(values + p.q_cells, h->d_r, 8 * (size_t)p.r_cells, hipMemcpyDeviceToDevice, S(stream)));
    HIP_TRY(hipMemcpyAsync(values + p.q_cells + p.r_cells, h->d_b, 8 * (size_t)p.r_cells, hipMemcpyDeviceToDevice, S(stream)));
  }
  HIP_TRY(hipMemcpyAsync(got, h->d_post, 8 * (size_t)(p.n * p.n + p.n + 2), hipMemcpyDeviceToHost, S(stream)));
  return PGM_OK;
}

extern "C" {

int pgm_xs_destroy(void *handle) {
  if (handle)
    for (void *e : static_cast<XsHandle *>(handle)->ev)
      if (e) (void)hipEventDestroy(static_cast<hipEvent_t>(e));
  return pgm_plan_destroy<XsHandle>(handle);
}

int pgm_xs_set_tiling(void *handle, int32_t tile_log2, int32_t high_bits) {
  if (!handle) return pgmi_fail(PGM_EINVAL, "xs_set_tiling: null handle");
  XsHandle *h = static_cast<XsHandle *>(handle);
  XsPlan p;
  const int st = xs_plan_build(h->p.n, tile_log2, high_bits, p);
  if (st != PGM_OK) return st;
  h->dev.release(kHipDevOps);  // the lists change with the tiling; frees nothing on a handle that never ran
  h->p = std::move(p);
  return PGM_OK;
}

int pgm_xs_run(void *handle, const int32_t *fam_node, const uint32_t *fam_mask, const double *fam_score, int64_t n_fam,
               pgm_xs_result_t *out, double *values, uint32_t *winners, void *stream) {
  XsHandle *h = static_cast<XsHandle *>(handle);
  std::vector<uint32_t> cell, mask;
  std::vector<double> score;
  int st = xs_run_check("xs_run", h, fam_node, fam_mask, fam_score, n_fam, out != nullptr, cell, mask, score);
  if (st != PGM_OK) return st;
  if ((values && (uintptr_t)values % 8) || (winners && (uintptr_t)winners % 4))
    return pgmi_fail(PGM_EINVAL, "xs_run: a table pointer is misaligned");
  if ((st = xs_use(h, false)) != PGM_OK || (st = xs_events(h)) != PGM_OK) return st;
  XsRecord rec;
  int32_t bits = 0;
  h->timed = 0;
  st = xs_enqueue(h, cell, mask, score, values, winners, &rec, stream);
  if (st == PGM_OK) st = flag_read(h->dev, stream, &bits);  // synchronises the stream
  if (st != PGM_OK) {
    (void)hipStreamSynchronize(S(stream));  // what was enqueued reads the vectors above and writes rec
    return st;
  }
  for (int i = 0; i < PGM_XS_PHASES; ++i) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, static_cast<hipEvent_t>(h->ev[i]), static_cast<hipEvent_t>(h->ev[i + 1])));
    h->phase_ms[i] = ms;
  }
  h->timed = PGM_XS_PHASES;
  out->score = rec.score, out->infeasible = bits != 0, out->n = h->p.n;
  memcpy(out->parents, rec.parents, sizeof rec.parents);
  memcpy(out->order, rec.order, sizeof rec.order);
  return PGM_OK;
}

int pgm_xs_posterior(void *handle, const int32_t *fam_node, const uint32_t *fam_mask, const double *fam_score,
                     int64_t n_fam, double *edge_post, double *log_z, double *mass, int32_t *infeasible, double *values,
                     void *stream) {
  XsHandle *h = static_cast<XsHandle *>(handle);
  std::vector<uint32_t> cell, mask;
  std::vector<double> score;
  int st = xs_run_check("xs_posterior", h, fam_node, fam_mask, fam_score, n_fam, edge_post && log_z && mass && infeasible,
                        cell, mask, score);
  if (st != PGM_OK) return st;
  if (values && (uintptr_t)values % 8) return pgmi_fail(PGM_EINVAL, "xs_posterior: the table pointer is misaligned");
  const XsPlan &p = h->p;
  XspEdgeArgs e = {};
  xs_by_node(p, cell, mask, score, e.off);
  if ((st = xs_use(h, true)) != PGM_OK || (st = xs_events(h)) != PGM_OK) return st;
  // the families of this call: the scores, then the cells, then the masks, in one allocation
  const size_t m = cell.size();
  char *fam = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&fam), 16 * std::max<size_t>(m, 1)));
  std::vector<double> got((size_t)(p.n * p.n + p.n + 2));
  int32_t bits = 0;
  h->timed = 0;
  st = xsp_enqueue(h, e, fam, cell, mask, score, values, got.data(), stream);
  if (st == PGM_OK) st = flag_read(h->dev, stream, &bits);  // synchronises the stream
  if (st != PGM_OK) (void)hipStreamSynchronize(S(stream));  // what was enqueued reads the vectors above and writes got
  (void)hipFree(fam);
  if (st != PGM_OK) return st;
  for (int i = 0; i < PGM_XS_POST_PHASES; ++i) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, static_cast<hipEvent_t>(h->ev[i]), static_cast<hipEvent_t>(h->ev[i + 1])));
    h->phase_ms[i] = ms;
  }
  h->timed = PGM_XS_POST_PHASES;
  std::copy(got.begin(), got.begin() + p.n * p.n, edge_post);
  std::copy(got.begin() + p.n * p.n, got.end() - 2, mass);
  log_z[0] = got[got.size() - 2], log_z[1] = got[got.size() - 1];
  *infeasible = bits != 0;
  return PGM_OK;
}
}

// pgm_xs.h — private interface between the two units of the exact structure search (include/pgmhip.h "Exact
// structure search"): pgmxs_plan.cpp (host only: the tiling, the popcount-ordered lists the sink kernel walks, the
// launch counts, the checks of the family list, pgm_xs_create / pgm_xs_info) and pgmxs.hip (the fill, scatter, zeta,
// sink and read-back kernels, the log-space kernels of the edge posteriors, the device side of the handle, pgm_xs_run /
// pgm_xs_posterior / pgm_xs_set_tiling / pgm_xs_destroy).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_fit.h"
#include "pgmhip.h"

static constexpr int kXsBlock = 256;       // work-items of a workgroup in every kernel of the unit
static constexpr int kXsMaxTile = 12;      // log2 of the largest LDS tile: 4,096 cells
static constexpr int kXsDefaultHigh = 4;   // high zeta bits per trip through memory
static constexpr int kXsChunk = 1 << 16;   // families staged per scatter launch
static constexpr uint32_t kXsNone = PGM_XS_NONE;
static constexpr int kXsPostCells = 1 << 23;  // cells of the posterior's row workspace: 64 MiB, one row of 24 nodes

// one launch of k_xs_zeta: a tile is 2^hh groups, b0 apart in the row, of 2^c consecutive cells, 2^(c + hh) = the
// tile; the passes run over the LDS bits [p0, p1).  The low launch has hh = 0, c = b0 = the tile, p0 = 0.
struct XsTrip {
  int32_t c, b0, hh, p0, p1;
};

struct PGM_FIT_LOCAL XsPlan {
  int32_t n = 0, W = 0;    // nodes; bits of a row's index = n - 1
  int32_t L = kXsMaxTile, h = kXsDefaultHigh;
  int32_t Lz = 0, Ls = 0;  // log2 of the zeta tile = min(L, W); of the sink tile = min(L, n)
  std::vector<XsTrip> trips;       // the zeta launches in order (none when W = 0)
  std::vector<uint32_t> hi_list;   // the high parts of a set, by (popcount, value)
  std::vector<int32_t> hi_off;     // [n - Ls + 2]: where each popcount starts in hi_list
  std::vector<uint16_t> lo_list;   // the low parts, by (popcount, value)
  int32_t lo_off[kXsMaxTile + 2] = {};
  int64_t q_cells = 0, r_cells = 0;  // n * 2^W; 2^n
  int32_t post_rows = 0;             // rows of gamma the posterior holds at a time: min(n, kXsPostCells >> W)
};

// the result as the read-back kernel writes it (pgm_xs_result_t without the flag, which is the handle's flag word)
struct XsRecord {
  double score;
  uint32_t parents[PGM_XS_MAX_NODES];
  int32_t order[PGM_XS_MAX_NODES];
};

struct PGM_FIT_LOCAL XsHandle {
  XsPlan p;
  pgmdev::PlanDev dev;
  double *d_q = nullptr, *d_r = nullptr;  // the base: Q and R of a search, alpha and F of a posterior
  uint32_t *d_a = nullptr, *d_k = nullptr;  // stage 0: the winners, which only a search keeps
  double *d_b = nullptr, *d_g = nullptr, *d_post = nullptr;  // stage 1, the posterior's: B, post_rows rows of gamma, the outputs
  const uint32_t *d_hi_list = nullptr;
  const uint16_t *d_lo_list = nullptr;
  uint32_t *d_fam_cell = nullptr, *d_fam_mask = nullptr;  // the staging of one chunk of families
  double *d_fam_score = nullptr;
  XsRecord *d_rec = nullptr;
  // the events of the last run (hipEvent_t, made by pgmxs.hip on device ev_device) and the times between them
  void *ev[PGM_XS_POST_PHASES + 1] = {};
  int ev_device = -1;
  double phase_ms[PGM_XS_POST_PHASES] = {};
  int timed = 0;  // the phases of the last completed run: PGM_XS_PHASES, PGM_XS_POST_PHASES, or 0 before it
};

static inline int64_t xs_zeta_lds(const XsPlan &p) { return ((int64_t)12) << p.Lz; }  // fp64 value + uint32 winner
static inline int64_t xs_sink_lds(const XsPlan &p) { return ((int64_t)9) << p.Ls; }   // fp64 value + uint8 winner
static inline int64_t xs_post_lds(int32_t tile_log2) { return ((int64_t)8) << tile_log2; }  // fp64 value alone

// the plan of n nodes under the tiling (L, h); PGM_EINVAL outside 1 <= n <= PGM_XS_MAX_NODES, 1 <= h <= L <= 12
PGM_FIT_LOCAL int xs_plan_build(int32_t n, int32_t L, int32_t h, XsPlan &out);
// The checks of pgm_xs_run and pgm_xs_posterior (no HIP call; `who` opens the messages, `out` is the run's result or
// the posterior's outputs and'ed together).  On PGM_OK cell / mask / score hold the families with a finite score, ready
// for the scatter kernel: cell = v * 2^W + (the mask with bit v squeezed out).
PGM_FIT_LOCAL int xs_run_check(const char *who, const XsHandle *h, const int32_t *fam_node, const uint32_t *fam_mask,
                               const double *fam_score, int64_t n_fam, bool out, std::vector<uint32_t> &cell,
                               std::vector<uint32_t> &mask, std::vector<double> &score);
// The families of xs_run_check by ascending cell, so by node: off [n + 1] is where each node's families start.  The
// order of the caller's list is gone after it: the posterior's sums do not depend on it.
PGM_FIT_LOCAL void xs_by_node(const XsPlan &p, std::vector<uint32_t> &cell, std::vector<uint32_t> &mask,
                              std::vector<double> &score, uint32_t *off);

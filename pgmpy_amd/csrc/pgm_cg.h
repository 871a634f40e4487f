// pgm_cg.h — private interface between the two units of the conditional-Gaussian scores (include/pgmhip.h
// "conditional-Gaussian scores"): pgmcg_plan.cpp (host only: validation of the families, the tile / block /
// job layout, the choice of the row slice and of the passes, the argument checks of the pgm_cg_* entry
// points) and pgmcg.hip (k_cg_moments, k_cg_reduce, k_cg_score, k_cg_score_sum, the device side of the
// handle, the launches).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_CG_LOCAL __attribute__((visibility("hidden")))

static constexpr int kCgMaxCont = PGM_CG_MAX_CONT;
static constexpr int kCgMaxRows = PGM_CG_MAX_ROWS;
static constexpr int kCgTile = 16;          // operand rows of one v_mfma_f64_16x16x4_f64 accumulator
static constexpr int kCgTileDoubles = 256;  // one accumulator: 4 registers x 64 lanes
static constexpr int kCgTilesPerWave = PGM_CG_TILES_PER_WAVE;
static constexpr int kCgRowsPerLane = 4;    // consecutive rows of its column a lane holds per step
static constexpr int kCgStep = 16;          // rows of one step: 4 k slots x kCgRowsPerLane
static constexpr int64_t kCgMaxSlices = PGM_CG_MAX_SLICES;
static constexpr int64_t kCgSliceMin = PGM_CG_SLICE_MIN;
static constexpr int64_t kCgSliceMax = (int64_t)1 << 40;
static constexpr int64_t kCgStageTiles = PGM_CG_STAGE_TILES;
static constexpr int kCgScoreChunk = PGM_CG_SCORE_CHUNK;
static constexpr int kCgSumBlock = 64;
// a column whose centred sum of squares is at or below kCgConstant (n_g + 2) times its shifted sum of squares is
// constant to rounding (4 u, u = 2^-53): its variance is taken as 0 and the factorisation drops it
static constexpr double kCgConstant = 4.0 * 1.1102230246251565e-16;

// a family as the kernels read it
struct CgFam {
  int32_t n_disc, m, mp, var_disc;
  int32_t Q, QD;             // configurations of all the code columns / of the discrete parents (the jobs)
  int32_t n_tiles, cpt;      // tiles of 16 operand rows; configurations per tile = 16 / mp
  int64_t mom_off;           // of its [Q][mp][mp] block in the moments buffer
  int32_t dcol[PGM_MAX_DIMS], card[PGM_MAX_DIMS], stride[PGM_MAX_DIMS];
  int32_t ccol[kCgMaxCont + 1];
};

// a wave of a moments launch: tiles [tile0, tile0 + n_tiles) of family fam; tile_off: the index of its first
// tile among all the plan's tiles
struct CgBlock {
  int32_t fam, tile0, n_tiles, reserved;
  int64_t tile_off;
};

struct PGM_CG_LOCAL CgPlan {
  std::vector<CgFam> fams;
  std::vector<CgBlock> blocks;
  std::vector<int64_t> chunk_off;  // n_families + 1: the score workgroups of family f are [chunk_off[f], chunk_off[f + 1])
  int32_t n_code_cols = 0, n_value_cols = 0;
  int64_t total_tiles = 0, total_jobs = 0, moments_size = 0, stage_tiles = 0;
  int64_t slice_rows = 0;  // 0: chosen per call; else forced (pgm_cg_plan_set_slice)
};

struct PGM_CG_LOCAL CgHandle {
  CgPlan p;
  pgmdev::PlanDev dev;
  const CgFam *d_fams = nullptr;
  const CgBlock *d_blocks = nullptr;
  const int64_t *d_chunk_off = nullptr;
  double *d_part = nullptr;        // stage kCgMomentStage: stage_tiles accumulators
  double *d_score_part = nullptr;  // stage kCgScoreStage: one partial of each output per chunk
  int64_t *d_score_ipart = nullptr;
};
enum { kCgMomentStage = 0, kCgScoreStage = 1 };

// consecutive blocks whose partials of n_slices slices fit the stage
struct CgPass {
  int64_t block0, n_blocks, tile_off, n_tiles;
};

PGM_CG_LOCAL int cg_plan_build(const pgm_cg_family *fams, int32_t n, CgPlan &out);
// rows per slice of a moments launch over n_rows rows: a function of n_rows alone, or the forced value
PGM_CG_LOCAL int64_t cg_slice_rows(const CgPlan &p, int64_t n_rows);
PGM_CG_LOCAL bool cg_vec16(const void *X, int64_t ld_x, int64_t row0);
PGM_CG_LOCAL void cg_passes(const CgPlan &p, int64_t n_slices, std::vector<CgPass> &out);
PGM_CG_LOCAL int cg_moments_check(const CgHandle *h, const uint8_t *codes, int32_t n_code_cols, int64_t ld_codes, const double *X,
                                  int32_t n_value_cols, int64_t ld_x, int64_t row0, int64_t n_rows, const double *shift,
                                  const double *moments, int64_t *slice, int64_t *n_slices);
PGM_CG_LOCAL int cg_score_check(const CgHandle *h, const double *moments, const double *ll, const int64_t *n_complete,
                                const int64_t *n_observed, const int64_t *n_dropped);

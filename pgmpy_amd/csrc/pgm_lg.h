// pgm_lg.h — private interface between the two units of the linear-Gaussian networks: pgmlg_plan.cpp (host
// only: validation of the columns and families, the tile groups, the choice of the row slice, the argument
// checks of the pgm_lg_* entry points) and pgmlg.hip (k_lg_colsum, k_lg_gram, k_lg_sample, k_lg_logpdf,
// k_lg_affine, the device side of the two handles, the launches).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_LG_LOCAL __attribute__((visibility("hidden")))

// Geometry of k_lg_gram (include/pgmhip.h "linear-Gaussian networks").  The d data columns and the ones
// column are laid end to end and cut into tiles of kLgTile = 16 columns (one v_mfma_f64_16x16x4_f64 operand
// side) and super-tiles of kLgSuper = 4 tiles.  A wave owns one group (super-tile I against super-tile J,
// I <= J) and one row slice: 4 x 4 accumulators of 16 x 16 fp64, 8 registers per lane each.  A step is
// kLgStep = 16 rows: lane (i, q) holds the kLgRowsPerLane = 4 rows r + 4 q .. r + 4 q + 3 of column i of
// every tile, and issues up to 16 MFMAs per row slot.
static constexpr int kLgTile = PGM_LG_TILE;
static constexpr int kLgSuper = PGM_LG_SUPER;
static constexpr int kLgSuperCols = kLgTile * kLgSuper;
static constexpr int kLgRowsPerLane = PGM_LG_ROWS_PER_LANE;
static constexpr int kLgStep = PGM_LG_STEP;
static constexpr int kLgAccPerGroup = kLgSuper * kLgSuper;
static constexpr int kLgAccDoubles = 256;  // one 16 x 16 accumulator: 4 registers x 64 lanes
static constexpr int64_t kLgTargetBlocks = PGM_LG_TARGET_BLOCKS;
static constexpr int64_t kLgSliceMin = PGM_LG_SLICE_MIN;
static constexpr int64_t kLgSliceMax = (int64_t)1 << 40;
static constexpr int kLgColsumBlock = 256;
static constexpr int64_t kLgColsumChunk = PGM_LG_COLSUM_CHUNK;
static constexpr int64_t kLgColsumMaxChunks = PGM_LG_COLSUM_MAX_CHUNKS;
static constexpr int kLgMaxParents = PGM_LG_MAX_PARENTS;
static constexpr int kLgBlock = PGM_LG_BLOCK;
static constexpr int64_t kLgMaxBlocks = PGM_LG_MAX_BLOCKS;
static constexpr int kLgAffineChunk = PGM_LG_AFFINE_CHUNK;
static constexpr int kLgMaxColumns = 16384;  // d of a Gram handle: 257 super-tiles, 33,153 groups (the reduce kernel's grid.y)

// what a lane's column is: >= 0 a data column of X, else one of these
enum { kLgOnes = -1, kLgPad = -2 };

struct LgGroup {
  int32_t I, J;
};

struct PGM_LG_LOCAL LgGramPlan {
  std::vector<int32_t> cols;     // the d columns
  std::vector<int32_t> lane_col; // n_super * 64 entries: the column of every padded index (kLgOnes at d, kLgPad after)
  std::vector<LgGroup> groups;   // I <= J, I-major
  int32_t d = 0, n_cols = 0, n_tiles = 0, n_super = 0;
  int64_t n_tile_pairs = 0;
  int64_t max_slices = 0;
  int64_t slice_rows = 0;        // 0: chosen per call; else forced (pgm_lg_gram_plan_set_slice)
};

struct PGM_LG_LOCAL LgGramHandle {
  LgGramPlan p;
  pgmdev::PlanDev dev;
  const int32_t *d_lane_col = nullptr;
  const LgGroup *d_groups = nullptr;
  const int32_t *d_cols = nullptr;
  double *d_part = nullptr;    // stage kLgGramStage: max_slices x n_groups x 16 accumulators
  double *d_colpart = nullptr; // stage kLgColsumStage: d x kLgColsumMaxChunks pieces
};
enum { kLgNoStage = -1, kLgGramStage = 0, kLgColsumStage = 1 };

struct PGM_LG_LOCAL LgNetPlan {
  std::vector<int32_t> fam_off, fam_cols;
  int32_t n_cols = 0, max_parents = 0;
};

struct PGM_LG_LOCAL LgNetHandle {
  LgNetPlan p;
  pgmdev::PlanDev dev;
  const int32_t *d_fam_off = nullptr;
  const int32_t *d_fam_cols = nullptr;
  double *d_part = nullptr;  // stage 0: kLgMaxBlocks workgroup partials of pgm_lg_logpdf
};

PGM_LG_LOCAL int lg_gram_plan_build(const int32_t *cols, int32_t d, LgGramPlan &out);
// rows per slice of a Gram over n_rows rows (forced: the plan's own, rounded up and raised to fit max_slices)
PGM_LG_LOCAL int64_t lg_slice_rows(const LgGramPlan &p, int64_t n_rows);
// whether every 16-byte operand load of a Gram over this window is aligned
PGM_LG_LOCAL bool lg_vec16(const void *X, int64_t ld, int64_t row0);
// rows of one piece of a column sum over n_rows rows
PGM_LG_LOCAL int64_t lg_colsum_chunk(int64_t n_rows);
// the window checks every entry point shares (no HIP call)
PGM_LG_LOCAL int lg_window_check(const char *what, const void *X, int32_t n_cols, int32_t plan_cols, int64_t ld, int64_t row0,
                                 int64_t n_rows);
PGM_LG_LOCAL int lg_colsum_check(const LgGramHandle *h, const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                                 const double *sums, const int64_t *counts, int64_t *chunk, int64_t *n_chunks);
PGM_LG_LOCAL int lg_gram_check(const LgGramHandle *h, const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                               const double *shift, const double *out, int64_t *slice, int64_t *n_slices);
PGM_LG_LOCAL int lg_net_build(const int32_t *fam_off, const int32_t *fam_cols, int32_t n, LgNetPlan &out);
PGM_LG_LOCAL int lg_sample_check(const LgNetHandle *h, const double *coef, const double *X, int32_t n_cols, int64_t ld,
                                 int64_t row0, int64_t n_rows, int64_t first_row, int64_t *blocks);
PGM_LG_LOCAL int lg_logpdf_check(const LgNetHandle *h, const double *coef, const double *konst, const double *X, int32_t n_cols,
                                 int64_t ld, int64_t row0, int64_t n_rows, const double *logp, const double *total,
                                 int64_t *blocks);
PGM_LG_LOCAL int lg_affine_check(const double *W, const double *c, const int32_t *in_cols, int32_t n_in, int32_t n_out,
                                 const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, const double *out,
                                 int64_t ld_out, int64_t *blocks);

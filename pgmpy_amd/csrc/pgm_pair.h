// pgm_pair.h — private interface between the two units of the pairwise counts: pgmpair_plan.cpp (host only:
// validation, the state table, the tile-pair and group lists, the choice of the row slice, the argument
// checks of the pgm_pair_* entry points) and pgmpair.hip (k_pair_count, k_pair_mi, k_pair_emi, the device
// side of the handle, the launches).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_PAIR_LOCAL __attribute__((visibility("hidden")))

// Geometry of k_pair_count.  The states of all variables are laid end to end and cut into tiles of
// kPairTile = 16 states (one MFMA operand: v_mfma_i32_16x16x64_i8 takes 16 states x 64 rows per side) and
// into super-tiles of kPairSuper = 4 tiles.  A wave owns one group: super-tile I against super-tile J
// (I <= J), a register tile of 4 x 4 accumulators of 16 x 16 int32 (64 accumulator registers per lane).
// Each step of kPairStep = 64 rows forms 4 A and 4 B fragments and issues up to 16 MFMAs, so a fragment is
// reused four times.  A workgroup is kPairWaves waves on one group and one row slice; wave w takes the
// steps w, w + kPairWaves, ... of the slice.
static constexpr int kPairTile = 16;
static constexpr int kPairSuper = 4;
static constexpr int kPairSuperStates = kPairTile * kPairSuper;
static constexpr int kPairStep = 64;
static constexpr int kPairWaves = 4;
static constexpr int kPairBlock = 64 * kPairWaves;
// the slice: a multiple of kPairSliceQuantum rows (every wave gets whole steps), at most kPairSliceMax (an
// int32 accumulator holds a slice's count), chosen so that a launch has about kPairTargetBlocks workgroups
// (four per CU of a 256-CU device: one wave per SIMD and workgroup)
static constexpr int64_t kPairSliceQuantum = (int64_t)kPairStep * kPairWaves;
static constexpr int64_t kPairSliceMax = (int64_t)1 << 30;
static constexpr int64_t kPairTargetBlocks = 1024;
static constexpr int64_t kPairMaxSlices = 65535;  // grid.y
// the statistic kernels: one workgroup of kPairStatBlock work-items per (stratum, pair)
static constexpr int kPairStatBlock = PGM_PAIR_STAT_BLOCK;
static constexpr int kPairMaxCard = 254;

// one state as the count kernel reads it (device memory, one per lane and fragment)
struct PairState {
  int32_t col;   // code column of the state's variable
  int32_t k;     // local state: the code byte that means this state
  int32_t card;  // cardinality of the variable
  int32_t pad;   // 1: no state (past S); its fragment is zero
};
// one group: super-tile I against super-tile J
struct PairGroup {
  int32_t I, J;
  int32_t check;     // bit 0: the A side checks its codes, bit 1: the B side does (each super-tile once)
  int32_t reserved;
};
// one pair of variables u < v as the statistic kernels read it
struct PairVars {
  int32_t off_u, off_v, card_u, card_v;
};
static_assert(sizeof(PairState) == 16 && sizeof(PairGroup) == 16 && sizeof(PairVars) == 16, "descriptor packing");

struct PGM_PAIR_LOCAL PairPlan {
  std::vector<int32_t> cols, cards;
  std::vector<int64_t> off;        // first state of each variable, + S
  std::vector<PairState> states;   // S rounded up to kPairSuperStates entries
  std::vector<int32_t> tile_pairs; // (ti, tj), ti <= tj: the tiles that touch a block of two variables
  std::vector<PairGroup> groups;   // the super-tile pairs that hold one of them
  std::vector<PairVars> pairs;     // u < v, u-major
  int64_t S = 0, Sp = 0;
  int32_t n_cols = 0;              // 1 + the largest code column read
  int64_t slice_rows = 0;          // 0: chosen per call; else forced (pgm_pair_plan_set_slice)
};

struct PGM_PAIR_LOCAL PairHandle {
  PairPlan p;
  pgmdev::PlanDev dev;
  const PairState *d_states = nullptr;
  const PairGroup *d_groups = nullptr;
  const PairVars *d_pairs = nullptr;
};

PGM_PAIR_LOCAL int pair_plan_build(const int32_t *cols, const int32_t *cards, int32_t n_vars, PairPlan &out);
// rows per slice of a count over n_rows rows in n_strata strata (forced: the plan's own, rounded up)
PGM_PAIR_LOCAL int64_t pair_slice_rows(const PairPlan &p, int64_t n_rows, int32_t n_strata);
// the argument checks of pgm_pair_count (no HIP call); *slice: rows per slice, *n_slices: grid.y (0: nothing to do)
PGM_PAIR_LOCAL int pair_count_check(const PairHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                                    int64_t n_rows, int32_t strat_col, int32_t n_strata, const int64_t *counts,
                                    int64_t *slice, int64_t *n_slices);
// whether every 16-byte operand load of a count over this window is aligned
PGM_PAIR_LOCAL bool pair_codes_vec16(const void *codes, int64_t ld, int64_t row0);
// the argument checks of pgm_pair_mi / pgm_pair_emi (no HIP call); what: the entry point's name
PGM_PAIR_LOCAL int pair_stat_check(const char *what, const PairHandle *h, const int64_t *counts, int32_t n_strata,
                                   const void *const *outs, int n_outs);

// pgm_dbn.h — private interface between the two units of the dynamic-network filter (include/pgmhip.h
// "dynamic Bayesian networks"): pgmdbn_plan.cpp (host only: validation of the slice nodes and the two
// family sets, the offset tables, the launch geometry, the argument checks of pgm_dbn_run, pgm_dbn_viterbi and
// pgm_dbn_estep) and pgmdbn.hip (k_dbn, k_dbn_viterbi, k_dbn_estep, the device side of the handle, the
// launches).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_DBN_LOCAL __attribute__((visibility("hidden")))

static constexpr int kDbnMaxConfigs = PGM_DBN_MAX_CONFIGS;
static constexpr int kDbnMaxNodes = 255;
static constexpr int kDbnMaxSlices = 65535;
static constexpr int kDbnBlock = 64;            // one wave per workgroup: a barrier is one wave's
static constexpr int64_t kDbnLdsMax = 163840;   // a workgroup may take the CU's whole LDS

// What the kernel reads of a plan: offsets into one int32 table (DbnPlan::tab), and the geometry.
// Set 0 is the slice-0 families, set 1 the transition families; family f is the family of node f (its table
// lies where the order given put it: voff), so products run in node order whatever order the caller used.
struct DbnLayout {
  int32_t n, J, S, R;           // slice nodes; joint states of the free nodes; of the free interface; J / S
  int32_t P, spw;               // lanes of a sequence (a power of two <= 64); sequences per wave
  int32_t n_free, n_prev, n_cur, Q;
  int32_t o_card, o_clamp, o_xstride, o_free;  // [n] each ([n_free] the last)
  int32_t o_ix, o_xperm;                        // [J]: I(x); the x of interface state i at [i R, (i + 1) R)
  int32_t o_voff[2], o_xoff[2];                 // [n] table offset; [n J] offset the free nodes of x add
  int32_t o_ctoff[2], o_ctidx[2], o_ctstr[2];   // clamped terms of family f: [ctoff[f], ctoff[f + 1])
  int32_t o_cur, o_prev;        // transition families without / with a free slice-t parent
  int32_t o_ioff;               // [n_prev S]: offset the interface state adds
  int32_t o_qnode, o_qstate;    // [Q]
};

struct PGM_DBN_LOCAL DbnPlan {
  DbnLayout L = {};
  std::vector<int32_t> tab;
  std::vector<int64_t> off[2], size[2];  // per family of a set, in the order given
  int64_t total[2] = {0, 0};
  int64_t lds_bytes = 0;
};

struct PGM_DBN_LOCAL DbnHandle {
  DbnPlan p;
  pgmdev::PlanDev dev;
  const int32_t *d_tab = nullptr;
};

static inline int64_t dbn_lds_bytes(int32_t spw, int32_t n, int32_t J, int32_t S) {
  return (int64_t)spw * (8 * ((int64_t)J + 2 * (int64_t)S) + 4 * (int64_t)n + 2 * (int64_t)n);
}

PGM_DBN_LOCAL int dbn_plan_build(const int32_t *card, const uint8_t *clamped, const uint8_t *queried, int32_t n,
                                 const pgm_fit_family *fam0, int32_t n_fam0, const pgm_fit_family *fam1, int32_t n_fam1,
                                 DbnPlan &out);
// the checks of pgm_dbn_run (no HIP call); *launch: whether there is anything to launch
PGM_DBN_LOCAL int dbn_run_check(const DbnHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                                int64_t n_rows, int32_t n_slices, const double *values0, const double *values1,
                                const double *filter, const double *smooth, const double *loglik, const double *scratch,
                                int64_t scratch_bytes, bool *launch);
// k_dbn_estep's accumulation (include/pgmhip.h "expected counts"): the fp64 tile of both table sets lies in
// LDS behind the sequences' state, at the next multiple of 8 bytes; the grid of the tile path is capped at
// kDbnCus x the workgroups whose LDS fits a CU, so that a workgroup flushes its tile once
static constexpr int kDbnCus = 256;            // the MI355X's; another count changes the cap, not the result
static constexpr int kDbnWavesPerCu = 32;      // one-wave workgroups a CU holds
struct DbnEstepGeom {
  bool tile = false, fits = false;
  int64_t tile_at = 0;      // doubles into LDS where the tile begins
  int64_t tile_bytes = 0, lds_bytes = 0;
  int32_t blocks_per_cu = 0;
  int64_t max_blocks = 0;
};
PGM_DBN_LOCAL DbnEstepGeom dbn_estep_geom(const DbnPlan &p, uint32_t flags);
// the checks of pgm_dbn_estep (no HIP call): dbn_run_check's for a smoother, the tables, the flags
PGM_DBN_LOCAL int dbn_estep_check(const DbnHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                                  int64_t n_rows, int32_t n_slices, const double *values0, const double *values1,
                                  const double *tables0, const double *tables1, const double *loglik, const double *scratch,
                                  int64_t scratch_bytes, uint32_t flags, bool *launch);
// the checks of pgm_dbn_viterbi (no HIP call); the backpointers take dbn_viterbi_scratch(...) bytes
static inline double dbn_viterbi_scratch(int64_t n_rows, int32_t n_slices, int32_t J) {
  return (double)n_rows * (n_slices - 1) * J * 2.0;
}
PGM_DBN_LOCAL int dbn_viterbi_check(const DbnHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                                    int64_t n_rows, int32_t n_slices, const double *values0, const double *values1,
                                    const uint8_t *path, int64_t ld_out, int64_t row0_out, const double *logmap,
                                    const void *scratch, int64_t scratch_bytes, bool *launch);

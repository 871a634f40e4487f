// pgm_emrows.h — private interface between the two units of the rows E-step (pgm_fit_estep_rows: expectation
// maximisation on rows with missing cells): pgmemrows_plan.cpp (host only: the plan's column lists, the latent
// columns of a call, the argument checks, pgm_fit_estep_rows_info) and pgmemrows.hip (the kernel, the device
// side of the stage, the launch).  Both work on the fit plan's handle (pgm_fit.h).  Not part of include/pgmhip.h.
#pragma once
#include "pgm_fit.h"

// Launch geometry.  A workgroup of kEmrBlock work-items (kEmrWaves waves) takes kEmrRows consecutive rows in
// passes of kEmrBlock: a lane scans one row, then a wave takes one queued row at a time.  A row costs a wave
// here, not a lane as in the counting kernel, so a workgroup takes a quarter of kFitRowsPerBlock: 1 M rows are
// 977 workgroups, four per CU, and the tile is flushed once per 1,024 rows.
static constexpr int kEmrBlock = kFitBlock;
static constexpr int kEmrWaves = kEmrBlock / 64;
static constexpr int kEmrRows = kFitRowsPerBlock / 4;
// the kernel takes 153 VGPRs: 3 waves per SIMD, so the 4 SIMDs of a CU hold 3 workgroups of 4 waves
static constexpr int kEmrBlocksPerCuByRegs = 3;
static constexpr int kEmrMaxU = PGM_EMR_MAX_UNOBSERVED;      // unobserved cells of a row
static constexpr int kEmrMaxRowFam = PGM_EMR_MAX_ROW_FAMILIES;  // families a row touches
static constexpr int kEmrMaxFam = PGM_EM_MAX_FAMILIES;       // families one component touches
static constexpr int kEmrMaxDigits = 12;                     // variables with >= 2 states of a component: 2^12 = PGM_EM_MAX_CONFIGS
static_assert((1 << kEmrMaxDigits) == PGM_EM_MAX_CONFIGS, "a component within the cap has at most kEmrMaxDigits digits");
static_assert(kEmrMaxU == 32, "a family's unobserved members are one uint32 mask over U");

// One wave's slice of LDS: the row it works on.  U(r) in ascending column order (label = index in U until the
// propagation), the touched families with their members of U as a mask, and the stage of the component
// being enumerated: its digits' cardinalities and per family the table offset, the observed part of the
// entry and the stride of every digit (0: not in the family's scope).
struct EmrWave {
  int32_t u_col[kEmrMaxU], u_card[kEmrMaxU], u_label[kEmrMaxU], u_slot[kEmrMaxU];
  int32_t u_nfam[kEmrMaxU], u_configs[kEmrMaxU], u_poff[kEmrMaxU + 1];
  double u_z[kEmrMaxU];
  int32_t f_id[kEmrMaxRowFam];
  uint32_t f_mask[kEmrMaxRowFam];
  int64_t c_off[kEmrMaxFam];
  int32_t c_base[kEmrMaxFam];
  int32_t c_stride[kEmrMaxFam][kEmrMaxDigits];
  int32_t c_card[kEmrMaxDigits];
};
// static LDS of the kernel: the waves' slices, the queue of the pass (one int32 per lane) and its counters
static constexpr int32_t kEmrStaticLds = kEmrWaves * (int32_t)sizeof(EmrWave) + kEmrBlock * 4 + 8;

// The call's side of the launch, passed by value (workgroup-uniform: scalar loads from the kernarg segment).
struct EmrSpec {
  int32_t n_latent, n_pos;  // latent columns; positions of the plan's column list
  int32_t n_fam, flags;
  int32_t tile, total_bins;       // 1: the tables are privatised in LDS as total_bins fp64
  int32_t pos[kEmrMaxU];          // the latents' positions in the column list, ascending
};

// the plan's column lists (h->emr), built once; PGM_OK, or PGM_EINVAL for a column with two cardinalities
PGM_FIT_LOCAL int emr_lists(FitHandle *h, const char *what);
// the latent columns of a call against the plan (no HIP call); *n_obs_cols: 1 + the largest observed column
PGM_FIT_LOCAL int emr_spec(FitHandle *h, const int32_t *latent_cols, int32_t n_latent, int32_t flags, bool want_tables,
                           const char *what, EmrSpec *spec, int32_t *n_obs_cols);
// the argument checks of pgm_fit_estep_rows (no HIP call); *blocks: workgroups of the launch
PGM_FIT_LOCAL int emr_check(FitHandle *h, const int32_t *latent_cols, int32_t n_latent, int32_t flags,
                            const double *values, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                            int64_t n_rows, const double *tables, const double *loglik, EmrSpec *spec, int64_t *blocks);

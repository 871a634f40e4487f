// pgm_dbn_pf.h — private interface between the two units of the dynamic-network particle filter
// (include/pgmhip.h "dynamic Bayesian networks: the particle filter"): pgmdbn_pf_plan.cpp (host only: validation
// of the slice nodes and the two family sets, the plan order, the interface, the LDS geometry, the argument
// checks of pgm_dbn_pf_run and pgm_dbn_pf_trace) and pgmdbn_pf.hip (k_dbn_pf_cdf, k_dbn_pf, k_dbn_pf_trace, the
// device side of the handle, the launches).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgm_plan_dev.h"
#include "pgmhip.h"

#define PGM_DBN_PF_LOCAL __attribute__((visibility("hidden")))

static constexpr int kPfMaxNodes = 255;
static constexpr int kPfMaxCard = 254;
static constexpr int kPfMaxSlices = 65535;
static constexpr int kPfMaxBlock = 256;         // work-items of a workgroup: min(N, 256)
static constexpr int64_t kPfLdsMax = 163840 - 256;  // the CU's LDS less the 256 static bytes the compiler gives k_dbn_pf
static constexpr int kPfPadBytes = 128;         // the reduction pad: 4 wave maxima, 4 wave totals, 3 sums, 2 flags
static constexpr int kPfQuantBits = 36;         // q = trunc(ldexp(w / w_max, 36))
static constexpr int kPfEssShift = 16;          // q' = q >> 16

// One family in plan order, as the kernel reads it.  A parent is a byte row of the workgroup's code tile:
// row v < n is node v of the slice being drawn, row n + i is interface node i of the slice before.
struct PfFam {
  int32_t node, card, ncol, n_par;   // ncol: parent configurations (the stride of a state in the table)
  int32_t off;                       // the table's offset in the set's value buffer
  int32_t src[PGM_MAX_DIMS - 1];
  int32_t stride[PGM_MAX_DIMS - 1];
};

struct PGM_DBN_PF_LOCAL PfPlan {
  int32_t n = 0, n_iface = 0, n_qnodes = 0, bins = 0;
  std::vector<PfFam> fams;              // [2 n]: the slice-0 set in its plan order, then the transition set
  std::vector<int64_t> col_off;         // [2 (n + 1)]: CPD columns before family f of a set, in plan order
  std::vector<int32_t> tab;             // card [n], iface [n_iface], qnode [n_qnodes], qoff [n_qnodes]
  int32_t o_card = 0, o_iface = 0, o_qnode = 0, o_qoff = 0;
  std::vector<int32_t> order[2];        // the plan order of a set: node indices
  std::vector<int64_t> off[2];          // per family of a set, in the order given
  int64_t total[2] = {0, 0};
};

struct PGM_DBN_PF_LOCAL PfHandle {
  PfPlan p;
  pgmdev::PlanDev dev;
  const PfFam *d_fams = nullptr;
  const int64_t *d_col_off = nullptr;
  const int32_t *d_tab = nullptr;
  double *d_cdf0 = nullptr, *d_cdf1 = nullptr;  // the running sums of the two value buffers
};

// The LDS of a workgroup, in this order: the code tile [(n + n_iface)][N] bytes (rounded up to 8), the
// weights / quanta / their scan [N] 8 bytes, the histogram [bins] 8 bytes, the pad, the slice's evidence [n].
static inline int64_t pf_lds_bytes(int32_t n, int32_t n_iface, int32_t bins, int64_t N) {
  const int64_t tile = (((int64_t)n + n_iface) * N + 7) / 8 * 8;
  return tile + 8 * N + 8 * (int64_t)bins + kPfPadBytes + ((int64_t)n + 7) / 8 * 8;
}
// the largest power of two in [64, 4096] whose LDS fits, 0 when none does
static inline int32_t pf_max_particles(const PfPlan &p) {
  int32_t best = 0;
  for (int32_t N = PGM_DBN_PF_MIN_PARTICLES; N <= PGM_DBN_PF_MAX_PARTICLES; N *= 2)
    if (pf_lds_bytes(p.n, p.n_iface, p.bins, N) <= kPfLdsMax) best = N;
  return best;
}

PGM_DBN_PF_LOCAL int pf_plan_build(const int32_t *card, const uint8_t *queried, int32_t n, const pgm_fit_family *fam0,
                                   int32_t n_fam0, const pgm_fit_family *fam1, int32_t n_fam1, PfPlan &out);
// the checks of pgm_dbn_pf_run (no HIP call); *launch: whether there is anything to launch
PGM_DBN_PF_LOCAL int pf_run_check(const PfHandle *h, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                                  int64_t n_rows, int32_t n_slices, const double *values0, const double *values1,
                                  int32_t n_particles, int64_t first_row, const double *filter, const double *loglik,
                                  const double *ess, const uint16_t *ancestors, const uint8_t *traj, bool *launch);
// the checks of pgm_dbn_pf_trace (no HIP call)
PGM_DBN_PF_LOCAL int pf_trace_check(const PfHandle *h, const uint16_t *ancestors, const uint8_t *traj, int64_t n_rows,
                                    int32_t n_slices, int32_t n_particles, const uint8_t *out, int64_t ld_out,
                                    int64_t row0_out, bool *launch);

// pgm_rows.h — private interface between the two units of the fused row plan: pgmrows_plan.cpp (host
// only: the plan compiler, the generator of the plan-specialised kernel source, the launch predicates)
// and pgmrows.hip (the kernels, the handle, the pgm_rows_* C-ABI).  Not part of include/pgmhip.h.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "pgmhip.h"

// Descriptors live in device memory as packed structs (one s_load_dwordx16 per component, one
// s_load_dwordx4 per evidence term).  Table-driven components: for every entry e of a component's
// (query x hidden) index space the host precomputes each factor's offset (tab[off_base + e*nf + j]),
// the marginal rows each query dim accumulates into (tab[marg_base + qi*nq + i]) and the entry's MAP
// index digit (tab[map_base + qi]).  Affine components (one query dim, no hidden dim) need no
// table: factor j sits at base_j + s * fstride[j] for query state s.
struct RowsComp {
  int32_t nf, nt, P, H;
  int32_t simple, mstride, q_lo, q_hi;
  int32_t off_base, marg_base, map_base, ev_lo;  // ev_lo: first evidence term (n_ev when none)
  int32_t val_lo, val_hi, marg0, nq;              // marg0: marginal row of the (affine) query dim
  int32_t fbase[PGM_ROWS_MAX_FAC];
  int32_t fstride[PGM_ROWS_MAX_FAC];
  // affine fast kernel: evidence terms folded into per-slot strides (term j adds code_j * aS[j][k]
  // to factor slot k), padded to 8 terms (stride 0, card 256, a real column)
  int32_t a_S[8][4];
  int32_t a_col[8], a_card[8];
};
struct RowsTerm {
  int32_t col, stride, card, slot;  // evidence column, stride in its factor, cardinality, factor slot
};
struct RowsK {
  int32_t n_values, n_marg, n_joint, n_comp;  // n_values includes the trailing 1.0 (index one_idx)
  int32_t n_waves, terms_off, tab_off, one_idx;  // offsets (in int32) into the descriptor buffer
  int32_t q_marg_off[PGM_ROWS_MAX_LOOP], q_card[PGM_ROWS_MAX_LOOP];
};
static_assert(sizeof(RowsComp) % 16 == 0 && sizeof(RowsTerm) == 16, "descriptor packing");

// internal to the library: not in its dynamic symbol table
#define PGM_ROWS_LOCAL __attribute__((visibility("hidden")))

// a compiled pgm_rows_plan: what the kernels read, before anything touches a device
struct PGM_ROWS_LOCAL RowsPlan {
  RowsK k;
  std::vector<int32_t> desc;  // descriptor buffer: [RowsComp x n_comp][RowsTerm blocks][tables][0]
  int max_nf = 1, max_nt = 0;
  bool any_table = false, all_affine = false;
  int n_cols = 0;         // 1 + the largest evidence column the plan reads (0: none)
  std::vector<int> cols;  // the evidence columns the plan reads, ascending
  std::string jit_src;    // source of the plan-specialised kernels (plans without a table component)
};

// How the generated kernels touch memory: the cache policy of the evidence-code loads and of the output
// stores.  Nothing else depends on it (addresses, widths, arithmetic, grid and LDS use are the same for
// every policy, so the outputs are bit-identical); the CPT loads and the ring's system-scope code loads
// are default-policy under all of them.  The default policy emits the source the golden files pin.
struct RowsPolicy {
  enum Stores { kStoreSc1 = 0, kStoreSc1Nt = 1, kStoreSc0Sc1Nt = 2 };  // all write-through (kRowsJitWriteThrough)
  bool nt_loads = false;  // evidence codes with the nontemporal hint
  int stores = kStoreSc1;
  bool is_default() const { return !nt_loads && stores == kStoreSc1; }
};

// validate and compile a plan (pl non-null); PGM_OK, or PGM_EINVAL with pgm_last_error set
PGM_ROWS_LOCAL int rows_plan_compile(const pgm_rows_plan *pl, RowsPlan &out);
// pgm_rows_plan_source without the copy-out: the specialisability check and the generated source
PGM_ROWS_LOCAL int rows_plan_source(const pgm_rows_plan *pl, std::string &src, const RowsPolicy &pol = RowsPolicy());

// the alignment / addressing contract of the two-rows-per-lane body (pgm_rows_jit2, pgm_rows_ring)
PGM_ROWS_LOCAL bool rows2_aligned(int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0, int64_t n_rows,
                                  const double *marg, int64_t ld_out, const int32_t *map, const double *gap,
                                  int n_marg);
// whether a launch runs the two-rows-per-thread kernel: big enough, and its alignment contract holds
// (else the one-row kernel runs)
PGM_ROWS_LOCAL bool rows_jit2_ok(int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0, int64_t n_rows,
                                 const double *marg, int64_t ld_out, const int32_t *map, const double *gap,
                                 int n_marg);

// The launch of a compiled plan: pgm_rows_plan_run's argument checks (rows_launch_check, in its order,
// with its messages), then which kernel runs, with which template arguments, grid and LDS
// (rows_launch_choose).  rows_plan_run, pgm_rows_plan_bind and pgm_rows_launch_info all go through
// these two, so what is reported is what runs.  jit: the plan-specialised kernel is compiled and loaded
// (callers ask for it only when rows_jit_mode(mode) holds and the plan has a generated source).
PGM_ROWS_LOCAL bool rows_jit_mode(int32_t mode);  // no mode bit rules the specialised kernel out
PGM_ROWS_LOCAL int rows_launch_check(const RowsPlan &p, int32_t mode, const uint8_t *codes, int64_t n_rows,
                                     const double *marg, const double *joint, int64_t ld_out, const int32_t *map,
                                     const double *gap);
PGM_ROWS_LOCAL int rows_launch_choose(const RowsPlan &p, int32_t mode, const uint8_t *codes, int64_t ld_codes,
                                      int64_t row0, int64_t n_rows, const double *marg, int64_t ld_out,
                                      const int32_t *map, const double *gap, bool jit, pgm_rows_launch_info_t *info);
// pgm_rows_launch_info without STALE_PROBE: compile, check, choose
PGM_ROWS_LOCAL int rows_launch_info(const pgm_rows_plan *pl, int32_t mode, const uint8_t *codes, int64_t ld_codes,
                                    int64_t row0, int64_t n_rows, const double *marg, const double *joint,
                                    int64_t ld_out, const int32_t *map, const double *gap, bool jit_available,
                                    pgm_rows_launch_info_t *info);

// launch geometry the generated source is written for (the launchers must use the same numbers)
PGM_ROWS_LOCAL int jit_wg();  // workgroup size of pgm_rows_jit / jit2 / floor / floor2
// workgroup size of the ring kernel: 256 = one wave per
// SIMD per workgroup; the loop around the two-row body takes ~147 VGPRs (3 waves per SIMD), so three
// workgroups are resident per CU (a 1,024-thread bound caps it at 128 VGPRs and spills to scratch;
// 512 threads fit one workgroup per CU)
static constexpr int ring_wg() { return 256; }

// output store form of the specialised kernels: write-through — 8-B relaxed agent-scope atomic stores /
// 16-B buffer stores with the sc1 bit — so every output line goes past the XCD's L2 in the dispatch that
// writes it (no dirty output left for an end-of-dispatch release to write back; measured MI355X, 100k
// rows: HIP launch 4.7 -> 3.8 us, direct queue 6.2 -> 4.0 us with the per-dispatch release dropped,
// WRITE_SIZE 13.28 MB per launch either way; r02 also measured plain (write-back) and nontemporal forms
// and rejected them — plain `nt` is not write-through; the streaming policy's stores are sc1 AND nt, with
// the same WRITE_SIZE: RowsPolicy above, the rule in pgmrows.hip)
static constexpr bool kRowsJitWriteThrough = true;

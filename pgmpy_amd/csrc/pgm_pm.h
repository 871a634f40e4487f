// pgm_pm.h — what pgmpm_gen.cpp (host only: the planner of the fused product + marginal step, the choice
// of its specialisation, the generators of the specialised sources) gives pgmpm.cpp (hipRTC, the loaded
// kernels, the bound launches) and the CPU self-test (tools/pm_gen_selftest.cpp).  No HIP here: plain
// structs in, a source string plus launch geometry out.  The planner itself (pgmi_plan_product_marg)
// and the plan structs are in pgm_internal.h, where pgmhip.hip sees them too.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "pgm_internal.h"

// two marginals of one product in a single pass (no product stored): block = one state of the dims
// both keep (K) x a row chunk; the dims only one of them keeps (U = R1 + R2) are unrolled at
// generation time with one register accumulator per R1 / R2 state; dims neither keeps (Z) are runtime
// inner loops.  Batched-BP distribute: a parent's sigma' for two child scopes from its operands.
struct PMMulti {
  int n_ops = 0;
  int kind[MOPS] = {}, vec[MOPS] = {};
  int nK = 0, nU = 0, nZ = 0;
  unsigned kcard[KMAX] = {}, ucard[KMAX] = {}, zcard[KMAX] = {};
  int64_t ks[MOPS][KMAX] = {}, k1[KMAX] = {}, k2[KMAX] = {};
  int64_t us[MOPS][KMAX] = {}, u1[KMAX] = {}, u2[KMAX] = {};
  int64_t zs[MOPS][KMAX] = {};
  uint32_t n_outer = 0, NP = 0;
  unsigned n1 = 1, n2 = 1;  // accumulators (R1 / R2 states)
};

struct PMSpec {  // one fused step's specialisation
  int multi = 0;  // 1: PMMulti body (two marginals), else the ProdMK body
  PMMulti mm;
  ProdMK k;
  int red = PGM_RED_SUM, XI = 1, unroll = 8;
  bool store = true, xcd = false, nt = false;
  bool has_m = true;  // false: the product alone (pgm_product_n_bind), no marginal
  unsigned gx = 1;
  uint64_t total = 0;  // blocks
  // marginal-only passes: a kept dim no row operand carries (only row-less operands such as psi vary along
  // it), walked inside the block — its T states share the loaded row-operand values (-1: none)
  int tdim = -1;
  unsigned T = 1;
};

// a merged launch's kernel arguments stay within 4 KB (512 pointers); bodies per merged launch (a block finds
// its body through a balanced tree of block-range compares, so the count costs log2 compares; r06: 64 -> 128,
// C4's level 1 holds 74 specialised steps)
static constexpr size_t kPmMaxArgPtrs = 512;
static constexpr size_t kPmMaxTablePtrs = 8192;  // a specialised contraction batch's pointers through a table
static constexpr int kPmMaxBodies = 128;

// the specialisation of a planned fused step (reduce: PGM_RED_SUM / PGM_RED_MAX; store: the product is
// written; has_m: the marginal is): row pairs per lane, entries unrolled, tiled kept dim, blocks.
// false: the generic kernel runs (fewer than 2^12 entries, or too many blocks for one grid)
bool pm_specialise(const ProdMK &k, int32_t reduce, bool store, bool has_m, PMSpec &sp);
// the two-marginal pass planned and specialised; 1 = supported (sp filled), 0 = not (the caller runs two
// passes), < 0 error
int plan_two_marginals(const pgm_productn_desc *d, const double *const *ops, const int64_t *s1, const int64_t *s2,
                       const double *M1, const double *M2, int32_t reduce, PMSpec &sp);
// operand pointers a body takes (its kernel arguments are these, then C and M)
int pm_nops(const PMSpec &sp);
// kernel pgm_pm over the bodies (kernel argument: each body's operand pointers, then C and M);
// starts[i] = first block of body i, *blocks = the grid size
std::string pm_source(const std::vector<PMSpec> &specs, std::vector<uint64_t> &starts, uint64_t *blocks);

// a specialised contraction batch: kernel pgm_pm of `blocks` workgroups of `threads`, its argument the flat
// pointer list (per job: A, B, C / A, codes, C, err / its operands, C) — or, when table, one pointer to
// that list in device memory
struct CSBatch {
  std::string src;
  unsigned blocks = 0, threads = 256;
  std::vector<const double *> ptrs;
  bool table = false;
};
// one_wg = 0: one launch of the batch's blocks (one level); 1: the single-workgroup levelled form
// (level_off: first block of each level + the end).  false: not a batch this form takes
bool cs_source(const pgmi_cs_job *jobs, int n, const uint32_t *level_off, int n_levels, int one_wg, CSBatch &out);

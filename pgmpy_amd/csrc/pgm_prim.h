// pgm_prim.h — private interface between the two units of the primitive factor operations: pgmprim_plan.cpp
// (host only: descriptor validation, dim coalescing, the choice of kernel and geometry, batch job assembly,
// and the entry points that never touch the device) and pgmhip.hip (the kernels, the template launch
// switches, the batch's device allocations, the launches).  Not part of include/pgmhip.h.  ContractK,
// GatherK and ContractNK, which the specialised batch kernels also take, are pgm_internal.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pgm_internal.h"
#include "pgmhip.h"

// ---------------------------------------------------------------------------- what the kernels read
#define RTAB_MAX 512  // reduction offsets of k_contract_rows_tab / _tab2 (their LDS tables)

// a planned n-ary product (k_productn, k_productn_rows2, the product jobs of a batch)
struct ProdNK {
  int32_t n_ops, nk;
  int32_t kind[PMAX];
  uint32_t n_out, row_mode;
  uint32_t pairs, _pad;  // batched jobs: two innermost elements per lane with 16-B accesses
  FDiv kdiv[KMAX];
  int64_t ksc[KMAX];
  int64_t ks[PMAX][KMAX];
  const double *ops[PMAX];
};

// one job of a batch as k_batch / k_batch_c / k_batch_p read it
struct BatchJob {
  int32_t kind, cmb, red, _pad;  // kind 0: contraction, 1: gather, 2: n-ary product, 3: findings indicator
  int64_t ind_rows, ind_card, ind_s_state, ind_s_row;
  uint32_t block0, nblocks;
  const double *A, *B;
  double *C;
  const uint8_t *codes;
  int32_t *err;
  ContractK c;
  GatherK g;
  ProdNK pn;
};

// A single-workgroup levelled batch of contractions only (the tail of a contraction path, C1 / C2): the
// job descriptors (contraction part only), the block map and the level table are copied into LDS once at
// the start — every load of them independent, issued together — so each level's blocks read their
// descriptor from LDS instead of a block-map load followed by a dependent descriptor load from memory
// (two round trips per level).  Same per-job code as k_batch_c, so the same results bit for bit.
struct alignas(16) ChainJob {
  int32_t cmb, red;
  uint32_t block0, nblocks;
  const double *A, *B;
  double *C;
  ContractK c;
};

struct BatchHandle {
  std::vector<BatchJob> jobs;
  std::vector<uint32_t> block_job;
  std::vector<uint32_t> level_off{0};  // single-workgroup levelled batch: first block of each level (+ the end)
  BatchJob *d_jobs = nullptr;
  uint32_t *d_map = nullptr;
  uint32_t *d_level = nullptr;
  int32_t mode = PGM_BATCH_GRID;  // PGM_BATCH_ONE_WORKGROUP: k_batch_wg_c
  int32_t spec = -1;  // every job a contraction with one (combine, reduce): combine * 3 + reduce; products: 100
  ChainJob *d_chain = nullptr;  // ONE_WORKGROUP batch (contractions only): descriptors staged in LDS
  size_t chain_lds = 0;         // dynamic LDS bytes of k_batch_wg_c
  // r06: n-ary contraction jobs (kind 4; BatchJob::_pad indexes these): specialised kernel only
  std::vector<ContractNK> njobs;
  std::vector<std::vector<const double *>> nops;
};

static const int32_t kBatchSpecProducts = 100;  // BatchHandle::spec of a products-only batch
// single-workgroup chains of contractions: descriptors, block map and level table staged in LDS
// (k_batch_wg_c) up to this many bytes
static const size_t kChainLdsMax = 48 * 1024;

// ---------------------------------------------------------------------------- the planner (pgmprim_plan.cpp)
namespace pgmprim {

// Loop dims with one stride row per operand (and, for kept dims, a last row for the output).
struct Dims {
  int n = 0;     // dims, the last fastest
  int nops = 0;  // stride rows in use
  int64_t card[PGM_MAX_DIMS];
  int64_t s[MOPS + 1][PGM_MAX_DIMS];
};
// drop extent-1 dims, merge a dim into its outer neighbour where every row steps through the two as one
// (outer stride == extent * stride).  The caller has checked the extents.
void coalesce(Dims &d);

// row mode: y-blocks over the outer kept index, x-blocks over the chunks of the innermost kept dim, about
// kRowTargetBlocks blocks in all
static const uint64_t kRowTargetBlocks = 2048;
void row_grid(uint64_t n_outer, uint64_t xchunks, uint32_t grid[3]);
// log2 of the lanes that share one output's reduction: doubled up to 64 while the job has fewer than `cap`
// lanes and the lanes do not outnumber `extent`
int lanes_log2(uint64_t n_out, uint64_t cap, uint64_t extent);
static const uint64_t kTargetThreads = 256ull * 2048;  // a stand-alone launch's cap: 256 CUs x 32 waves x 64 lanes

struct ContractLaunch {
  ContractK k;
  uint32_t grid[3];
  uint64_t ws_doubles;
  bool empty;
};
int plan_contract(const pgm_contract_desc *d, ContractLaunch &L);
// two-rows-per-lane eligibility of a row-mode COPY contraction (A read, C written)
bool rows2_ok(const ContractK &k, const double *A, const double *C);
// the kernel a planned contraction runs (enum pgm_contract_kernel) and its grid: the one place that
// decides it, for the launcher and for pgm_contract_info
int contract_kernel(const ContractLaunch &L, int combine, int reduce, const double *A, const double *C,
                    uint32_t grid[3]);
// output pairs (16-B accesses) for a batch's flat-mode contraction job with one lane per output
bool contract_pairs_ok(const ContractK &k, int combine, const double *A, const double *B, const double *C);

// descriptor -> kernel parameters (coalesced dims, aliased unused operand slots); shared by
// pgm_product_n and the batched product_n job
int plan_prodn(const pgm_productn_desc *d, const double *const *ops, ProdNK &k);
// two innermost elements per lane with 16-B accesses (k_productn_rows2, prodn_flat2): even innermost
// extent, output innermost stride 1, every operand's innermost stride 0 or 1, the bases and outer
// strides of every 16-B accessed array even
bool prodn_pairs_ok(const ProdNK &k, const double *C);

int plan_gather(const pgm_gather_desc *d, GatherK &k);

// an n-ary contraction's plan: unit dims dropped, adjacent dims merged where every operand (and C, for
// kept dims) steps through them as one, G lanes per output for long reductions of few outputs
int plan_contract_n(const pgm_contractn_desc *d, const double *const *ops, ContractNK &k, bool need_ops = true);
// an n-ary job's lanes and block cap in a batch (pgm_batch_add_contract_n and pgm_contract_n_info)
uint64_t contract_n_threads(const ContractNK &k);
uint64_t contract_n_cap(const ContractNK &k);

// 256-thread blocks a batch job of `threads` lanes takes (cap 0: PGM_BATCH_MAX_BLOCKS; its lanes grid-stride beyond)
uint64_t batch_job_blocks(uint64_t threads, uint64_t cap = 0);
int batch_append(BatchHandle *h, BatchJob &J, uint64_t threads, uint64_t cap = 0);
// what pgm_batch_finalize settles before it touches the device: the last level closed, BatchHandle::spec,
// the two refusals of a single-workgroup batch, and that mode's ChainJob table with its LDS bytes
int batch_close(BatchHandle *h, std::vector<ChainJob> &chain, size_t &chain_lds);

}  // namespace pgmprim

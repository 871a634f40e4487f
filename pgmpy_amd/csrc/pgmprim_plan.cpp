// pgmprim_plan.cpp — the host side of the primitive factor operations (include/pgmhip.h: pgm_contract,
// pgm_product_n, pgm_gather, the pgm_batch_* jobs): descriptor validation, dim coalescing, the choice of
// kernel and launch geometry, the assembly of batch jobs, and the entry points that never touch the device
// (pgm_contract_workspace, pgm_contract_info, pgm_contract_n_info, pgm_batch_add_*, pgm_batch_set_mode,
// pgm_batch_blocks, pgm_batch_add_level).  No HIP call and no HIP include: a stand-alone CPU program drives
// all of it (tools/prim_plan_selftest.cpp).  The kernels and launches are pgmhip.hip.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "pgm_prim.h"

namespace pgmprim {

// ----------------------------------------------------------------------------- the shared rules
void coalesce(Dims &d) {
  int n = 0;  // dims written so far: in place, n <= i
  for (int i = 0; i < d.n; ++i) {
    const int64_t card = d.card[i];
    if (card == 1) continue;
    bool merge = n > 0;
    for (int t = 0; merge && t < d.nops; ++t) merge = d.s[t][n - 1] == card * d.s[t][i];
    const int j = merge ? n - 1 : n++;
    d.card[j] = merge ? d.card[j] * card : card;
    for (int t = 0; t < d.nops; ++t) d.s[t][j] = d.s[t][i];
  }
  d.n = n;
}

void row_grid(uint64_t n_outer, uint64_t xchunks, uint32_t grid[3]) {
  const uint64_t gy = std::min<uint64_t>(n_outer, 65535);
  grid[0] = (uint32_t)std::min<uint64_t>(xchunks, std::max<uint64_t>(1, kRowTargetBlocks / gy));
  grid[1] = (uint32_t)gy;
  grid[2] = 1;
}

int lanes_log2(uint64_t n_out, uint64_t cap, uint64_t extent) {
  int g = 0;
  while (g < 6 && (n_out << g) < cap && (1ull << (g + 1)) <= extent) ++g;
  return g;
}

static uint64_t env_u64(const char *name, uint64_t dflt) {
  const char *v = getenv(name);
  return v && *v ? strtoull(v, nullptr, 10) : dflt;
}
// a batch contraction job with a reduction takes G lanes per output (G a power of two up to the innermost
// reduction extent) while its outputs x G stay under this many lanes (r04: 32 K / 128 K slower on C2,
// profiles/r04p/)
static const uint64_t kBatchLanesCap = env_u64("PGM_BATCH_LANES_CAP", 4096);
// workgroups one batch job may take (its lanes grid-stride over the job's outputs beyond that; r04:
// 1,024 / 4,096 no faster on C1 / C2 / C4, profiles/r04j/)
static const uint64_t kBatchMaxBlocks = env_u64("PGM_BATCH_MAX_BLOCKS", 256);
// a batch contraction without a reduction (a broadcast product or a copy: one load per operand per output)
// may take more workgroups than one that reduces: its lanes otherwise walk several outputs one after
// another, a full memory round trip each (C2's 448,000-output product level: 11.7 -> 8.9 us at 1,024
// blocks, profiles/r04t/), while the reducing jobs of a level were measured slower with more
static const uint64_t kBatchMaxBlocksProduct = env_u64("PGM_BATCH_MAX_BLOCKS_PRODUCT", 1024);

// ----------------------------------------------------------------------------- contract
int plan_contract(const pgm_contract_desc *d, ContractLaunch &L) {
  if (!d) return pgmi_failf(PGM_EINVAL, "contract: null descriptor");
  if (d->n_keep < 0 || d->n_keep > PGM_MAX_DIMS || d->n_red < 0 || d->n_red > PGM_MAX_DIMS)
    return pgmi_failf(PGM_EINVAL, "contract: n_keep/n_red out of range (%d, %d)", d->n_keep, d->n_red);
  if (d->combine < 0 || d->combine > 4 || d->reduce < 0 || d->reduce > 2)
    return pgmi_failf(PGM_EINVAL, "contract: bad combine/reduce (%d, %d)", d->combine, d->reduce);
  if (d->reduce == PGM_RED_NONE && d->n_red > 0)
    return pgmi_failf(PGM_EINVAL, "contract: reduction dims given with PGM_RED_NONE");
  Dims kd, rd;  // kept: A, B, C; reduced: A, B
  kd.n = d->n_keep;
  kd.nops = 3;
  uint64_t n_out = 1, n_red = 1;
  for (int i = 0; i < d->n_keep; ++i) {
    if (d->keep_card[i] <= 0) return pgmi_failf(PGM_EINVAL, "contract: keep_card[%d] = %lld", i, (long long)d->keep_card[i]);
    kd.card[i] = d->keep_card[i];
    kd.s[0][i] = d->keep_sa[i];
    kd.s[1][i] = d->keep_sb[i];
    kd.s[2][i] = d->keep_sc[i];
    n_out *= (uint64_t)d->keep_card[i];
  }
  rd.n = d->n_red;
  rd.nops = 2;
  for (int i = 0; i < d->n_red; ++i) {
    if (d->red_card[i] <= 0) return pgmi_failf(PGM_EINVAL, "contract: red_card[%d] = %lld", i, (long long)d->red_card[i]);
    rd.card[i] = d->red_card[i];
    rd.s[0][i] = d->red_sa[i];
    rd.s[1][i] = d->red_sb[i];
    n_red *= (uint64_t)d->red_card[i];
  }
  if (n_out >= (1ull << 31) || n_red >= (1ull << 31))
    return pgmi_failf(PGM_EINVAL, "contract: index space too large (%llu x %llu; limit 2^31 each)",
                      (unsigned long long)n_out, (unsigned long long)n_red);
  coalesce(kd);
  coalesce(rd);
  // few outputs (flat mode) and one long reduction run: cut the run into (outer x chunk) so the
  // split-K below has reduction-outer indices to distribute (a batched dot product over a packed
  // operand pair would otherwise leave 64 lanes per output walking the whole run)
  if (d->reduce != PGM_RED_NONE && rd.n > 0 && rd.n < KMAX && kd.n <= KMAX && n_out <= 4096 &&
      !(kd.n > 0 && kd.card[kd.n - 1] >= 64)) {
    const int64_t ri = rd.card[rd.n - 1];
    if (ri >= 8192 && n_red / (uint64_t)ri < 256) {
      for (int64_t c = 4096; c >= 256; c >>= 1) {
        if (ri % c) continue;
        const int last = rd.n - 1;
        rd.card[rd.n] = c;
        rd.s[0][rd.n] = rd.s[0][last];
        rd.s[1][rd.n] = rd.s[1][last];
        rd.card[last] = ri / c;
        rd.s[0][last] *= c;
        rd.s[1][last] *= c;
        ++rd.n;
        break;
      }
    }
  }
  if (kd.n > KMAX || rd.n > KMAX)
    return pgmi_failf(PGM_EINVAL, "contract: %d keep / %d reduce dims after coalescing (limit %d)", kd.n, rd.n, KMAX);
  ContractK &k = L.k;
  memset(&k, 0, sizeof k);
  k.nk = kd.n;
  k.nr = rd.n;
  for (int i = 0; i < kd.n; ++i) {
    k.kdiv[i] = make_fdiv((uint32_t)kd.card[i]);
    k.ksa[i] = kd.s[0][i];
    k.ksb[i] = kd.s[1][i];
    k.ksc[i] = kd.s[2][i];
  }
  for (int i = 0; i < rd.n; ++i) {
    k.rdiv[i] = make_fdiv((uint32_t)rd.card[i]);
    k.rsa[i] = rd.s[0][i];
    k.rsb[i] = rd.s[1][i];
  }
  k.n_out = (uint32_t)n_out;
  k.n_red = (uint32_t)n_red;
  L.empty = (n_out == 0);
  // reduction = outer (decoded, wave-uniform) x innermost (walked by increments)
  if (rd.n > 0) {
    k.ri_card = (uint32_t)rd.card[rd.n - 1];
    k.ri_sa = rd.s[0][rd.n - 1];
    k.ri_sb = rd.s[1][rd.n - 1];
  } else {
    k.ri_card = 1;
    k.ri_sa = k.ri_sb = 0;
  }
  k.n_ro = (uint32_t)(n_red / k.ri_card);
  const bool has_red = d->reduce != PGM_RED_NONE && n_red > 1;
  const uint64_t NX = kd.n > 0 ? (uint64_t)kd.card[kd.n - 1] : 1;
  // row mode when the innermost output dim fills waves and no lane-parallel reduction is needed
  const bool red_contig = rd.n > 0 && rd.s[0][rd.n - 1] == 1;
  k.row_mode = (kd.n > 0 && NX >= 64 && !(has_red && red_contig && NX < 256 && n_out < kTargetThreads)) ? 1 : 0;
  int g_log2 = 0;
  uint32_t n_split = 1;
  if (k.row_mode) {
    row_grid(n_out / NX, (NX + 255) / 256, L.grid);
    const uint64_t blocks = (uint64_t)L.grid[0] * L.grid[1];
    k.ri_chunk = k.ri_card;
    k.ri_nb = 1;
    if (has_red && blocks < kRowTargetBlocks / 2) {
      // few outputs and a long reduction: split it (virtual outer index = (ro, chunk of the inner dim))
      const uint64_t want = (kRowTargetBlocks / 2 + blocks - 1) / blocks;
      if (k.n_ro < want && k.ri_card >= 64) {
        const uint64_t nb = std::min<uint64_t>((want + k.n_ro - 1) / k.n_ro, k.ri_card / 16);
        k.ri_nb = (uint32_t)std::max<uint64_t>(nb, 1);
        k.ri_chunk = (uint32_t)((k.ri_card + k.ri_nb - 1) / k.ri_nb);
        k.ri_nb = (k.ri_card + k.ri_chunk - 1) / k.ri_chunk;
      }
      n_split = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(want, (uint64_t)k.n_ro * k.ri_nb), 256);
    }
    k.n_v = k.n_ro * k.ri_nb;
    L.grid[2] = n_split;
  } else {
    if (has_red) {
      g_log2 = lanes_log2(n_out, kTargetThreads, k.ri_card);
      const uint64_t par = n_out << g_log2;
      if (par < kTargetThreads / 4 && k.n_ro > 1) {
        uint64_t want = (kTargetThreads / 4 + par - 1) / par;
        n_split = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(want, k.n_ro), 1024);
      }
    }
    const uint64_t threads = n_out << g_log2;
    uint64_t blocks = (threads + 255) / 256;
    blocks = std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 65535);
    L.grid[0] = (uint32_t)blocks;
    L.grid[1] = n_split;
    L.grid[2] = 1;
  }
  k.g_log2 = g_log2;
  k.n_split = (int32_t)n_split;
  k.red_chunk = k.row_mode ? (uint32_t)((k.n_v + n_split - 1) / n_split) : (uint32_t)((k.n_ro + n_split - 1) / n_split);
  L.ws_doubles = n_split > 1 ? (uint64_t)n_split * n_out : 0;
  return PGM_OK;
}

// (r01's 8-B-only row paths ran at 0.54-0.70x the 16-B rate)
bool rows2_ok(const ContractK &k, const double *A, const double *C) {
  if (!k.row_mode || k.nk < 1) return false;
  const int kx = k.nk - 1;
  if (k.kdiv[kx].d % 2 || k.ksa[kx] != 1 || k.ksc[kx] != 1) return false;
  if (((uintptr_t)A & 15) || ((uintptr_t)C & 15)) return false;
  for (int i = 0; i < kx; ++i)
    if (k.ksa[i] % 2 || k.ksc[i] % 2) return false;
  for (int i = 0; i < k.nr; ++i)
    if (k.rsa[i] % 2) return false;
  return k.nr == 0 || k.ri_sa % 2 == 0;
}

int contract_kernel(const ContractLaunch &L, int combine, int reduce, const double *A, const double *C,
                    uint32_t grid[3]) {
  memcpy(grid, L.grid, sizeof L.grid);
  if (!L.k.row_mode) return PGM_CK_FLAT;
  if (reduce == PGM_RED_NONE || L.k.n_split != 1 || L.k.ri_nb != 1 || L.k.n_red > RTAB_MAX) return PGM_CK_ROWS;
  if (combine != PGM_COMBINE_COPY || !rows2_ok(L.k, A, C)) return PGM_CK_ROWS_TAB;
  grid[0] = (uint32_t)std::max<uint64_t>(1, (grid[0] + 1) / 2);
  return PGM_CK_ROWS_TAB2;
}

// every access along the innermost kept dim aligned and unit-stride (or broadcast); host check of contract_flat2
bool contract_pairs_ok(const ContractK &k, int combine, const double *A, const double *B, const double *C) {
  const int kx = k.nk - 1;
  const bool use_b = combine != PGM_COMBINE_COPY;
  bool pairs = kx >= 0 && k.kdiv[kx].d % 2 == 0 && k.ksc[kx] == 1 && ((uintptr_t)C & 15) == 0;
  const bool va = pairs && k.ksa[kx] != 0, vb = pairs && use_b && k.ksb[kx] != 0;
  pairs = pairs && (k.ksa[kx] == 0 || k.ksa[kx] == 1) && (!use_b || k.ksb[kx] == 0 || k.ksb[kx] == 1);
  for (int i = 0; pairs && i < kx; ++i) pairs = k.ksc[i] % 2 == 0 && (!va || k.ksa[i] % 2 == 0) && (!vb || k.ksb[i] % 2 == 0);
  for (int i = 0; pairs && i + 1 < k.nr; ++i) pairs = (!va || k.rsa[i] % 2 == 0) && (!vb || k.rsb[i] % 2 == 0);
  if (pairs) pairs = (!va || (k.ri_sa % 2 == 0 && ((uintptr_t)A & 15) == 0)) && (!vb || (k.ri_sb % 2 == 0 && ((uintptr_t)B & 15) == 0));
  return pairs;
}

// ----------------------------------------------------------------------------- n-ary product
int plan_prodn(const pgm_productn_desc *d, const double *const *ops, ProdNK &k) {
  if (!d || !ops) return pgmi_failf(PGM_EINVAL, "product_n: null argument");
  if (d->n_ops < 1 || d->n_ops > PMAX || d->n_keep < 0 || d->n_keep > PGM_MAX_DIMS)
    return pgmi_failf(PGM_EINVAL, "product_n: n_ops %d (1..%d) / n_keep %d", d->n_ops, PMAX, d->n_keep);
  Dims kd;  // the operands, then C
  kd.n = d->n_keep;
  kd.nops = d->n_ops + 1;
  uint64_t n_out = 1;
  for (int i = 0; i < d->n_keep; ++i) {
    if (d->keep_card[i] <= 0) return pgmi_failf(PGM_EINVAL, "product_n: keep_card[%d] <= 0", i);
    n_out *= (uint64_t)d->keep_card[i];
    kd.card[i] = d->keep_card[i];
    for (int t = 0; t < d->n_ops; ++t) kd.s[t][i] = d->keep_s[t][i];
    kd.s[d->n_ops][i] = d->keep_sc[i];
  }
  coalesce(kd);
  const int n = kd.n;
  if (n_out >= (1ull << 31)) return pgmi_failf(PGM_EINVAL, "product_n: output too large");
  if (n > KMAX) return pgmi_failf(PGM_EINVAL, "product_n: %d dims after coalescing (limit %d)", n, KMAX);
  memset(&k, 0, sizeof k);
  k.n_ops = d->n_ops;
  k.nk = n;
  k.n_out = (uint32_t)n_out;
  for (int i = 0; i < n; ++i) {
    k.kdiv[i] = make_fdiv((uint32_t)kd.card[i]);
    k.ksc[i] = kd.s[d->n_ops][i];
    for (int t = 0; t < d->n_ops; ++t) k.ks[t][i] = kd.s[t][i];
  }
  for (int t = 0; t < d->n_ops; ++t) {
    if (!ops[t]) return pgmi_failf(PGM_EINVAL, "product_n: null operand %d", t);
    k.ops[t] = ops[t];
    k.kind[t] = d->op_kind[t];
    if (d->op_kind[t] < 0 || d->op_kind[t] > 2) return pgmi_failf(PGM_EINVAL, "product_n: bad op_kind[%d]", t);
    if (d->op_kind[t] == PGM_PRODN_RATIO && (t + 1 >= d->n_ops || d->op_kind[t + 1] != PGM_PRODN_DEN))
      return pgmi_failf(PGM_EINVAL, "product_n: a RATIO operand must be followed by its DEN operand");
    if (d->op_kind[t] == PGM_PRODN_DEN && (t == 0 || d->op_kind[t - 1] != PGM_PRODN_RATIO))
      return pgmi_failf(PGM_EINVAL, "product_n: a DEN operand must follow a RATIO operand");
  }
  for (int t = d->n_ops; t < PMAX; ++t) {  // unused slots alias operand 0 with stride 0 (valid loads)
    k.ops[t] = k.ops[0];
    k.kind[t] = PGM_PRODN_MUL;
    for (int i = 0; i < n; ++i) k.ks[t][i] = 0;
  }
  const uint64_t NX = n > 0 ? (uint64_t)kd.card[n - 1] : 1;
  k.row_mode = (n > 0 && NX >= 64) ? 1 : 0;
  return PGM_OK;
}

bool prodn_pairs_ok(const ProdNK &k, const double *C) {
  const int kx = k.nk - 1;
  bool pairs = kx >= 0 && k.kdiv[kx].d % 2 == 0 && k.ksc[kx] == 1 && ((uintptr_t)C & 15) == 0;
  for (int i = 0; pairs && i < kx; ++i) pairs = k.ksc[i] % 2 == 0;
  for (int t = 0; pairs && t < k.n_ops; ++t) {
    const int64_t sx = k.ks[t][kx];
    pairs = sx == 0 || (sx == 1 && ((uintptr_t)k.ops[t] & 15) == 0);
    for (int i = 0; pairs && sx == 1 && i < kx; ++i) pairs = k.ks[t][i] % 2 == 0;
  }
  return pairs;
}

// ----------------------------------------------------------------------------- gather
int plan_gather(const pgm_gather_desc *d, GatherK &k) {
  if (d->n_keep < 0 || d->n_keep > KMAX || d->n_ev < 0 || d->n_ev > PGM_MAX_DIMS)
    return pgmi_failf(PGM_EINVAL, "gather: n_keep %d (limit %d) / n_ev %d", d->n_keep, KMAX, d->n_ev);
  if (d->batch_dim >= d->n_keep) return pgmi_failf(PGM_EINVAL, "gather: batch_dim out of range");
  memset(&k, 0, sizeof k);
  k.nk = d->n_keep;
  k.n_ev = d->n_ev;
  k.batch_dim = d->batch_dim;
  k.ld = d->ld;
  k.row0 = d->row0;
  uint64_t n_out = 1;
  for (int i = 0; i < d->n_keep; ++i) {
    if (d->keep_card[i] <= 0) return pgmi_failf(PGM_EINVAL, "gather: keep_card[%d] <= 0", i);
    n_out *= (uint64_t)d->keep_card[i];
    k.kdiv[i] = make_fdiv((uint32_t)d->keep_card[i]);
    k.ksa[i] = d->keep_sa[i];
    k.ksc[i] = d->keep_sc[i];
  }
  if (n_out >= (1ull << 31)) return pgmi_failf(PGM_EINVAL, "gather: output too large");
  for (int j = 0; j < d->n_ev; ++j) {
    k.ev_col[j] = d->ev_col[j];
    k.ev_stride[j] = d->ev_stride[j];
    k.ev_card[j] = (int32_t)d->ev_card[j];
  }
  k.n_out = (uint32_t)n_out;
  return PGM_OK;
}

// ----------------------------------------------------------------------------- n-ary contraction
int plan_contract_n(const pgm_contractn_desc *d, const double *const *ops, ContractNK &k, bool need_ops) {
  if (!d || (need_ops && !ops)) return pgmi_failf(PGM_EINVAL, "contract_n: null argument");
  const int n = d->n_ops;
  if (n < 1 || n > MOPS) return pgmi_failf(PGM_EINVAL, "contract_n: %d operands (1..%d)", n, MOPS);
  if (d->reduce != PGM_RED_SUM && d->reduce != PGM_RED_MAX) return pgmi_failf(PGM_EINVAL, "contract_n: reduce must be sum or max");
  if (d->n_keep < 0 || d->n_keep > PGM_MAX_DIMS || d->n_red < 0 || d->n_red > PGM_MAX_DIMS)
    return pgmi_failf(PGM_EINVAL, "contract_n: %d kept / %d reduced dims", d->n_keep, d->n_red);
  for (int t = 0; need_ops && t < n; ++t)
    if (!ops[t]) return pgmi_failf(PGM_EINVAL, "contract_n: operand %d is null", t);
  memset(&k, 0, sizeof k);
  k.n_ops = n;
  k.red = d->reduce;
  for (int i = 0; i < d->n_keep; ++i)
    if (d->keep_card[i] == 0) {
      k.n_out = 0;
      return PGM_OK;  // empty output: nothing to do
    }
  // kept dims (C-order: the last fastest; the operands, then C), then reduced dims (the operands)
  Dims kd, rd;
  kd.n = d->n_keep;
  kd.nops = n + 1;
  for (int i = 0; i < d->n_keep; ++i) {
    if (d->keep_card[i] < 0) return pgmi_failf(PGM_EINVAL, "contract_n: negative cardinality");
    kd.card[i] = d->keep_card[i];
    for (int t = 0; t < n; ++t) kd.s[t][i] = d->keep_s[t][i];
    kd.s[n][i] = d->keep_sc[i];
  }
  rd.n = d->n_red;
  rd.nops = n;
  for (int i = 0; i < d->n_red; ++i) {
    if (d->red_card[i] < 0) return pgmi_failf(PGM_EINVAL, "contract_n: negative cardinality");
    rd.card[i] = d->red_card[i];
    for (int t = 0; t < n; ++t) rd.s[t][i] = d->red_s[t][i];
  }
  coalesce(kd);
  coalesce(rd);
  if (kd.n > KMAX || rd.n > KMAX)
    return pgmi_failf(PGM_EINVAL, "contract_n: %zu kept / %zu reduced dims after merging (at most %d each)", (size_t)kd.n,
                      (size_t)rd.n, KMAX);
  uint64_t n_out = 1, n_red = 1;
  k.nk = kd.n;
  k.nr = rd.n;
  for (int i = 0; i < k.nk; ++i) {
    n_out *= (uint64_t)kd.card[i];
    if (n_out > 0x7fffffffull) return pgmi_failf(PGM_EINVAL, "contract_n: output over 2^31 entries");
    k.kcard[i] = (uint32_t)kd.card[i];
    k.ksc[i] = kd.s[n][i];
    for (int t = 0; t < n; ++t) k.ks[t][i] = kd.s[t][i];
  }
  for (int i = 0; i < k.nr; ++i) {
    if (rd.card[i] == 0) {
      n_red = 0;
      break;
    }
    n_red *= (uint64_t)rd.card[i];
    if (n_red > 0x7fffffffull) return pgmi_failf(PGM_EINVAL, "contract_n: reduction over 2^31 entries");
    k.rcard[i] = (uint32_t)rd.card[i];
    for (int t = 0; t < n; ++t) k.rs[t][i] = rd.s[t][i];
  }
  if (n_red == 0) return pgmi_failf(PGM_EINVAL, "contract_n: an empty reduction");
  k.n_out = (uint32_t)n_out;
  k.n_red = (uint32_t)n_red;
  // lanes per output: up to 64 while the job's lanes stay under 4x a batch contraction's cap (a fused
  // step's reduction is a walk of dependent load rounds; more lanes, fewer rounds each)
  static const uint64_t nary_lanes = env_u64("PGM_NARY_LANES", 4 * kBatchLanesCap);
  k.g_log2 = k.nr > 0 ? lanes_log2(k.n_out, nary_lanes, n_red) : 0;
  return PGM_OK;
}

uint64_t contract_n_threads(const ContractNK &k) { return (uint64_t)k.n_out << k.g_log2; }
uint64_t contract_n_cap(const ContractNK &k) { return k.nr == 0 ? kBatchMaxBlocksProduct : 0; }

// ----------------------------------------------------------------------------- batched small jobs
uint64_t batch_job_blocks(uint64_t threads, uint64_t cap) {
  return std::min<uint64_t>(std::max<uint64_t>((threads + 255) / 256, 1), cap ? cap : kBatchMaxBlocks);
}

int batch_append(BatchHandle *h, BatchJob &J, uint64_t threads, uint64_t cap) {
  if (h->d_jobs) return pgmi_failf(PGM_EINVAL, "batch: already finalized");
  const uint64_t nb = batch_job_blocks(threads, cap);
  if (h->block_job.size() + nb > 0x7fffffffull) return pgmi_failf(PGM_EINVAL, "batch: too many blocks");
  J.block0 = (uint32_t)h->block_job.size();
  J.nblocks = (uint32_t)nb;
  h->block_job.insert(h->block_job.end(), nb, (uint32_t)h->jobs.size());
  h->jobs.push_back(J);
  return PGM_OK;
}

int batch_close(BatchHandle *h, std::vector<ChainJob> &chain, size_t &chain_lds) {
  if (h->level_off.back() < h->block_job.size()) h->level_off.push_back((uint32_t)h->block_job.size());
  h->spec = -1;
  bool uni = true, prod = true, contract_only = true;
  for (const BatchJob &J : h->jobs) {
    uni = uni && J.kind == 0 && J.cmb == h->jobs[0].cmb && J.red == h->jobs[0].red;
    prod = prod && J.kind == 2;
    contract_only = contract_only && (J.kind == 0 || J.kind == 4);  // (kind 4: specialised kernel only)
  }
  if (uni) h->spec = h->jobs[0].cmb * 3 + h->jobs[0].red;
  if (prod) h->spec = kBatchSpecProducts;
  chain.clear();
  chain_lds = h->jobs.size() * sizeof(ChainJob) + 4 * (h->block_job.size() + h->level_off.size());
  if (h->mode != PGM_BATCH_ONE_WORKGROUP) return PGM_OK;
  if (!contract_only) return pgmi_failf(PGM_EINVAL, "batch_finalize: a single-workgroup batch takes contractions only");
  if (chain_lds > kChainLdsMax)
    return pgmi_failf(PGM_EINVAL, "batch_finalize: single-workgroup tables of %zu bytes exceed the LDS budget", chain_lds);
  chain.resize(h->jobs.size());  // k_batch_wg_c: the staged descriptors
  for (size_t i = 0; i < h->jobs.size(); ++i) {
    const BatchJob &J = h->jobs[i];
    ChainJob &c = chain[i];
    memset(&c, 0, sizeof c);
    c.cmb = J.cmb;
    c.red = J.red;
    c.block0 = J.block0;
    c.nblocks = J.nblocks;
    c.A = J.A;
    c.B = J.B;
    c.C = J.C;
    c.c = J.c;
  }
  return PGM_OK;
}

}  // namespace pgmprim

using namespace pgmprim;

// ============================================================================= C-ABI (host only)
extern "C" {

int pgm_contract_workspace(const pgm_contract_desc *d, size_t *bytes) {
  STALE_PROBE();
  if (!bytes) return pgmi_failf(PGM_EINVAL, "null pointer");
  ContractLaunch L;
  int rc = plan_contract(d, L);
  if (rc) return rc;
  *bytes = L.ws_doubles * sizeof(double);
  return PGM_OK;
}

int pgm_contract_info(const pgm_contract_desc *d, const double *A, const double *C, pgm_contract_info_t *info) {
  if (!info) return pgmi_failf(PGM_EINVAL, "null pointer");
  ContractLaunch L;
  int rc = plan_contract(d, L);
  if (rc) return rc;
  memset(info, 0, sizeof *info);
  const ContractK &k = L.k;
  info->kernel = contract_kernel(L, d->combine, d->reduce, A, C, info->grid);
  info->g_log2 = k.g_log2;
  info->n_split = (uint32_t)k.n_split;
  info->red_chunk = k.red_chunk;
  info->ri_nb = k.ri_nb;
  info->ri_chunk = k.ri_chunk;
  info->n_ro = k.n_ro;
  info->n_v = k.n_v;
  info->n_out = k.n_out;
  info->n_red = k.n_red;
  info->ri_card = k.ri_card;
  const uint64_t NX = k.nk > 0 ? k.kdiv[k.nk - 1].d : 1;
  info->nx = (uint32_t)NX;
  info->unrolled = info->kernel == PGM_CK_ROWS && d->reduce == PGM_RED_NONE && NX > 3ull * info->grid[0] * 256;
  // split s covers reduction-outer indices [s * red_chunk, ...): empty once that start is past the end
  const uint64_t units = k.row_mode ? k.n_v : k.n_ro;
  const uint64_t used = k.red_chunk ? (units + k.red_chunk - 1) / k.red_chunk : 0;
  info->empty_splits = (uint32_t)((uint64_t)k.n_split > used ? (uint64_t)k.n_split - used : 0);
  return PGM_OK;
}

int pgm_contract_n_info(const pgm_contractn_desc *d, const double *const *ops, pgm_contractn_info_t *info) {
  if (!info) return pgmi_failf(PGM_EINVAL, "contract_n_info: null pointer");
  ContractNK k;
  int rc = plan_contract_n(d, ops, k, false);
  if (rc != PGM_OK) return rc;
  memset(info, 0, sizeof *info);
  info->nk = k.nk;
  info->nr = k.nr;
  info->g_log2 = k.g_log2;
  info->n_out = k.n_out;
  info->n_red = k.n_red;
  for (int i = 0; i < k.nk; ++i) info->kcard[i] = k.kcard[i];
  for (int i = 0; i < k.nr; ++i) info->rcard[i] = k.rcard[i];
  info->blocks = k.n_out ? (uint32_t)batch_job_blocks(contract_n_threads(k), contract_n_cap(k)) : 0;
  return PGM_OK;
}

int pgm_batch_add_contract(void *handle, const pgm_contract_desc *d, const double *A, const double *B, double *C) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h || !A || !C) return pgmi_failf(PGM_EINVAL, "batch_add_contract: null argument");
  if (d && d->combine != PGM_COMBINE_COPY && !B) return pgmi_failf(PGM_EINVAL, "batch_add_contract: null B");
  ContractLaunch L;
  int rc = plan_contract(d, L);
  if (rc != PGM_OK) return rc;
  if (L.empty) return PGM_OK;
  BatchJob J;
  memset(&J, 0, sizeof J);
  J.kind = 0;
  J.cmb = d->combine;
  J.red = d->reduce;
  J.A = A;
  J.B = B;
  J.C = C;
  J.c = L.k;
  // flat mode, no split: lanes per output grow while the job is small and the reduction long
  ContractK &k = J.c;
  k.row_mode = 0;
  k.n_split = 1;
  k.red_chunk = k.n_ro;
  // (a single-workgroup levelled batch runs its blocks one after another: spread a job over at most
  // one block's lanes there)
  const uint64_t lanes_cap = h->mode == PGM_BATCH_ONE_WORKGROUP ? 256 : kBatchLanesCap;
  const int g = d->reduce != PGM_RED_NONE && (uint64_t)k.n_ro * k.ri_card > 1 ? lanes_log2(k.n_out, lanes_cap, k.ri_card) : 0;
  k.g_log2 = g;
  const uint64_t cap = k.n_red <= 1 ? kBatchMaxBlocksProduct : 0;
  // output pairs with 16-B accesses when one lane per output is the choice anyway
  if (g == 0 && contract_pairs_ok(k, d->combine, A, B, C)) {
    k.row_mode = 2;
    return batch_append(h, J, (uint64_t)k.n_out / 2, cap);
  }
  return batch_append(h, J, (uint64_t)k.n_out << g, cap);
}

int pgm_batch_add_gather(void *handle, const pgm_gather_desc *d, const double *A, const uint8_t *codes, double *C,
                         int32_t *err_flag) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h || !d || !A || !C) return pgmi_failf(PGM_EINVAL, "batch_add_gather: null argument");
  if (d->n_ev > 0 && !codes) return pgmi_failf(PGM_EINVAL, "batch_add_gather: null codes");
  BatchJob J;
  memset(&J, 0, sizeof J);
  int rc = plan_gather(d, J.g);
  if (rc != PGM_OK) return rc;
  if (J.g.n_out == 0) return PGM_OK;
  J.kind = 1;
  J.A = A;
  J.C = C;
  J.codes = codes;
  J.err = err_flag;
  return batch_append(h, J, J.g.n_out);
}

int pgm_batch_add_product_n(void *handle, const pgm_productn_desc *d, const double *const *ops, double *C) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h || !C) return pgmi_failf(PGM_EINVAL, "batch_add_product_n: null argument");
  BatchJob J;
  memset(&J, 0, sizeof J);
  int rc = plan_prodn(d, ops, J.pn);
  if (rc != PGM_OK) return rc;
  if (J.pn.n_out == 0) return PGM_OK;
  J.kind = 2;
  J.C = C;
  ProdNK &k = J.pn;
  k.pairs = prodn_pairs_ok(k, C) ? 1u : 0u;
  return batch_append(h, J, k.pairs ? k.n_out / 2 : k.n_out);
}

int pgm_batch_add_contract_n(void *handle, const pgm_contractn_desc *d, const double *const *ops, double *C) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h || !C) return pgmi_failf(PGM_EINVAL, "batch_add_contract_n: null argument");
  ContractNK k;
  int rc = plan_contract_n(d, ops, k);
  if (rc != PGM_OK) return rc;
  if (k.n_out == 0) return PGM_OK;
  BatchJob J;
  memset(&J, 0, sizeof J);
  J.kind = 4;
  J.red = k.red;
  J.C = C;
  J._pad = (int32_t)h->njobs.size();
  rc = batch_append(h, J, contract_n_threads(k), contract_n_cap(k));
  if (rc != PGM_OK) return rc;
  h->njobs.push_back(k);
  h->nops.emplace_back(ops, ops + k.n_ops);
  return PGM_OK;
}

int pgm_batch_add_indicator(void *handle, const uint8_t *codes, int64_t n_rows, int64_t card, double *out,
                            int64_t s_state, int64_t s_row, int32_t *err_flag) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h || !codes || !out) return pgmi_failf(PGM_EINVAL, "batch_add_indicator: null argument");
  if (n_rows <= 0 || card <= 0) return PGM_OK;
  BatchJob J;
  memset(&J, 0, sizeof J);
  J.kind = 3;
  J.codes = codes;
  J.C = out;
  J.err = err_flag;
  J.ind_rows = n_rows;
  J.ind_card = card;
  J.ind_s_state = s_state;
  J.ind_s_row = s_row;
  return batch_append(h, J, (uint64_t)(n_rows * card));
}

int pgm_batch_set_mode(void *handle, int32_t mode) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h) return pgmi_failf(PGM_EINVAL, "batch_set_mode: null handle");
  if (h->d_jobs || !h->jobs.empty()) return pgmi_failf(PGM_EINVAL, "batch_set_mode: set before the first job");
  if (mode != PGM_BATCH_GRID && mode != PGM_BATCH_ONE_WORKGROUP) return pgmi_failf(PGM_EINVAL, "batch_set_mode: mode %d", mode);
  h->mode = mode;
  return PGM_OK;
}

int pgm_batch_blocks(void *handle, int64_t *blocks) {
  BatchHandle *h = (BatchHandle *)handle;
  if (!h || !blocks) return pgmi_failf(PGM_EINVAL, "batch_blocks: null argument");
  *blocks = (int64_t)h->block_job.size();
  return PGM_OK;
}

int pgm_batch_add_level(void *handle) {
  STALE_PROBE();
  BatchHandle *h = (BatchHandle *)handle;
  if (!h) return pgmi_failf(PGM_EINVAL, "batch_add_level: null handle");
  if (h->d_jobs) return pgmi_failf(PGM_EINVAL, "batch_add_level: already finalized");
  if (h->mode != PGM_BATCH_ONE_WORKGROUP) return pgmi_failf(PGM_EINVAL, "batch_add_level: levels need PGM_BATCH_ONE_WORKGROUP");
  if (h->block_job.size() > h->level_off.back()) h->level_off.push_back((uint32_t)h->block_job.size());
  return PGM_OK;
}

}  // extern "C"

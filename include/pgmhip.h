/*
 * pgmhip.h — C-ABI of the MI355X (gfx950) discrete-factor engine.
 *
 * Plain C types only (pointers, sizes, fixed-layout structs); no torch and no
 * HIP types cross this boundary (streams travel as opaque `void*`).  Every
 * entry point returns an int status: PGM_OK (0) or a negative PGM_E* code; the
 * thread-local message of the last failure is read with pgm_last_error().  No
 * C++ exception crosses the ABI.  The Python binding is ctypes
 * (pgmpy_amd/_native.py); INTEGRATION.md shows the stub a pgmpy maintainer adds
 * to pgmpy/utils/compat_fns.py to bind it.
 *
 * The reference (pgmpy 1.0.0, /root/reference) is pure Python: every entry
 * point below replaces a numpy / opt_einsum call site, cited per function.
 *
 * Data layout: factor values are fp64 (pgmpy/global_vars.py:38 DTYPE
 * "float64") addressed through per-dimension element strides, so a C-order
 * DiscreteFactor (pgmpy/factors/discrete/DiscreteFactor.py:122, last variable
 * fastest), a broadcast operand (stride 0), a transposed view, and a batch of
 * evidence rows (one extra loop dimension, "batch-innermost" stride 1) are all
 * the same descriptor.  Evidence is column-major uint8 state codes
 * codes[col * ld + row] (code 255 = not observed).
 */
#ifndef PGMHIP_H
#define PGMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (Python maps them to the exception pgmpy raises for the same misuse) */
#define PGM_OK 0
#define PGM_EINVAL (-1)  /* ValueError  */
#define PGM_EINDEX (-2)  /* IndexError  (state code >= cardinality)      */
#define PGM_ENOMEM (-3)  /* MemoryError */
#define PGM_EDEVICE (-4) /* RuntimeError: HIP runtime failure / no device */

#define PGM_MAX_DIMS 32     /* loop dims accepted per side before coalescing */
#define PGM_EV_MISSING 255  /* evidence code meaning "not observed" */

/* ---------------------------------------------------------------- runtime */
int pgm_version(void);                         /* ABI version (PGM_OK-free: returns the number) */
int pgm_last_error(char *buf, size_t len);     /* copies the thread-local message */
int pgm_device_count(int *n);
int pgm_set_device(int device);
int pgm_alloc(void **ptr, size_t bytes);
int pgm_free(void *ptr);
int pgm_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int pgm_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);  /* synchronises the stream */
/* stream-ordered D2H without the synchronize (graph-capturable; dst pinned host memory) */
int pgm_memcpy_d2h_async(void *dst, const void *src, size_t bytes, void *stream);
int pgm_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
int pgm_memset(void *dst, int value, size_t bytes, void *stream);
/* host memory that kernels read and write directly (pinned, mapped, coherent / fine-grained; zeroed):
 * a single query's evidence codes and result, so its captured graph needs no copy nodes */
int pgm_host_alloc(void **ptr, size_t bytes);
int pgm_host_free(void *ptr);
int pgm_stream_sync(void *stream);
/* the same wait by polling (no blocking wait's wake-up latency; a host core spins meanwhile): the single
 * query path (VariableElimination.query, ExactInference.py:246-440) waits for its one graph launch this way */
int pgm_stream_sync_spin(void *stream);
/* HIP events, for timing a kernel on the stream it runs on (bench.py) */
int pgm_event_create(void **ev);
int pgm_event_destroy(void *ev);
int pgm_event_record(void *ev, void *stream);
int pgm_event_elapsed_ms(void *start, void *stop, float *ms);

/* ---------------------------------------------------------------- contract
 * The one generic kernel behind DiscreteFactor.product / sum / divide /
 * marginalize / maximize / normalize and every pairwise step of the
 * sum-product contraction:
 *
 *   C[keep] = REDUCE_{red} COMBINE(A[keep, red], B[keep, red])
 *
 * keep dims are the output loop (outermost first; C is written at keep_sc
 * strides), red dims are summed (PGM_RED_SUM) or max-ed (PGM_RED_MAX) away.
 * Replaces:
 *   product      np.einsum(A, ia, B, ib, union)    DiscreteFactor.py:771-777
 *   marginalize  np.einsum(A, range(n), keep)      DiscreteFactor.py:408
 *   maximize     np.max(A, axis)                   DiscreteFactor.py:480 (compat_fns.py:53-60)
 *   sum          A + B (broadcast)                 DiscreteFactor.py:712
 *   divide       A / B, NaN -> 0                   DiscreteFactor.py:859-863
 *   normalize    A / A.sum()                       DiscreteFactor.py:530 (two calls: SUM, then DIV_RAW)
 *   one pairwise tensordot/einsum step of opt_einsum.contract(..., "greedy")
 *                                                  ExactInference.py:404-406, factors/base.py:106
 */
enum pgm_combine {
  PGM_COMBINE_MUL = 0,     /* A*B                                   */
  PGM_COMBINE_ADD = 1,     /* A+B                                   */
  PGM_COMBINE_DIV = 2,     /* A/B with NaN -> 0 (factor division)   */
  PGM_COMBINE_COPY = 3,    /* A (B unused)                          */
  PGM_COMBINE_DIV_RAW = 4  /* A/B, IEEE (0/0 = NaN, as normalize)   */
};
enum pgm_reduce { PGM_RED_NONE = 0, PGM_RED_SUM = 1, PGM_RED_MAX = 2 };

typedef struct {
  int32_t combine; /* enum pgm_combine */
  int32_t reduce;  /* enum pgm_reduce  */
  int32_t n_keep;
  int32_t n_red;
  int64_t keep_card[PGM_MAX_DIMS];
  int64_t keep_sa[PGM_MAX_DIMS];
  int64_t keep_sb[PGM_MAX_DIMS];
  int64_t keep_sc[PGM_MAX_DIMS];
  int64_t red_card[PGM_MAX_DIMS];
  int64_t red_sa[PGM_MAX_DIMS];
  int64_t red_sb[PGM_MAX_DIMS];
} pgm_contract_desc;

/* bytes of device workspace pgm_contract needs for this descriptor (0 = none) */
int pgm_contract_workspace(const pgm_contract_desc *d, size_t *bytes);
int pgm_contract(const pgm_contract_desc *d, const double *A, const double *B, double *C,
                 void *workspace, size_t workspace_bytes, void *stream);

/* Which kernel pgm_contract would launch for this descriptor and these operand addresses, and with which
 * plan.  Host-only (no HIP call, no device needed; A and C are only compared for 16-B alignment, which
 * decides PGM_CK_ROWS_TAB2; NULL counts as aligned).  The launcher takes its choice from the
 * same function, so what is reported is what runs.  For tests and inspection. */
enum pgm_contract_kernel {
  PGM_CK_FLAT = 0,     /* k_contract: G = 2^g_log2 lanes per output, grid (blocks, n_split)          */
  PGM_CK_ROWS = 1,     /* k_contract_rows: innermost kept dim across lanes, grid (x, outer, n_split) */
  PGM_CK_ROWS_TAB = 2, /* k_contract_rows_tab: <= 512 reduction offsets from an LDS table, no split  */
  PGM_CK_ROWS_TAB2 = 3 /* k_contract_rows_tab2: the same for COPY, two rows per lane (16-B accesses) */
};
typedef struct {
  int32_t kernel;        /* enum pgm_contract_kernel */
  int32_t g_log2;        /* flat: log2 of the lanes per output */
  uint32_t n_split;      /* > 1: partial results in the workspace, then k_contract_final */
  uint32_t red_chunk;    /* reduction-outer (flat: of n_ro, rows: of n_v) indices per split */
  uint32_t ri_nb;        /* rows: chunks the innermost reduction dim is cut into */
  uint32_t ri_chunk;     /* rows: innermost reduction entries per chunk */
  uint32_t grid[3];      /* of the contraction kernel as launched */
  uint32_t n_ro;         /* reduction-outer indices */
  uint32_t n_v;          /* rows: n_ro * ri_nb (0 in flat mode) */
  uint32_t n_out;        /* outputs */
  uint32_t n_red;        /* reduction entries per output */
  uint32_t ri_card;      /* innermost reduction extent after coalescing */
  uint32_t nx;           /* innermost kept extent after coalescing (rows: the dim across the lanes) */
  uint32_t unrolled;     /* rows without a reduction: 1 when the 4-wide loop is entered (NX > 3 * grid.x * 256) */
  uint32_t empty_splits; /* splits whose range starts past the last reduction-outer index (they write the identity) */
} pgm_contract_info_t;
int pgm_contract_info(const pgm_contract_desc *d, const double *A, const double *C, pgm_contract_info_t *info);

/* ---------------------------------------------------------------- n-ary product
 * C[keep] = prod_i X_i[keep . keep_s[i]]  (up to PGM_PRODN_MAX_OPS broadcast operands).
 * factor_product's left fold of __mul__ (pgmpy/factors/base.py:20-66) in one pass, and the
 * batched-BP clique update beta = psi x findings x prod(child messages) written once instead of
 * once per incoming message (ExactInference.py:798-802).  ops is a HOST array of device pointers.
 */
#define PGM_PRODN_MAX_OPS 8
enum pgm_prodn_kind {
  PGM_PRODN_MUL = 0,   /* prod *= X_i                                                    */
  PGM_PRODN_RATIO = 1, /* prod *= X_i / X_{i+1}, NaN -> 0 (sepset update sigma / mu,     */
  PGM_PRODN_DEN = 2,   /*   ExactInference.py:798-802 + DiscreteFactor.py:859-863)       */
  PGM_PRODN_MDIV = 3   /* pgm_product_n_marginal only: prod *= X_i like MUL, and the marginal M is
                          stored divided by X_i (0/0 -> 0) — X_i must not vary over the entries M sums
                          (a child's message mu on its separator: M = sigma' / mu, the child's update
                          ratio, ExactInference.py:798-802).  At most one per call; other calls:
                          PGM_EINVAL */
};
typedef struct {
  int32_t n_ops;
  int32_t n_keep;
  int32_t op_kind[PGM_PRODN_MAX_OPS];
  int64_t keep_card[PGM_MAX_DIMS];
  int64_t keep_sc[PGM_MAX_DIMS];
  int64_t keep_s[PGM_PRODN_MAX_OPS][PGM_MAX_DIMS];
} pgm_productn_desc;

int pgm_product_n(const pgm_productn_desc *d, const double *const *ops, double *C, void *stream);

/* r06: an n-ary contraction, C[keep] = REDUCE over red of prod_t X_t[keep . keep_s[t] + red . red_s[t]]
 * (up to PGM_PRODN_MAX_OPS operands, reduce PGM_RED_SUM or PGM_RED_MAX), as a JOB of a batch only
 * (pgm_batch_add_contract_n): several consecutive pairwise steps of a contraction path
 * (ExactInference.py:404-406, opt_einsum's pairwise tensordots) in one job of one launch, so the
 * compiled path has fewer dependency levels.  A batch holding one runs only as its specialised kernel
 * (pgm_batch_specialise); pgm_batch_run refuses it (PGM_EINVAL).  Products are rounded before they are
 * summed, operands multiplied in order (a left fold, as factor_product). */
typedef struct {
  int32_t n_ops;
  int32_t reduce;
  int32_t n_keep;
  int32_t n_red;
  int64_t keep_card[PGM_MAX_DIMS];
  int64_t keep_sc[PGM_MAX_DIMS];
  int64_t keep_s[PGM_PRODN_MAX_OPS][PGM_MAX_DIMS];
  int64_t red_card[PGM_MAX_DIMS];
  int64_t red_s[PGM_PRODN_MAX_OPS][PGM_MAX_DIMS];
} pgm_contractn_desc;

/* The same product and, in the same pass, M = reduce(C) over the keep dims with marg_s == 0
 * (marg_s[i]: stride of keep dim i in M; the last keep dim, the evidence rows, must have stride 1
 * in C and M).  Batched-BP collect (a clique belief and its message to the parent,
 * ExactInference.py:784-802) and distribute (beta_c *= sigma'/mu in place, C may alias operand 0,
 * with the marginal onto a child separator) read each clique once.  reduce: PGM_RED_SUM or
 * PGM_RED_MAX (max-calibration).  Only shapes with pgm_product_n_marginal_ok() == 1 run fused
 * (<= 4 operands, rows innermost with an even count >= 64, <= 512 reduced states per kept state,
 * enough kept states to fill the chip); others return PGM_EINVAL without launching and the caller
 * runs pgm_product_n + pgm_contract.  C == NULL computes M alone (the strides of C still describe
 * the product's index space): a batched-BP collect message without writing the clique belief, which
 * the distribute pass then writes once. */
int pgm_product_n_marginal_ok(const pgm_productn_desc *d, const double *const *ops, const double *C,
                              const int64_t *marg_s, const double *M);
int pgm_product_n_marginal(const pgm_productn_desc *d, const double *const *ops, double *C,
                           const int64_t *marg_s, int32_t reduce, double *M, void *stream);

/* The same fused step bound to its pointers with the plan compiled in (hipRTC, gfx950): kept /
 * reduced index spaces, strides and operand kinds as literals, the reduced entries as unrolled loops.
 * *bound = NULL (PGM_OK) when the generic kernel should run instead (clique below the size threshold,
 * or PGM_PM_JIT=0 / PGM_NO_JIT set, or the compile failed); the same shape errors as
 * pgm_product_n_marginal otherwise.  pgm_pm_bound_run launches it on stream (capturable in a
 * graph); the pointers must stay valid until pgm_pm_bound_destroy.  Replaces the per-step
 * DiscreteFactor.product / marginalize pair of a batched calibration (ExactInference.py:784-802). */
int pgm_product_n_marginal_bind(const pgm_productn_desc *d, const double *const *ops, double *C,
                                const int64_t *marg_s, int32_t reduce, double *M, void **bound);
/* pgm_product_n as a bound specialised step (no marginal; every dim kept), mergeable with the other
 * bound steps of its level (pgm_pm_merge); *bound = NULL when the shape is not one the fused
 * kernel handles (rows innermost, even, >= 64) or is too small. */
int pgm_product_n_bind(const pgm_productn_desc *d, const double *const *ops, double *C, void **bound);

/* Two marginals of the same product in ONE pass (nothing else stored), as a bound specialised step
 * (mergeable): M1 over the keep dims with marg_s1 != 0, M2 likewise with marg_s2 (rows last, stride 1
 * in both).  A batched-BP parent's sigma' onto two child scopes from its operands
 * (ExactInference.py:784-797: each sigma is a marginalize of the same belief).  *bound = NULL when
 * the shapes are outside the pass's limits (<= 32 accumulators, <= 512 unrolled states); then run two
 * marginal passes. */
int pgm_product_n_marginals_bind(const pgm_productn_desc *d, const double *const *ops, const int64_t *marg_s1,
                                 double *M1, const int64_t *marg_s2, double *M2, int32_t reduce, void **bound);

/* The generated kernel source for the same arguments (no compile, no GPU): returns its length (0
 * when the generic kernel would run), copies at most len-1 bytes + NUL into buf.  Inspection and
 * host-side tests. */
int pgm_product_n_marginal_source(const pgm_productn_desc *d, const double *const *ops, double *C,
                                  const int64_t *marg_s, int32_t reduce, double *M, char *buf, size_t len);
/* Compile (hipRTC, distinct sources, optionally on parallel threads, code-object disk cache) and load the kernels
 * of bound / merged steps that are not loaded yet; a bound step not prepared compiles at its first
 * run.  Call before graph capture. */
int pgm_pm_prepare(void *const *bounds, int32_t n);
/* The generated source of a bound / merged step (its length; at most len-1 bytes + NUL copied). */
int pgm_pm_bound_source(void *bound, char *buf, size_t len);
int pgm_pm_bound_run(void *bound, void *stream);
/* Several bound steps with no dependence between them (one level of a batched-BP sweep) as ONE
 * launch: a kernel whose block ranges run the steps' bodies.  *merged = NULL (PGM_OK) when the merge
 * is not possible (grid too large, compile failed): launch the steps separately.  The inputs stay
 * valid and owned by the caller; destroy the merged handle with pgm_pm_bound_destroy. */
int pgm_pm_merge(void *const *bounds, int32_t n, void **merged);
int pgm_pm_bound_destroy(void *bound);

/* ---------------------------------------------------------------- dense pairwise step (FP64 MFMA)
 * C[b, m, n] = sum_k A[b, m, k] * B[b, k, n] where each index is a GROUP of variables laid out in
 * any order inside its tensor: the element offsets come from a DEVICE int64 table,
 *   offsets = [A_b (batch) | B_b (batch) | C_b (batch) | A_m (m) | C_m (m) | A_k (k) | B_k (k) |
 *              B_n (n) | C_n (n)]
 * so A is read at A[A_b[b] + A_m[m] + A_k[k]] and C written at C[C_b[b] + C_m[m] + C_n[n]].
 * These are the greedy contraction's pairwise steps that are genuine GEMMs — the two factors
 * share summed-out variables (k), each keeps its own (m, n), shared kept variables batch (b) —
 * as in the tensordot/BLAS calls opt_einsum makes for opt_einsum.contract(..., "greedy")
 * (pgmpy/inference/ExactInference.py:404-406, pgmpy/factors/base.py:106).  Exact fp64 products
 * (v_mfma_f64_16x16x4_f64); the k-summation order differs from a sequential loop.
 */
typedef struct {
  int64_t batch, m, n, k;
  const int64_t *offsets; /* device, 3*batch + 2*m + 2*k + 2*n entries */
  int64_t stride[9];      /* per table part: >= 0 -> offset = index * stride (table not read), -1 -> table */
  int32_t lane_order;     /* hint for table groups: bit 0 = consecutive m are adjacent in A, bit 1 = consecutive
                             k are adjacent in B (tile loads then run along that axis); strided groups are
                             detected from the strides */
  int32_t _pad;
} pgm_gemm_desc;

int pgm_gemm(const pgm_gemm_desc *d, const double *A, const double *B, double *C, void *stream);

/* Evidence ingestion: per-column int8 category indices raw[col * ld_raw + row]
 * (pandas Categorical codes / Arrow dictionary indices, -1 = NaN) -> uint8 state codes
 * out[col * ld_out + row] through a per-column LUT lut[col * lut_stride + category] (254 marks a
 * category that is not a state name: err_flag is set), 255 for NaN.  When row_key is given (zeroed
 * by the caller, with row_nmiss), row_key[row] ^= col_key[col] and row_nmiss[row] += 1 for every
 * missing column: the row's evidence-pattern key, from which predict() groups rows.  When row_hash
 * is given (zeroed, 2 x uint64 per row) it receives a 128-bit hash of the row's codes (predict's
 * de-duplication of identical rows, DiscreteBayesianNetwork.py:867-870).  Replaces the
 * per-cell state-name lookups of the reference (state_name.py:71-84 via DiscreteFactor.py:589-597,
 * called per row from DiscreteBayesianNetwork.py:871-878 / :974-979). */
int pgm_codes_remap(const int8_t *raw, int64_t ld_raw, int32_t n_cols, int64_t n_rows, const uint8_t *lut,
                    int32_t lut_stride, const uint64_t *col_key, uint8_t *out, int64_t ld_out, uint64_t *row_key,
                    uint32_t *row_nmiss, uint64_t *row_hash, int32_t *err_flag, void *stream);

/* predict(stochastic=True): for each output row r, numpy's Generator.choice over the joint column
 * joint[i * ld + group[r]] (i < P): cdf = cumsum(p); cdf /= cdf[-1]; out_idx[r] = searchsorted(cdf,
 * u[r], "right") (DiscreteFactor.sample, DiscreteFactor.py:868-912, called per unique evidence row at
 * DiscreteBayesianNetwork.py:889-892).  u: the uniforms of the reference's seeded stream. */
int pgm_sample_joint(const double *joint, int64_t ld, int64_t P, const int32_t *group, const double *u, int64_t n,
                     int32_t *out_idx, void *stream);

/* ---------------------------------------------------------------- evidence column select
 * out[j * n_rows + r] = codes[cols[j] * ld + row0 + r]: copies the evidence columns a compiled
 * plan reads into its own fixed buffer (so the captured graph never sees caller pointers).
 * cols is a DEVICE int32 array of n_cols column indices. */
int pgm_codes_select(const uint8_t *codes, int64_t ld, int64_t row0, const int32_t *cols, int32_t n_cols,
                     int64_t n_rows, uint8_t *out, void *stream);

/* ---------------------------------------------------------------- HIP graphs
 * Capture every launch issued on `stream` between begin and end into an executable graph, then
 * replay it with one launch (compiled BP schedules, fixed-shape contraction plans).  The stream
 * must not be the legacy default stream. */
int pgm_graph_capture_begin(void *stream);
int pgm_graph_capture_end(void *stream, void **graph_exec);
int pgm_graph_launch(void *graph_exec, void *stream);
int pgm_graph_destroy(void *graph_exec);

/* ---------------------------------------------------------------- evidence gather
 * Batched DiscreteFactor.reduce: one evidence row per value of the batch
 * loop dim; the reduced variables' states come from the per-row codes.
 *   C[keep] = A[keep_sa . keep + sum_j codes[ev_col[j]*ld + row] * ev_stride[j]]
 * Replaces basic indexing values[tuple(slice_)] (DiscreteFactor.py:614;
 * the greedy path's per-factor slice ExactInference.py:352-365,385).
 * A code >= ev_card[j] sets *err_flag (-> IndexError, test_Factor.py:555-565);
 * PGM_EV_MISSING is rejected the same way (the plan must not gather it).
 */
typedef struct {
  int32_t n_keep;
  int32_t n_ev;
  int32_t batch_dim; /* index into keep dims that enumerates rows (-1: row 0 only) */
  int32_t _pad;
  int64_t ld;        /* leading dimension of codes (rows per column) */
  int64_t row0;      /* first row of this call (sharding offset) */
  int64_t keep_card[PGM_MAX_DIMS];
  int64_t keep_sa[PGM_MAX_DIMS];
  int64_t keep_sc[PGM_MAX_DIMS];
  int64_t ev_col[PGM_MAX_DIMS];
  int64_t ev_stride[PGM_MAX_DIMS];
  int64_t ev_card[PGM_MAX_DIMS];
} pgm_gather_desc;

int pgm_gather(const pgm_gather_desc *d, const double *A, const uint8_t *codes, double *C,
               int32_t *err_flag, void *stream);

/* 0/1 evidence indicator (BP findings):
 * out[k*s_state + r*s_row] = (codes[r] == k) or 1 when codes[r] == PGM_EV_MISSING */
int pgm_indicator(const uint8_t *codes, int64_t n_rows, int64_t card, double *out, int64_t s_state,
                  int64_t s_row, int32_t *err_flag, void *stream);

/* ---------------------------------------------------------------- argmax
 * First-flat-index argmax per row (np.argmax semantics incl. NaN-first):
 * replaces compat_fns.argmax (compat_fns.py:70-74) in map_query
 * (ExactInference.py:616).  idx[r] = argmax_i X[r*s_row + i*s_elem], written to
 * out_idx (int64) and/or out_idx32 (int32); either may be NULL. */
int pgm_argmax(const double *X, int64_t n_rows, int64_t row_len, int64_t s_row, int64_t s_elem,
               int64_t *out_idx, int32_t *out_idx32, void *stream);

/* ---------------------------------------------------------------- batched small jobs
 * Many INDEPENDENT small contractions / evidence gathers run as one launch (one level of a
 * compiled greedy contraction path, ExactInference.py:404-406: every step whose inputs are ready;
 * or all of a plan's per-factor evidence slices, ExactInference.py:352-365).  Jobs are planned on
 * add (same descriptors and checks as pgm_contract / pgm_gather; contractions run in flat mode
 * without split-K), uploaded once by finalize, and replayed by run (graph-capturable).  The
 * caller guarantees that no job reads another job's output. */
int pgm_batch_create(void **handle);
int pgm_batch_add_contract(void *handle, const pgm_contract_desc *d, const double *A, const double *B, double *C);
int pgm_batch_add_gather(void *handle, const pgm_gather_desc *d, const double *A, const uint8_t *codes, double *C,
                         int32_t *err_flag);
/* an n-ary product job (pgm_product_n's descriptor and checks; flat mode): batched BP runs every
 * small clique / separator product of one dependency level of the calibration as one launch */
int pgm_batch_add_product_n(void *handle, const pgm_productn_desc *d, const double *const *ops, double *C);
/* r06: an n-ary contraction job (pgm_contractn_desc; ops: a HOST array of n_ops device pointers). */
int pgm_batch_add_contract_n(void *batch, const pgm_contractn_desc *d, const double *const *ops, double *C);
/* What pgm_batch_add_contract_n plans for this descriptor, without adding a job: the kept / reduced dims
 * after unit dims are dropped and adjacent dims merged, the lanes per output, and the 256-thread blocks the
 * job takes in a PGM_BATCH_GRID batch.  Host-only (no HIP call, no device needed; ops is not read and may
 * be NULL: the plan depends on cardinalities and strides alone).  The batch entry point plans with the same
 * function, so what is reported is what runs.  An empty output reports n_out = 0 and blocks = 0. */
typedef struct {
  int32_t nk, nr;                /* kept / reduced dims after merging (at most 12 each) */
  int32_t g_log2;                /* log2 of the lanes per output */
  uint32_t blocks;               /* 256-thread blocks of the job in a grid batch */
  uint32_t n_out, n_red;         /* outputs, reduction entries per output */
  uint32_t kcard[PGM_MAX_DIMS];  /* merged kept extents, the last fastest */
  uint32_t rcard[PGM_MAX_DIMS];  /* merged reduced extents */
} pgm_contractn_info_t;
int pgm_contract_n_info(const pgm_contractn_desc *d, const double *const *ops, pgm_contractn_info_t *info);
/* a findings-indicator job (pgm_indicator's arguments): all of a BP sweep's findings in one launch */
int pgm_batch_add_indicator(void *handle, const uint8_t *codes, int64_t n_rows, int64_t card, double *out,
                            int64_t s_state, int64_t s_row, int32_t *err_flag);
/* Single-workgroup levelled batch (mode PGM_BATCH_ONE_WORKGROUP, set before the first job): jobs added
 * after pgm_batch_add_level belong to the next level and may read earlier levels' outputs.  run
 * launches ONE 1,024-thread workgroup that stages every job descriptor, the block map and the level
 * table in LDS and executes each level's blocks (four 256-thread virtual blocks at a time) with a
 * workgroup barrier between levels (no grid barrier, no cache maintenance: producer and consumer are
 * the same workgroup) — for chains of tiny dependent levels (the last levels of a contraction path
 * down to the query marginal and its normalisation, ExactInference.py:404-421), whose
 * one-launch-per-level cost is all launch latency.  Contraction jobs only, tables <= 48 KB
 * (finalize: PGM_EINVAL otherwise).  pgm_batch_add_level needs this mode (PGM_EINVAL in the default
 * PGM_BATCH_GRID mode: one level, one launch).  ABI 20 removed the persistent grid-barrier form
 * (measured slower than one launch per level, r03) and pgm_batch_info. */
int pgm_batch_add_level(void *handle);
enum { PGM_BATCH_GRID = 0, PGM_BATCH_ONE_WORKGROUP = 1 };
int pgm_batch_set_mode(void *handle, int32_t mode);
/* blocks (256-thread workgroups) the jobs added so far occupy; the levelled single-workgroup kernel
 * runs them four at a time, so callers keep it to levels of a few blocks */
int pgm_batch_blocks(void *handle, int64_t *blocks);
int pgm_batch_finalize(void *handle);
int pgm_batch_run(void *handle, void *stream);
/* The finalized batch (contraction jobs only, either mode) as ONE plan-specialised kernel (hipRTC,
 * cached by source like the fused BP steps): each job's output decode, strides, reduction walk and
 * lanes per output are literals and a block finds its job from literal block ranges, so no block map
 * or descriptor is read (C1 / C2's path levels).  *bound = NULL when a job is not a contraction the
 * generator takes (the generic pgm_batch_run stays); else prepare / run / destroy it with
 * pgm_pm_prepare, pgm_pm_bound_run, pgm_pm_bound_destroy (not pgm_pm_merge).  The batch's pointers
 * must stay valid; the batch handle itself may be destroyed.  Up to 512 job pointers travel as the
 * kernel's arguments; a batch of more (up to 8,192) gets its pointer array copied into device memory
 * here and the kernel reads them from that table (freed with the bound launch); *bound = NULL above
 * 8,192 (split the batch). */
int pgm_batch_specialise(void *handle, void **bound);
int pgm_batch_destroy(void *handle);


/* ---------------------------------------------------------------- fused row plan
 * The batched-evidence hot path (DiscreteBayesianNetwork.predict /
 * predict_probability, DiscreteBayesianNetwork.py:731-989; the per-row
 * VariableElimination.query / map_query of ExactInference.py:246-624): per
 * evidence row, the whole reduce -> sum-product -> normalize ->
 * marginalize/argmax chain of one evidence pattern in ONE kernel, one lane per
 * row, CPT values staged in LDS, no HBM intermediates.
 *
 * After evidence reduction the factor graph over the unobserved variables splits
 * into independent COMPONENTS; each is summed over its own (query x hidden)
 * index space, so the joint is never expanded across components.  Loop dims are
 * grouped per component: [comp_loop_begin, +comp_n_query) are query dims,
 * [.., comp_loop_end) hidden (summed) dims.  Factor f (in component c, factors
 * of c are [comp_fac_begin, comp_fac_end)) evaluated at a loop point is
 *   values[fac_base[f] + sum_j code_j(row) * ev_stride_j + sum_k digit_k * fac_stride[f][k]]
 * Outputs follow the reference exactly: marginal = component marginal / its
 * mass; if the product of all component masses is 0 (impossible evidence) every
 * marginal is NaN (0/0 of DiscreteFactor.normalize, DiscreteFactor.py:530) and the
 * MAP index is 0 (np.argmax of an all-NaN joint).
 */
#define PGM_ROWS_MAX_LOOP 12
#define PGM_ROWS_MAX_FAC 16
#define PGM_ROWS_MAX_EV 48
#define PGM_ROWS_MAX_COMP 12
#define PGM_ROWS_MAX_MARG 192

enum pgm_rows_mode {
  PGM_ROWS_MARGINALS = 1, /* per query var normalized marginal (predict_probability) */
  PGM_ROWS_JOINT = 2,     /* normalized joint over the query dims (query joint=True); n_comp == 1 only */
  PGM_ROWS_MAP = 4,       /* first-index argmax of the joint (map_query / predict)  */
  PGM_ROWS_MAPGAP = 8,    /* also (best - second best) / best of the joint, for tie screening */
  PGM_ROWS_VALUES_GLOBAL = 16, /* tuning: read CPT values through L1/L2 instead of staging them in LDS */
  PGM_ROWS_ONE_GROUP = 32,     /* tuning: one 64-row group per workgroup (no staging amortisation) */
  PGM_ROWS_GENERIC = 64,       /* tuning: table-driven kernel even for all-affine plans (testing)  */
  PGM_ROWS_NO_JIT = 128,       /* testing: skip the plan-specialised (hipRTC) kernel, run the AOT ones */
  PGM_ROWS_FLOOR = 256         /* measurement (pgm_rows_plan_bind only): the plan's dispatch floor — same grid,
                                  same evidence-column loads and output stores as the specialised kernel, no
                                  CPT staging or arithmetic; the outputs are NOT results */
};

typedef struct {
  int32_t n_loop;
  int32_t n_query;  /* total query dims */
  int32_t n_fac;
  int32_t n_ev;
  int32_t n_values; /* packed CPT values (doubles) */
  int32_t n_comp;
  int32_t n_marg;   /* rows of the marginal output = sum of query cardinalities */
  int32_t n_joint;  /* entries of the joint = prod of query cardinalities */
  int32_t loop_card[PGM_ROWS_MAX_LOOP];
  int32_t loop_marg_off[PGM_ROWS_MAX_LOOP];   /* query dim: first marginal row of its variable (-1 hidden) */
  int32_t loop_map_stride[PGM_ROWS_MAX_LOOP]; /* query dim: stride in the flat joint / MAP index (0 hidden) */
  int32_t comp_loop_begin[PGM_ROWS_MAX_COMP];
  int32_t comp_n_query[PGM_ROWS_MAX_COMP];
  int32_t comp_loop_end[PGM_ROWS_MAX_COMP];
  int32_t comp_fac_begin[PGM_ROWS_MAX_COMP];
  int32_t comp_fac_end[PGM_ROWS_MAX_COMP];
  int32_t fac_base[PGM_ROWS_MAX_FAC];
  int32_t fac_stride[PGM_ROWS_MAX_FAC][PGM_ROWS_MAX_LOOP];
  int32_t fac_ev_begin[PGM_ROWS_MAX_FAC]; /* evidence terms of factor f: [begin, end) */
  int32_t fac_ev_end[PGM_ROWS_MAX_FAC];
  int32_t ev_col[PGM_ROWS_MAX_EV];
  int32_t ev_stride[PGM_ROWS_MAX_EV];
  int32_t ev_card[PGM_ROWS_MAX_EV];
} pgm_rows_plan;

int pgm_rows_plan_create(const pgm_rows_plan *plan, const double *host_values, void **handle);
int pgm_rows_plan_destroy(void *handle);
/* Source of the plan-specialised row kernel (hipRTC, compiled for gfx950 on the first run of an
 * all-affine plan: one query variable and no hidden variable per component).  Writes at most len
 * bytes (NUL-terminated) and the full size + 1 to *needed.  No device needed (tests, inspection). */
int pgm_rows_plan_source(const pgm_rows_plan *plan, char *buf, size_t len, size_t *needed);
/* The same kernels under the streaming cache policy (evidence codes and outputs pass the caches: a
 * second hipRTC program of the plan, bit-identical outputs), and to *min_rows (may be NULL) the row count
 * from which a launch runs it (INT64_MAX: never).  PGM_ROWS_STREAM, read when a plan is created, overrides
 * both for A/B runs: 0 = default program always; 1..5 = streaming always, nontemporal code loads if bit 0,
 * store form (value >> 1): 0 sc1, 1 sc1 nt, 2 sc0 sc1 nt.  Same buffer contract as pgm_rows_plan_source. */
int pgm_rows_plan_stream_source(const pgm_rows_plan *plan, char *buf, size_t len, size_t *needed, int64_t *min_rows);
/* Rows [row0, row0 + n_rows) of codes.  Outputs are column-major with leading dim ld_out (>= n_rows) and
 * row r written at column r (not row0 + r); any may be NULL unless its mode bit is set:
 *   marg [n_marg][ld_out] f64   joint [n_joint][ld_out] f64   map [n_rows] int32   gap [n_rows] f64 */
int pgm_rows_plan_run(void *handle, int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0,
                      int64_t n_rows, double *marg, double *joint, int64_t ld_out, int32_t *map,
                      double *gap, int32_t *err_flag, void *stream);

/* Which kernel pgm_rows_plan_run would launch for this plan and these launch arguments, and how.
 * Host-only (no HIP call, no device, no handle): the plan is compiled, the arguments are checked as
 * pgm_rows_plan_run checks them (same order, same messages), and the pointers are inspected for NULL
 * and alignment only (the two-rows-per-thread contract of pgm_rows_jit2).  jit_available: whether the
 * plan-specialised (hipRTC) kernel can be had; with 0 the ahead-of-time kernels are chosen, as when
 * hipRTC fails.  pgm_rows_plan_run and pgm_rows_plan_bind take their choice from the same function.
 * n_rows <= 0 launches nothing: kernel PGM_RK_NONE, blocks 0.  For tests and inspection. */
enum pgm_rows_kernel {
  PGM_RK_NONE = -1,
  PGM_RK_JIT = 0,    /* pgm_rows_jit: plan-specialised, one row per thread                       */
  PGM_RK_JIT2 = 1,   /* pgm_rows_jit2: plan-specialised, two rows per thread, 16-B stores        */
  PGM_RK_AFFINE = 2, /* k_rows_affine<values_lds, nf, nt, map>: all-affine plans                 */
  PGM_RK_TABLE = 3   /* k_rows<values_lds, acc_lds, maxfc, maxt>: table-driven components        */
};
typedef struct {
  int32_t kernel;     /* enum pgm_rows_kernel */
  int32_t values_lds; /* CPT values staged in LDS (else read from global memory) */
  int32_t acc_lds;    /* TABLE: marginal accumulators in LDS (else none, or in marg itself) */
  int32_t maxfc;      /* TABLE: factor slots of the instance (2, 4, 8, 16) */
  int32_t maxt;       /* TABLE: evidence terms of the instance (4, 8, 48) */
  int32_t nf;         /* AFFINE: factor slots of the instance (1, 2, 4) */
  int32_t nt;         /* AFFINE: evidence terms of the instance (4, 8) */
  int32_t map;        /* AFFINE: the instance that carries the MAP bookkeeping */
  int32_t rg;         /* 64-row groups per workgroup (1 for the specialised kernels) */
  uint32_t blocks;    /* workgroups */
  uint32_t wg;        /* work-items per workgroup */
  uint32_t lds_bytes; /* AOT: dynamic LDS of the launch; specialised: its static value array */
} pgm_rows_launch_info_t;
int pgm_rows_launch_info(const pgm_rows_plan *plan, int32_t mode, const uint8_t *codes, int64_t ld_codes,
                         int64_t row0, int64_t n_rows, const double *marg, const double *joint, int64_t ld_out,
                         const int32_t *map, const double *gap, int32_t jit_available,
                         pgm_rows_launch_info_t *info);

/* Prepared launch: validates the same arguments as pgm_rows_plan_run once and binds them; each
 * pgm_rows_bound_run then launches that pass (same result as the unbound call).  The buffers and the
 * plan handle must outlive the bound handle.  Replaces the per-batch Python call of predict()'s
 * inner loop (pgmpy/models/DiscreteBayesianNetwork.py:867-910) for repeated batches. */
int pgm_rows_plan_bind(void *handle, int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0,
                       int64_t n_rows, double *marg, double *joint, int64_t ld_out, int32_t *map,
                       double *gap, int32_t *err_flag, void *stream, void **bound);
int pgm_rows_bound_run(void *bound);
int pgm_rows_bound_destroy(void *bound);
/* which kernel a bound launch runs: "pgm_rows_jit" (one row per thread), "pgm_rows_jit2" (two rows
 * per thread, 16-B stores), "pgm_rows_floor" / "pgm_rows_floor2" (PGM_ROWS_FLOOR), or "" (an AOT kernel), with its grid and workgroup size */
int pgm_rows_bound_kernel(void *bound, char *name, size_t cap, uint32_t *blocks, uint32_t *wg);

/* Rows sharded over several GPUs from host buffers: the data-parallel axis of predict /
 * predict_probability (pgmpy/models/DiscreteBayesianNetwork.py:867-910, 912-989) split into n_shards
 * contiguous row blocks (shard i = rows [i n / S, (i + 1) n / S), as pgmpy_amd.distributed.shard_bounds),
 * shard i run by handles[i] on the HIP device that was current when that handle was created
 * (pgm_rows_plan_create once per device; the handles must describe the same plan).  One host thread per
 * shard: the shard's rows of the evidence columns the plan reads in (host_codes column-major uint8 with
 * columns [0, n_cols), leading dim ld_codes, the plan's column numbering), the plan's pass, its outputs
 * out to the caller's host arrays at the shard's columns — the gather of every shard's result is that
 * copy, each GPU's over its own host link.  A shard runs in chunks of 256 K rows (PGM_SHARD_CHUNK)
 * alternating between two streams and device buffers the handle keeps from its first call (no
 * allocation after it), so a chunk's copy-in and pass overlap the previous chunk's copy-out when the host
 * arrays are pinned (pgm_host_alloc); pageable arrays work and are staged by HIP.  One call at a time
 * per handle.  mode: PGM_ROWS_MARGINALS
 * (host_marg [n_marg][ld_out] f64) and / or PGM_ROWS_MAP (host_map [n_rows] int32).  *err_any is ORed
 * with the kernels' evidence-error flag (PGM_ROWS error semantics of pgm_rows_plan_run).  Returns when
 * every shard is done; the first failing shard's status otherwise.  Outputs equal one
 * pgm_rows_plan_run over all rows bit for bit.  (the multi-GPU entry a non-Python
 * FFI caller uses; the Python path shards with torch.distributed, pgmpy_amd/distributed.py.) */
int pgm_rows_shard_run(void *const *handles, int32_t n_shards, int32_t mode, const uint8_t *host_codes,
                       int64_t ld_codes, int64_t n_cols, int64_t n_rows, double *host_marg, int64_t ld_out,
                       int32_t *host_map, int32_t *err_any);

/* Host-side scan for evidence ingestion (no device needed): out[j] = 1 when any of the n int8 cells of
 * column cols[j] is negative (a pandas Categorical NaN code), else 0; up to `threads` host threads.
 * Finds the NaN-holding columns of a categorical frame in one native pass, so rows are grouped by
 * missing-column pattern from those columns only (predict's per-row NaN handling,
 * pgmpy/models/DiscreteBayesianNetwork.py:862-878). */
int pgm_host_any_negative_i8(const int8_t *const *cols, int32_t n_cols, int64_t n, uint8_t *out, int32_t threads);
/* r06 (pgmhost.cpp, one persistent pool of at most 16 host threads): the same scan as a job fed column by
 * column — begin (n rows, room for `capacity` columns), push column pointers as they become known (each
 * push is scanned on the pool while the caller goes on), end (waits, out[j] = 1 when pushed column j holds a
 * negative code; *n_cols = columns pushed; frees the job).  The caller keeps the columns alive until end.
 * pgm_host_lut_map_u8: dst[j * ld + i] = luts[j][(uint8_t)src[j][i]] (luts[j] NULL: the byte itself), on
 * the pool — the plan's evidence columns from category codes to state codes (state_name.py:71-84 per
 * cell in the reference). */
int pgm_host_scan_begin(int64_t n, int32_t capacity, int32_t threads, void **job);
int pgm_host_scan_push(void *job, const int8_t *const *cols, int32_t count);
int pgm_host_scan_end(void *job, uint8_t *out, int32_t *n_cols);
int pgm_host_lut_map_u8(const int8_t *const *src, const uint8_t *const *luts, int32_t n_cols, int64_t n, uint8_t *dst,
                        int64_t ld, int32_t threads);

/* Resident ring of row batches (streaming predict_probability / predict): one launch of the
 * plan-specialised two-rows-per-lane kernel ("pgm_rows_ring") stays resident while the host publishes
 * batches, so consecutive batches overlap on the chip instead of each paying a dispatch.  Replaces the
 * reference's per-batch caller loop (pgmpy/models/DiscreteBayesianNetwork.py:867-910, 912-989) for a
 * stream of equally sized batches.
 *   create: n_slots buffer sets; batch b reads codes[b % n_slots] (rows [row0, row0 + n_rows), leading
 *           dim ld_codes) and writes marg / map / gap[b % n_slots] (leading dim ld_out), as
 *           pgm_rows_plan_run.  mode: PGM_ROWS_MARGINALS | PGM_ROWS_MAP | PGM_ROWS_MAPGAP only; the
 *           two-rows-per-lane contract holds per slot (even n_rows / row0 / leading dims, 16-B aligned
 *           outputs) else PGM_EINVAL.  Needs the plan-specialised kernel (hipRTC).
 *   start:  launches the resident grid on `stream` for n_batches batches (the ring must not be
 *           running); waves that reach a batch not yet posted wait, and give up after timeout_s
 *           seconds (PGM_EDEVICE from finish).
 *   post:   publishes batches [0, n_posted) (monotone, <= n_batches).  A batch's inputs must be
 *           complete in device memory, and its slot's previous batch finished, before it is posted.
 *   finish: all n_batches posted -> waits for the launch (stream synchronize) and checks it.
 *   cancel: stops the launch early (waves exit at their next unposted batch) and waits.
 * Outputs of batch b equal pgm_rows_plan_run's on the same rows bit for bit. */
int pgm_rows_ring_create(void *handle, int32_t mode, int32_t n_slots, const uint8_t *const *codes,
                         const int64_t *ld_codes, const int64_t *row0, int64_t n_rows, double *const *marg,
                         int64_t ld_out, int32_t *const *map, double *const *gap, int32_t *err_flag, void *stream,
                         void **ring);
int pgm_rows_ring_start(void *ring, uint32_t n_batches, double timeout_s);
/* start_ready: start, then wait (up to ready_timeout_s) until every workgroup of the resident grid is
 * running with its CPT staged, so that what follows (posts, completions) no longer includes the launch
 * itself; PGM_EDEVICE (and the launch cancelled) if the grid does not come up in time */
int pgm_rows_ring_start_ready(void *ring, uint32_t n_batches, double timeout_s, double ready_timeout_s);
int pgm_rows_ring_post(void *ring, uint32_t n_posted);
int pgm_rows_ring_finish(void *ring);
int pgm_rows_ring_cancel(void *ring);
/* the ring's batch counter in pinned host memory and this launch's base: storing base + k (a plain,
 * aligned 32-bit store, monotone, k <= n_batches) publishes batches [0, k) exactly as
 * pgm_rows_ring_post(ring, k) does, without a library call per batch (finish then needs
 * pgm_rows_ring_post(ring, n_batches) or the store of base + n_batches) */
int pgm_rows_ring_counter(void *ring, uint32_t **counter, uint32_t *base);
/* the ring's kernel name ("pgm_rows_ring"), resident grid and workgroup size */
int pgm_rows_ring_kernel(void *ring, char *name, size_t cap, uint32_t *blocks, uint32_t *wg);
int pgm_rows_ring_destroy(void *ring);

/* Direct AQL dispatch (pgmpy_amd/csrc/pgmdq.cpp).  A user-mode HSA queue on the GPU agent of a HIP
 * device; a bound launch of the plan-specialised kernel (pgm_rows_plan_bind) is re-bound to it and
 * each pgm_dq_launch writes one kernel-dispatch packet (barrier bit set) and rings the doorbell — no
 * HIP runtime on the launch path.  Same kernel, same arguments, same results as pgm_rows_bound_run.
 * Ordering: pgm_dq_bind_rows waits for the device (inputs complete); dispatches on one queue run in
 * order; inputs may change only between pgm_dq_sync and the next launch (that launch first drains the
 * device with hipDeviceSynchronize, so HIP work issued in between is complete); call
 * pgm_dq_sync (a system-scope release barrier + wait) before HIP work reads the outputs.  The timer reports
 * the GPU span (queue profiling timestamps) from the first dispatch after pgm_dq_timer_start to the
 * last one issued.  The queue must outlive its bound launches.  Serves the same caller as
 * pgm_rows_bound_run (pgmpy/models/DiscreteBayesianNetwork.py:867-910, repeated batches). */
int pgm_dq_create(int hip_device, void **dq);
int pgm_dq_destroy(void *dq);
int pgm_dq_bind_rows(void *dq, void *bound, void **dbound);
int pgm_dq_launch(void *dbound);
/* a group of bound launches on one queue whose outputs are pairwise distinct (independent batches):
 * the first waits for everything before it (barrier bit), the others may overlap it and each other;
 * the next launch or sync waits for the whole group.  At most 128 launches, no launch repeated. */
int pgm_dq_launch_group(void *const *dbounds, int32_t n);
/* one dispatch whose own completion releases at system scope (its packet's release fence): the last
 * dispatch before the host or HIP reads the outputs, instead of a separate pgm_dq_sync barrier packet;
 * wait for it with pgm_dq_wait.  Like pgm_dq_sync, the next dispatch acquires at system scope. */
int pgm_dq_launch_release(void *dbound);
int pgm_dq_sync(void *dq);
/* the first half of pgm_dq_sync: append the system-scope release barrier packet without waiting for
 * it (pgm_dq_wait then waits for it with the dispatches), so several queues release in parallel */
int pgm_dq_release(void *dq);
/* wait until every dispatch issued on the queue has completed (no release barrier: call pgm_dq_sync
 * before HIP work reads the outputs) */
int pgm_dq_wait(void *dq);
int pgm_dq_timer_start(void *dq);
int pgm_dq_timer_stop_ms(void *dq, float *ms);
/* the same span as raw HSA system timestamps (start of the first timed dispatch, latest end) and their
 * frequency, so spans of several queues can be joined */
int pgm_dq_timer_stop_ticks(void *dq, uint64_t *start, uint64_t *end, uint64_t *freq);
/* after a timer stop: the sum of the timed dispatches' own durations (end - start, in the ticks of
 * pgm_dq_timer_stop_ticks) and how many were summed (those still in the 256-signal ring) — the
 * per-launch duration a kernel trace reports, which exceeds span / launches when queues overlap */
int pgm_dq_timer_dispatch_stats(void *dq, uint64_t *sum_ticks, uint64_t *count);
/* r06: after a timer stop, each timed dispatch's own start / end (HSA system ticks, the frequency of
 * pgm_dq_timer_stop_ticks) in issue order, at most cap of them (those still in the signal ring);
 * *count = how many were written.  The raw timestamps behind the C3 line's span-based frac. */
int pgm_dq_timer_dispatch_times(void *dq, uint64_t *start, uint64_t *end, int32_t cap, int32_t *count);
int pgm_dq_bound_destroy(void *dbound);
/* introspection (tests): the kernel object a bound launch dispatches, the device address of its kernarg
 * segment, and how many bound launches currently share its loaded code object.  Bound launches of one
 * code object on one device — whatever their queue — share one loaded executable, so they report the
 * same kernel object for the same kernel; kernarg segments are 256-byte slots of device allocations of
 * at least 64 KiB, reused after pgm_dq_bound_destroy.  Any output pointer may be NULL. */
int pgm_dq_bound_info(void *dbound, uint64_t *kernel_object, uint64_t *kernarg, int32_t *sharers);
/* r05 (ABI 22): a compiled query's steps on the queue (VariableElimination.query through a captured
 * plain Program, pgmpy/inference/ExactInference.py:349-440, C1 / C2).  pgm_dq_bind_pm re-binds one
 * plan-specialised launch (pgm_pm_bound_* handle: a fused product step, a merged level or a specialised
 * contraction batch) to the queue; pgm_dq_run_chain writes the n launches as one dependent chain (each
 * packet's barrier bit set unless independent[i] is 1 — launch i reads nothing launch i-1 writes; the last
 * packet always waits for every earlier one — and
 * agent-scope fences on every packet, the last releasing at system scope — inputs the host writes between
 * chains must be in coherent host memory (pgm_host_alloc), which the kernels read uncached; independent
 * may be NULL), rings the doorbell once and returns when the last has completed — the outputs are then
 * visible to the host.  Contract: no HIP work that writes the chain's inputs may be pending (the chain
 * does not drain the device; the host writes inputs through mapped memory).  At most 128 launches.  All n
 * slots are reserved at once after every check that can fail (no half-written chain is left on the
 * queue).  Refused (PGM_EINVAL) while a pgm_dq_timer span is open on the queue: only the last packet
 * carries a completion signal, so there are no per-dispatch timestamps to report.
 * pgm_dq_profiling turns the queue's dispatch timestamps on or off (pgm_dq_timer_* need them).  Leave it
 * on for a queue a profiler may intercept (r06): a kernel-tracing tool reads every dispatch's timestamps
 * from its own completion signals, which needs the queue's profiling enabled — r05 turned it off on the
 * query queue and rocprofv3 crashed on the chain. */
int pgm_dq_bind_pm(void *dq, void *pm_bound, void **dbound);
int pgm_dq_run_chain(void *const *dbounds, const uint8_t *independent, int32_t n);
int pgm_dq_profiling(void *dq, int32_t on);

/* ---------------------------------------------------------------- parameter learning
 * DiscreteBayesianNetwork.fit / fit_update (DiscreteBayesianNetwork.py:596-729) on the device: the state
 * counts of every family (a node plus its parents) in one launch, then every CPD's values in one more.
 * Replaces the reference's pandas groupby per node (estimators/base.py:67-176) and its per-CPD
 * normalisation (MLE.py:183-212, BayesianEstimator.py:252-264).  An extension of ABI 25.
 *
 * A family lists the code column and the cardinality of the node, then of each parent in the CPD's
 * order (the reference sorts them); at most PGM_MAX_DIMS - 1 parents.  Its count table has the CPD's
 * layout [node_card, prod(parent_card)] in C order (last parent fastest) and sits at offsets[f] of one
 * flat buffer of total_bins entries, families end to end in the order given.
 *
 * pgm_fit_count ADDS to `tables` (the caller zeroes them; several calls may count several row windows)
 * the rows [row0, row0 + n_rows) of codes[col * ld + row] (n_cols columns of ld rows).  A row whose code
 * is PGM_EV_MISSING in any column of a family is skipped for that family only (groupby / value_counts
 * drop NaN per family).  weights NULL: every row counts 1, tables are int64, exact and deterministic.
 * weights given (weights[row], ld entries; the `_weight` column): tables are fp64 and the order of
 * addition is not fixed.  A code that is neither PGM_EV_MISSING nor < its cardinality never indexes a
 * table: the row is skipped for that family and the call returns PGM_EINDEX (a device flag the call
 * reads back after the launch, so the call synchronises the stream).
 *
 * pgm_fit_finish writes values = normalise(counts + pseudo) for every CPD: pseudo (optional, fp64, the
 * tables' layout) is added, then each column is divided by its sum taken in state order
 * (values / values.sum(axis=0)).  PGM_FIT_MLE: a column that is all zero becomes uniform (MLE.py:187).
 * PGM_FIT_BAYES: no fill, 0/0 stays NaN.  | PGM_FIT_WEIGHTED: counts are the fp64 tables.
 *
 * Every argument is checked on the host before any HIP call; pgm_fit_plan_create and pgm_fit_plan_info
 * need no device (the descriptors are uploaded by the first count / finish).
 *
 * Plan handles (pgm_fit_plan_*, pgm_sample_plan_*, pgm_gibbs_plan_*; this section and the five after it).
 * Calls on one plan handle must not overlap, on any streams or threads: the device flag word a call reads
 * back, the staging buffer of its modes / clamp and the chunk partials of a score or CI launch belong to
 * the handle, not to the call.  Distinct plans are independent.  A plan follows the current device: its
 * descriptors are uploaded on first use on the device that is current at the call, and when a later call
 * finds another device current they are released there and uploaded again (what only the score or the CI
 * launches need is allocated by the first such call on that device).  pgm_*_plan_destroy frees all of it
 * and accepts NULL. */
#define PGM_FIT_MLE 0
#define PGM_FIT_BAYES 1
#define PGM_FIT_WEIGHTED 2
typedef struct {
  int32_t n_vars;             /* 1 + parents */
  int32_t col[PGM_MAX_DIMS];  /* code column: the node, then each parent */
  int32_t card[PGM_MAX_DIMS]; /* 1 .. 255 */
} pgm_fit_family;
typedef struct {
  int32_t n_families;
  int32_t n_groups;       /* workgroup groups: consecutive families whose tables share one LDS tile */
  int32_t tile_bins;      /* bins of the LDS tile; a larger family counts straight into global memory */
  int32_t rows_per_block; /* rows one workgroup counts for its group */
  int32_t n_cols;         /* 1 + the largest code column read */
  int32_t block;          /* work-items per workgroup */
  int64_t total_bins;     /* entries of the count / pseudo-count / value buffers */
  int64_t total_columns;  /* CPD columns (parent configurations) over all families */
} pgm_fit_info_t;
int pgm_fit_plan_create(const pgm_fit_family *families, int32_t n_families, void **plan);
int pgm_fit_plan_destroy(void *plan);
/* layout of a plan: per family its offset, its size, its PGM_MAX_DIMS strides (node first) and its group;
 * any output may be NULL */
int pgm_fit_plan_info(void *plan, pgm_fit_info_t *info, int64_t *offsets, int64_t *sizes, int32_t *strides,
                      int32_t *groups);
int pgm_fit_count(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                  const double *weights, void *tables, void *stream);
int pgm_fit_finish(void *plan, const void *counts, const double *pseudo, int32_t mode, double *values, void *stream);

/* ---------------------------------------------------------------- structure scores
 * The data-dependent part of the decomposable structure scores (estimators/StructureScore.py: K2, BDeu,
 * BDs, LogLikeliHood, BIC, AIC) of every family of a fit plan, from the int64 tables pgm_fit_count
 * wrote, without bringing them to the host.  An extension of ABI 25.
 *
 * Family f has r states and q columns (parent configurations); N_jk is the count of state k in column
 * j, N_j = sum_k N_jk.  scores[f] is the sum over the family's columns of the column term
 *   PGM_SCORE_BD   sum_k lgamma(N_jk + beta[f]) - lgamma(N_j + alpha[f])
 *                  | PGM_SCORE_SKIP_EMPTY: a column with N_j = 0 contributes exactly 0
 *   PGM_SCORE_LL   sum_{k: N_jk > 0} N_jk * (log N_jk - log N_j)      (alpha, beta ignored, may be NULL)
 * and n_observed[f] (optional) the number of columns with N_j > 0.  The constants that depend only on
 * (r, q, equivalent sample size) are the caller's.  alpha, beta, scores and n_observed are device
 * arrays with one entry per family.  fp64 (weighted) tables are not accepted.
 *
 * A family's columns are cut into chunks of PGM_SCORE_CHUNK columns counted from its own column 0; one
 * workgroup sums a chunk in a fixed order (a work-item its column's terms in state order, then a
 * fixed-shape tree), a second launch sums each family's chunk partials in a fixed order.  No
 * floating-point atomics: a family's score is bit-identical from run to run and does not depend on
 * which other families share the plan.  The chunk partials live in the plan (plan handles, above).
 * Every argument is checked on the host before any HIP call. */
#define PGM_SCORE_BD 0
#define PGM_SCORE_LL 1
#define PGM_SCORE_SKIP_EMPTY 2
#define PGM_SCORE_CHUNK 128 /* CPD columns per workgroup (two waves): small families waste few lanes */
int pgm_fit_score(void *plan, const int64_t *counts, int32_t mode, const double *alpha, const double *beta,
                  double *scores, int64_t *n_observed, void *stream);
/* n_states[f] (device, one per family) = the number of states k of family f's node with sum_j N_jk > 0.
 * The reference's state_counts(reindex=False) drops the other states' rows from a family with parents
 * (groupby(observed=True)), so its BDeu / BDs leave out their lgamma(beta) terms (StructureScore.py:
 * 463-473): the caller's correction needs their number.  Integer work only; checked on the host. */
int pgm_fit_states_observed(void *plan, const int64_t *counts, int64_t *n_states, void *stream);

/* ---------------------------------------------------------------- conditional-independence tests
 * (an extension of ABI 25.)  The Cressie-Read power-divergence test of X _|_ Y | Z for every family of a
 * fit plan, read as (X, Y, Z1 .. Zk), from the int64 tables pgm_fit_count filled: family f's table is
 * [rx][ry][qz], the Z configuration fastest.  The reference's CITests.power_divergence (CITests.py:445-499)
 * over scipy.stats.chi2_contingency, one pandas groupby and one scipy call per stratum there.
 *
 * Per stratum z with n_z > 0 rows: the rows x and columns y whose marginal R_x, C_y is zero are dropped,
 * dof_z = (rows left - 1)(columns left - 1); a stratum with dof_z = 0 adds nothing.  E_xy = R_x C_y / n_z.
 * With PGM_CI_YATES and dof_z = 1 each observed cell first moves towards its expectation by
 * min(0.5, |E - O|) (chi2_contingency's correction=True).  The stratum's statistic is
 *   lambda = 1    sum (O - E)^2 / E
 *   lambda = 0    2 sum O ln(O / E)            (a cell with O = 0 adds 0)
 *   lambda = -1   2 sum E ln(E / O)            (a cell with O = 0 gives +inf)
 *   otherwise     2 / (lambda (lambda + 1)) sum O ((O / E)^lambda - 1)
 * stat[f] and dof[f] are the sums over the strata and pvalue[f] = Q(dof / 2, stat / 2), the chi-square
 * survival function (csrc/pgm_igamc.h).  dof = 0: pvalue = 1 for a family without Z, NaN with one (the
 * reference's 1 - chi2.cdf(0, 0)); stat = +inf: pvalue = 0.  stat, dof, pvalue: device arrays, one entry
 * per family.  fp64 (weighted) tables are not accepted.
 *
 * A family's strata are cut into chunks of PGM_CI_CHUNK counted from its own stratum 0; a chunk is summed
 * in a fixed order and a second launch adds a family's chunk partials in index order.  No floating-point
 * atomics: a family's three outputs are bit-identical from run to run and do not depend on which other
 * families share the plan.  The chunk partials live in the plan (plan handles, above).  Every argument is
 * checked on the host before any HIP call: PGM_EINVAL for a null
 * plan / counts / stat / dof / pvalue, a non-finite lambda, unknown flag bits, or a family with fewer
 * than two variables. */
#define PGM_CI_YATES 1
#define PGM_CI_CHUNK 128 /* strata per workgroup */
int pgm_fit_citest(void *plan, const int64_t *counts, double lambda, int32_t flags, double *stat, int64_t *dof,
                   double *pvalue, void *stream);

/* ---------------------------------------------------------------- expectation maximisation: the E-step
 * (an extension of ABI 25.)  The expected family counts of a network with latent variables, for the
 * reference's ExpectationMaximization (estimators/EM.py:130-180, 389-397), in one launch: no frame of
 * unique rows x latent configurations, no get_value per CPD and expanded row.  The M-step is
 * pgm_fit_finish | PGM_FIT_WEIGHTED on the tables this call fills.
 *
 * plan is an ordinary fit plan: the families whose CPDs EM updates.  values (device, fp64: the current
 * CPDs) and tables (device, fp64, ADDED to, as pgm_fit_count does) have the plan's flat layout.
 * latent_cols (host, n_latent entries) names the code columns that are latent.  They are virtual: codes
 * is never read for them and n_cols bounds the observed columns only.  A latent's cardinality is the one
 * its families give it.
 *
 * For a row r of the window, with L the product of the latent cardinalities:
 *   p_l = product over the families with a latent in scope of max(values[entry], PGM_EM_FLOOR), the entry
 *         taken from the row's observed codes with the latents set to configuration l   (EM.py:116-126)
 *   Z = sum_l p_l,  w_l = p_l / Z
 *   tables[entry(l)] += w_l for every l, in every family with a latent
 *   tables[entry] += 1.0 in a family without one (its factor is the same for every l and cancels in w,
 *         and sum_l w_l = 1): those tables hold exact integers
 *   loglik[row0 + r] = log Z + sum over the latent-free families of log max(values[entry], PGM_EM_FLOOR)
 *         (loglik: optional, device, fp64, ld entries indexed by buffer row)
 * A row with PGM_EV_MISSING in any observed column of any family of the plan adds nothing to any table and
 * its loglik is 0 (the reference drops such rows, EM.py:93-102).  A row with a code that is neither
 * missing nor a state adds nothing either and the call returns PGM_EINDEX, through the device flag of
 * pgm_fit_count (so the call synchronises the stream).
 *
 * At most PGM_EM_MAX_FAMILIES clamped factors make p_l >= 1e-320, above fp64's smallest denormal: Z > 0
 * for every row and no row needs a rule of its own; below about 1e-290 p_l is denormal and the weights lose
 * precision.  The tables are added with fp64 atomics in no fixed order: nothing is bit-identical from run
 * to run.
 *
 * Every argument is checked on the host before any HIP call: PGM_EINVAL for a null plan / values / codes /
 * tables, n_latent outside 1 .. PGM_EM_MAX_LATENT, a latent column listed twice, in no family, or with two
 * cardinalities, L > PGM_EM_MAX_CONFIGS, more than PGM_EM_MAX_FAMILIES families with a latent, an observed
 * column >= n_cols, and a window outside ld.  pgm_fit_estep_info needs no device. */
#define PGM_EM_MAX_LATENT 8      /* latent variables of one call */
#define PGM_EM_MAX_CONFIGS 4096  /* product of their cardinalities */
#define PGM_EM_MAX_FAMILIES 32   /* families of the plan with a latent in scope */
#define PGM_EM_FLOOR 1e-10       /* EM.py:116-126: max(cpd value, 1e-10) */
typedef struct {
  int32_t n_latent, n_configs;                 /* L = n_configs */
  int32_t n_latent_families, n_plain_families; /* families with / without a latent in scope */
  int32_t block, rows_per_block;               /* work-items per workgroup, rows it takes for its group */
  int32_t lds_bytes, reserved;                 /* dynamic LDS of the launch: the fp64 tile + the index scratch */
} pgm_em_info_t;
int pgm_fit_estep_info(void *plan, const int32_t *latent_cols, int32_t n_latent, pgm_em_info_t *info);
int pgm_fit_estep(void *plan, const int32_t *latent_cols, int32_t n_latent, const double *values,
                  const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                  double *tables, double *loglik, void *stream);

/* ---------------------------------------------------------------- per-row log-probability
 * (an extension of ABI 25.)  The log-density of complete rows under a Bayesian network, for the reference's
 * BayesianModelProbability (metrics/bn_inference.py:23-148: per node, np.unique(axis=0) over the parent
 * codes and a Python loop over the rows), in one streaming pass over the column-major uint8 codes that
 * pgm_fit_count reads and pgm_sample_forward / pgm_gibbs_sweep write.
 *
 * plan is an ordinary fit plan: one family per node.  values and logv (device, fp64) have the plan's flat
 * layout, so values may be the buffer pgm_fit_finish wrote.
 *
 * pgm_fit_log_values: logv[i] = log(values[i]) over the flat layout in one launch; values[i] == 0 gives
 * -inf.  logv may alias values.  A negative or NaN value returns PGM_EINVAL (a device flag read back after
 * the launch: the call synchronises the stream).
 *
 * pgm_fit_logprob covers the rows [row0, row0 + n_rows) of codes[col * ld + row].  For such a row
 *   logp[row] = sum over the families f, in plan order, of
 *               logv[offsets[f] + x_node * stride_0 + sum_v x_parent_v * stride_v]
 * in fp64, starting from +0.0, each addition separately rounded (logp: optional, device, fp64, ld entries
 * indexed by buffer row; rows outside the window are not touched).  A row's value depends on its own codes
 * and logv only: its bits are the same whatever the launch geometry, the alignment path, row0, ld or the
 * other rows.  A row with a zero-probability cell is -inf.
 *
 * A row that holds PGM_EV_MISSING in any column a family reads is skipped: its logp is NaN and it is left
 * out of total.  A code that is neither PGM_EV_MISSING nor a state never indexes a table: its row is skipped
 * in the same way and the call returns PGM_EINDEX, through the device flag of pgm_fit_count (so the call
 * synchronises the stream).  n_skipped (optional, device, one int64) receives the number of skipped rows.
 *
 * total (optional, device, one fp64) receives the sum of the window's row values that are not skipped,
 * added without floating-point atomics in an order that is a function of n_rows alone.  With
 * R = PGM_LOGP_ROWS_PER_BLOCK and B = PGM_LOGP_BLOCK: workgroup b takes the window's rows [b R, (b + 1) R),
 * a skipped row or a row past the window counting +0.0; work-item t adds the rows t, t + B, t + 2 B, ... of
 * the workgroup in that order, a tree adds the work-items' sums (step w = B / 2, B / 4 .. 1: item t < w
 * adds item t + w), giving one partial per workgroup; a second launch of one workgroup adds the partials
 * the same way (work-item t takes the partials t, t + B, ... in index order, then the tree).  So total is
 * bit-identical from run to run and between the four-rows-per-lane and one-row paths.  The partials belong
 * to the handle: calls on one plan must not overlap, and a call covers at most PGM_LOGP_MAX_BLOCKS * R rows.
 *
 * Every argument is checked on the host before any HIP call: PGM_EINVAL for a null plan / values / logv /
 * codes, an fp64 or int64 pointer that is not 8-byte aligned, n_cols smaller than the plan's columns,
 * negative counts, a window outside ld, and more rows than one call covers.  n_rows == 0 is PGM_OK with
 * total = 0 and n_skipped = 0 and launches no kernel.  pgm_fit_logprob_info needs no device. */
#define PGM_LOGP_BLOCK 256            /* work-items per workgroup */
#define PGM_LOGP_ROWS_PER_BLOCK 1024  /* consecutive rows one workgroup takes: one dword of codes per lane and column */
#define PGM_LOGP_MAX_BLOCKS 65536     /* block partials a handle keeps: 64 Mi rows per call */
typedef struct {
  int32_t block;          /* work-items per workgroup */
  int32_t rows_per_block; /* rows one workgroup takes */
  int32_t vec4;           /* the launch takes the four-rows-per-lane path (codes, ld, row0 multiples of 4) */
  int32_t n_families;
  int64_t n_partials;     /* block partials of a launch over n_rows rows = its workgroups */
} pgm_logp_info_t;
/* launch geometry and the kernel path of a call with these (codes, ld, row0, n_rows): only the alignment of
 * the pointer matters */
int pgm_fit_logprob_info(void *plan, const void *codes, int64_t ld, int64_t row0, int64_t n_rows,
                         pgm_logp_info_t *info);
int pgm_fit_log_values(void *plan, const double *values, double *logv, void *stream);
int pgm_fit_logprob(void *plan, const double *logv, const uint8_t *codes, int32_t n_cols, int64_t ld,
                    int64_t row0, int64_t n_rows, double *logp, double *total, int64_t *n_skipped,
                    void *stream);

/* ---------------------------------------------------------------- forward sampling
 * BayesianModelSampling.forward_sample / likelihood_weighted_sample / rejection_sample and
 * DiscreteBayesianNetwork.simulate (sampling/Sampling.py:30-406, DiscreteBayesianNetwork.py:1400-1704)
 * on the device: every node of every row in one launch, into the column-major uint8 codes that
 * pgm_fit_count and the fused row plan read.  An extension of ABI 25.
 *
 * A plan is built from pgm_fit_family records given in a TOPOLOGICAL order: every parent's column is
 * the node column of an earlier family, with the cardinality it has there, and no column is the node of
 * two families (PGM_EINVAL otherwise).  values and cdf share the fit plan's flat layout: family f at
 * [offsets[f], offsets[f] + sizes[f]), shaped [node_card, parent configurations] in C order.
 *
 * pgm_sample_cdf writes the running sums of every CPD column in state order (c_0 = p_0,
 * c_s = c_{s-1} + p_s, fp64); values may be the buffer pgm_fit_finish wrote.  A column whose total is
 * not finite or not > 0 returns PGM_EINVAL (a device flag read back after the launch: the call
 * synchronises the stream).
 *
 * pgm_sample_forward draws the rows [row0, row0 + n_rows) of codes[col * ld + row]; buffer row row0 + i
 * is row first_row + i of the endless stream of `seed`.  The uniform of stream row r and code column c
 * is Philox4x32-10 with counter (r & 0xffffffff, r >> 32, c >> 1, 0) and key (seed & 0xffffffff,
 * seed >> 32): words (x0, x1) for an even c, (x2, x3) for an odd one, u = ((x_hi << 21) | (x_lo >> 11))
 * * 2^-53.  With t = u * c_{K-1} the state is min{s : c_s > t}, or min{s : c_s == c_{K-1}} if there is
 * none.  So a result depends on (seed, stream row, column) only: not on the launch geometry, the
 * alignment path, the row window or the device.
 *
 * modes (host, one uint8 per family, NULL: all PGM_SAMPLE_FREE): PGM_SAMPLE_GIVEN takes the code the
 * column already holds; PGM_SAMPLE_OBSERVED does too and multiplies the row's weight by
 * value / column total (likelihood weighting); a row whose given code is PGM_EV_MISSING is drawn (and
 * its weight left alone).  A given code that is neither a state nor PGM_EV_MISSING never indexes a table:
 * the nodes after it in plan order are written PGM_EV_MISSING for that row, its weight is 0 and the call
 * returns PGM_EINDEX (a device flag read back after the launch: the call synchronises the stream).
 * weights (optional, fp64, ld entries indexed by buffer row; needs values) start at 1 and are multiplied
 * in plan order.  uniforms (optional, fp64 [n_cols, ld], the layout of codes, values in [0, 1)) replace
 * the generator: the test hook for the boundaries of the running sums.
 *
 * Every argument is checked on the host before any HIP call; pgm_sample_plan_create and
 * pgm_sample_plan_info need no device. */
#define PGM_SAMPLE_FREE 0
#define PGM_SAMPLE_GIVEN 1
#define PGM_SAMPLE_OBSERVED 2
typedef struct {
  int32_t n_families;
  int32_t n_cols;            /* 1 + the largest code column */
  int32_t block;             /* work-items per workgroup */
  int32_t rows_per_block;    /* rows one workgroup draws */
  int64_t total_bins;        /* entries of the values / cdf buffers */
  int64_t total_columns;     /* CPD columns (parent configurations) over all families */
  int32_t vec4;              /* the launch takes the four-rows-per-lane path (codes, ld, row0 multiples of 4) */
  int32_t weighted;          /* weights given */
  int32_t explicit_uniforms; /* uniforms given */
  int32_t reserved;
} pgm_sample_info_t;
int pgm_sample_plan_create(const pgm_fit_family *families, int32_t n_families, void **plan);
int pgm_sample_plan_destroy(void *plan);
/* layout, launch geometry and the kernel path of a launch with these (codes, ld, row0, weights, uniforms):
 * only NULL and alignment of the pointers matter; any output may be NULL */
int pgm_sample_plan_info(void *plan, const void *codes, int64_t ld, int64_t row0, const void *weights,
                         const void *uniforms, pgm_sample_info_t *info, int64_t *offsets, int64_t *sizes);
int pgm_sample_cdf(void *plan, const double *values, double *cdf, void *stream);
int pgm_sample_forward(void *plan, const double *values, const double *cdf, const uint8_t *modes, uint8_t *codes,
                       int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int64_t first_row, uint64_t seed,
                       double *weights, const double *uniforms, void *stream);

/* ---------------------------------------------------------------- likelihood-weighted posteriors
 * (an extension of ABI 25.)  The reference's ApproxInference (inference/ApproxInference.py) for a batch of
 * evidence rows: every row draws n_samples samples, weights them and adds them to its own histograms in
 * one fused kernel.  No sampled code is written to memory.
 *
 * plan, values, cdf and modes are pgm_sample_forward's.  evidence[col * ld + row0 + r] (device, uint8,
 * read only) is evidence row r of n_rows: in a PGM_SAMPLE_GIVEN or PGM_SAMPLE_OBSERVED family the node
 * takes that code, PGM_EV_MISSING means it is drawn; a PGM_SAMPLE_FREE family never reads its column.
 * Sample s of row r is stream row first_row + r * n_samples + s of `seed`, with pgm_sample_forward's
 * uniforms and selection rule: the codes are the ones pgm_sample_forward writes for the evidence row
 * replicated n_samples times.  Its log-weight is lw = sum log(value / column total) over the
 * PGM_SAMPLE_OBSERVED families whose given code is a state, in plan order, in fp64 from +0.0 (one
 * division, one log and one addition per term; a value of 0 gives -inf).  The weight is never a product.
 *
 * targets is an ordinary fit plan.  Family (cols, cards) is one table over those columns in the fit
 * layout (the first column slowest): one column is a marginal, several are a joint.  The tables lie end
 * to end, total_bins entries per evidence row.  A sample adds its weight to one bin of every family.
 *
 * The sums are integers.  With M_r the largest lw of row r, K = min(52, 62 - ceil(log2 n_samples)):
 * a sample adds q = llrint(ldexp(exp(lw - M_r), K)) (0 when M_r = -inf) as uint64, first into an LDS tile
 * and from there with global integer atomics.  So every output of a row is bit-identical whatever the
 * workgroup size, the split of the samples over workgroups and the other rows of the batch.
 *   acc [n_rows, total_bins] uint64   the sums (written, not added to)
 *   scale [n_rows] fp64               M_r
 *   post [n_rows, total_bins] fp64    optional: acc / sum q, per family (all weights 0: 0/0 = NaN)
 *   log_evidence [n_rows] fp64        optional: M_r + log(sum q * 2^-K / n_samples); all weights 0: -inf
 *   ess [n_rows] fp64                 optional: (sum q')^2 / sum q'^2, q' = q >> max(K - 20, 0), integer
 *                                     sums; all weights 0: 0
 * All device memory, indexed by r, 8-byte aligned.  A row with an evidence code that is neither
 * PGM_EV_MISSING nor a state in a GIVEN / OBSERVED family indexes nothing: its acc is 0, its post, scale
 * and log_evidence are NaN, its ess 0, the other rows are not affected and the call returns PGM_EINDEX
 * (a device flag read back after the launches: the call synchronises the stream).
 *
 * A workgroup of `block` work-items takes PGM_LW_CHUNK samples of one row; a lane owns a sample at a time
 * and keeps its codes in LDS as [column][lane] bytes.  First every (row, chunk) finds its largest lw;
 * then the same samples are drawn again from the counter, quantised against M_r and added; a last launch
 * divides.  LDS: 8 * total_bins + n_cols * block + 2 KiB for the reductions, n_cols the sample plan's.
 * block 0 takes the largest of 256 / 128 / 64 that fits PGM_LW_LDS_BUDGET; 64, 128 or 256 forces it (the
 * test hook).  When none fits the call returns PGM_EINVAL.  The chunk maxima and row sums belong to the
 * sample plan's handle (plan handles, above): a launch covers PGM_LW_MAX_GROUPS (row, chunk) pairs and a
 * call makes as many as its rows need.
 *
 * Every argument is checked on the host before any HIP call: PGM_EINVAL for a null plan / targets /
 * values / cdf / evidence / acc / scale, an fp64 or uint64 pointer that is not 8-byte aligned, n_cols
 * smaller than either plan's columns, a window outside ld, n_samples outside 1 .. PGM_LW_MAX_SAMPLES, a
 * stream range past 2^63, a target column that is the node of no family of the sample plan or whose
 * cardinality differs from that node's, an unknown mode and a block other than 0 / 64 / 128 / 256.
 * n_rows == 0 is PGM_OK and launches nothing.  pgm_sample_posterior_info needs no device. */
#define PGM_LW_CHUNK 1024            /* samples of one row a workgroup takes */
#define PGM_LW_MAX_SAMPLES (1 << 20) /* samples per evidence row */
#define PGM_LW_LDS_BUDGET 163840     /* bytes of LDS a workgroup may take: the CU's 160 KiB */
#define PGM_LW_MAX_GROUPS 65536      /* (row, chunk) workgroups of one launch */
typedef struct {
  int32_t block;         /* work-items per workgroup */
  int32_t chunk;         /* samples per workgroup */
  int32_t k;             /* K: a weight of 1 (the row's largest) is 2^K */
  int32_t lds_bytes;     /* dynamic LDS of the accumulating launch */
  int32_t lds_budget;
  int32_t n_cols;        /* code columns a lane keeps: the sample plan's */
  int64_t total_bins;    /* bins per evidence row: the target plan's */
  int64_t chunks_per_row;
  int64_t workgroups;      /* n_rows * chunks_per_row */
  int64_t rows_per_launch; /* rows one launch covers */
} pgm_lw_info_t;
int pgm_sample_posterior_info(void *plan, void *targets, int64_t n_rows, int64_t n_samples, int32_t block,
                              pgm_lw_info_t *info);
int pgm_sample_posterior(void *plan, void *targets, const double *values, const double *cdf, const uint8_t *modes,
                         const uint8_t *evidence, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                         int64_t n_samples, int64_t first_row, uint64_t seed, int32_t block,
                         unsigned long long *acc, double *scale, double *post, double *log_evidence, double *ess,
                         void *stream);

/* ---------------------------------------------------------------- Gibbs sampling
 * GibbsSampling (sampling/Sampling.py:409-631) on the device: many chains per launch, one per lane, in
 * the column-major uint8 codes that pgm_fit_count and the fused row plan read.  An extension of ABI 25.
 *
 * A plan is built from factors: pgm_fit_family records (columns, cardinalities) in the C order of the
 * factor's table.  A CPD is the factor [node, parents...]; a Markov network's factor is given as it
 * stands.  values share the fit plan's flat layout: factor f at [offsets[f], offsets[f] + sizes[f]).
 * PGM_EINVAL unless every column 0 .. n_cols - 1 occurs in a factor, a column has the cardinality card[]
 * gives wherever it occurs, cardinalities are <= 254, a factor has at most PGM_MAX_DIMS columns, fewer
 * than 2^31 entries and lists no column twice.  The plan holds, per column, its incident factors
 * (factor, position of the column in it) in CSR form, factors ascending, of any degree.
 *
 * pgm_gibbs_sweep advances the chains in rows [row0, row0 + n_chains) of codes[col * ld + row] in place:
 * chains [first_chain, first_chain + n_chains) of the stream of `seed`, through sweeps first_sweep ..
 * first_sweep + n_sweeps - 1 (1 <= sweep < 2^32).  A sweep visits the columns in ascending order; a column
 * with clamp[col] != 0 (host, one uint8 per column, NULL: none) keeps its code.  For any other column of
 * cardinality K, w_s (s = 0 .. K - 1) is the product of values[off_f + base_f + s * stride_f] over the
 * incident factors in list order, starting from the first factor's value, base_f from the chain's
 * current codes of the factor's other columns; c_0 = w_0, c_s = c_{s-1} + w_s, t = u * c_{K-1}; the new
 * code is min{s : c_s > t}, or min{s : c_s == c_{K-1}} if there is none (pgm_sample_forward's rule).
 * Every multiplication and addition is one separately rounded fp64 operation (no FMA).  u is the
 * forward sampler's generator with the sweep as the fourth counter word: Philox4x32-10, counter
 * (chain & 0xffffffff, chain >> 32, col >> 1, sweep); sweep 0 is pgm_sample_forward's stream.  So a
 * result depends on (seed, chain, sweep, column) only: not on the kernel path, row0, or how the sweeps
 * are split over calls.
 *
 * A conditional whose total is not finite or not > 0 cannot be drawn (the state has probability 0): the
 * variable keeps its code, the walk goes on and the call returns PGM_EINVAL.  A chain that holds a code
 * >= its column's cardinality in any column is not advanced and nothing is indexed with that code: the
 * call returns PGM_EINDEX.  Both are device flags read back after the launch: the call synchronises the
 * stream.
 *
 * trace (optional, uint8 [n_cols, ld_trace]): after local sweep j = 1 .. n_sweeps with j % thin == 0 the
 * state of the chain in row row0 + r goes to trace[col * ld_trace + (j / thin - 1) * n_chains + r]; codes
 * always receives the final state.  uniforms (optional, fp64 [n_sweeps, n_cols, ld], values in [0, 1))
 * replace the generator: the test hook for the boundaries of the running sums.
 *
 * pgm_gibbs_start writes a start state for models that cannot be forward-sampled: column c of chain r is
 * min(floor(u * card[c]), card[c] - 1) with the sweep-0 uniform of (seed, first_chain + r, c).
 *
 * Every argument is checked on the host before any HIP call; pgm_gibbs_plan_create and
 * pgm_gibbs_plan_info need no device. */
#define PGM_GIBBS_LDS 0    /* the chains' codes live in LDS for the whole launch */
#define PGM_GIBBS_GLOBAL 1 /* the state stays in the code matrix */
typedef struct {
  int32_t n_factors;
  int32_t n_cols;
  int64_t total_entries;     /* entries of the values buffer */
  int64_t total_incidences;  /* (column, incident factor) pairs */
  int64_t blocks;            /* workgroups of a launch with n_chains chains */
  int32_t max_degree;        /* most factors incident to one column */
  int32_t max_card;
  int32_t path;              /* PGM_GIBBS_LDS / PGM_GIBBS_GLOBAL */
  int32_t block;             /* work-items = chains per workgroup */
  int32_t lds_bytes;         /* dynamic LDS of the launch: n_cols * block on the LDS path, else 0 */
  int32_t lds_budget;        /* the LDS path is taken while n_cols * block <= lds_budget */
  int32_t reg_card;          /* cardinalities up to this keep a conditional's weights in registers */
  int32_t reserved;
} pgm_gibbs_info_t;
int pgm_gibbs_plan_create(const pgm_fit_family *factors, int32_t n_factors, const int32_t *card, int32_t n_cols,
                          void **plan);
int pgm_gibbs_plan_destroy(void *plan);
/* layout and the launch a call with n_chains chains makes; offsets / sizes: n_factors entries; inc_off:
 * n_cols + 1 entries; inc: 2 * total_incidences entries (factor, position); any output may be NULL */
int pgm_gibbs_plan_info(void *plan, int64_t n_chains, pgm_gibbs_info_t *info, int64_t *offsets, int64_t *sizes,
                        int32_t *inc_off, int32_t *inc);
int pgm_gibbs_start(void *plan, uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_chains,
                    int64_t first_chain, uint64_t seed, void *stream);
int pgm_gibbs_sweep(void *plan, const double *values, uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0,
                    int64_t n_chains, int64_t first_chain, int64_t first_sweep, int64_t n_sweeps, uint64_t seed,
                    const uint8_t *clamp, uint8_t *trace, int64_t ld_trace, int64_t thin, const double *uniforms,
                    void *stream);

/* ---------------------------------------------------------------- pairwise counts
 * The contingency table of EVERY pair of columns, optionally per state of a stratum (class) column, in
 * one launch, and the statistics the tree learners weigh their edges with (estimators/TreeSearch.py:
 * mutual information, normalised and adjusted mutual information; the reference calls scikit-learn once
 * per pair, TreeSearch.py:196-356).  An extension of ABI 25.
 *
 * Variable v reads code column cols[v] (each column at most once) and has cards[v] states, 1 .. 254;
 * code PGM_EV_MISSING means missing.  The states of all variables are laid end to end: variable v owns
 * the states [offsets[v], offsets[v] + cards[v]), S = sum of the cardinalities = offsets[n_vars], and
 * Sp = S rounded up to 16.  `counts` is an int64 device array [n_strata][Sp][Sp] (table_size = Sp * Sp
 * entries per stratum): for u < v in the order given,
 *   counts[c][offsets[u] + a][offsets[v] + b]
 * is the number of rows with u = a, v = b and stratum code c, none of the three missing (without a stratum
 * column: none of the two).  With O the rows x S one-hot matrix this is the block (u, v) of O^T O, which
 * one int8 MFMA kernel computes exactly (0/1 operands, int32 accumulators per row slice, int64 atomics).
 * ONLY these blocks are specified: the cells of a variable against itself, the lower triangle (v before
 * u) and the padding rows and columns past S hold unspecified values.
 *
 * pgm_pair_count ADDS to `counts` (the caller zeroes them; several calls may count several row windows)
 * the rows [row0, row0 + n_rows) of codes[col * ld + row] (n_cols columns of ld rows).  strat_col = -1:
 * one stratum (n_strata = 1); else stratum c takes the rows whose code in column strat_col is c <
 * n_strata, and rows with any other code there (PGM_EV_MISSING included) are counted nowhere; the stratum
 * column may also be one of the variables.  A row with PGM_EV_MISSING in a column is left out of exactly
 * the pairs with that column (per-pair complete cases).  A code of a variable that takes part in a pair
 * and is neither PGM_EV_MISSING nor < its cardinality is counted nowhere, and the call returns PGM_EINDEX
 * (a device flag the call reads back after the launch, so the call synchronises the stream).  The rows
 * are cut into slices of slice_rows rows (chosen on the host so that a small input still fills the
 * device; at most 2^30, so an int32 accumulator cannot wrap); pgm_pair_plan_set_slice forces a slice
 * length (0: back to the automatic choice), which changes the launch and none of the integers.  Operands
 * are loaded 16 aligned bytes at a time when codes, ld and row0 are multiples of 16, else byte by byte;
 * no load leaves [row0, row0 + n_rows) of a column the plan names.
 *
 * pgm_pair_mi writes, for stratum c and pair p (u < v, u-major: (0,1), (0,2), ..., (1,2), ...) at
 * [c * n_pairs + p]: from the block's own row sums a, column sums b and total N (so missing cells are
 * handled per pair),
 *   mi = max(0, sum over n_ab > 0 of (n_ab / N) (log n_ab + log N - log a_a - log b_b)),
 *   hu = sum over a_a > 0 of (a_a / N) (log N - log a_a), hv likewise over b, and n = N;
 * N = 0 gives mi = hu = hv = 0.  pgm_pair_emi writes the expected mutual information of the block's
 * marginals under the hypergeometric model (scikit-learn's expected_mutual_information): the sum over
 * a, b and n = max(1, a_a + b_b - N) .. min(a_a, b_b) of (n / N) log(N n / (a_a b_b)) times the
 * hypergeometric probability, the exponential of nine lgamma terms; 0 when N = 0.
 * Both are fp64 with one workgroup of PGM_PAIR_STAT_BLOCK work-items per (stratum, pair), every addition
 * in an order fixed by the pair's shape alone and no floating-point atomics: a pair's numbers are
 * bit-identical whatever else is in the plan.  mi, hu, hv, emi (fp64) and n (int64) are device arrays of
 * n_strata * n_pairs entries.
 *
 * Every argument is checked on the host before any HIP call; pgm_pair_plan_create, pgm_pair_plan_info,
 * pgm_pair_plan_set_slice and pgm_pair_count_info need no device.  The handle follows the rules of the
 * plan handles (parameter learning, above). */
#define PGM_PAIR_STAT_BLOCK 64 /* work-items per (stratum, pair) of the statistic kernels */
typedef struct {
  int32_t n_vars;
  int32_t n_cols;          /* 1 + the largest code column read */
  int64_t S;               /* states of all variables */
  int64_t Sp;              /* S rounded up to 16: the side of a stratum's table */
  int64_t table_size;      /* Sp * Sp: int64 entries of one stratum */
  int64_t n_pairs;         /* n_vars (n_vars - 1) / 2 */
  int64_t n_tile_pairs;    /* 16 x 16 tile pairs (ti <= tj) that touch a block of two variables */
  int64_t n_groups;        /* 64 x 64 super-tile pairs that hold one of them: grid.x of the count launch */
  int64_t n_state_entries; /* entries of the state table: S rounded up to 64 */
  int64_t slice_rows;      /* the forced slice length, 0: automatic */
} pgm_pair_info_t;
int pgm_pair_plan_create(const int32_t *cols, const int32_t *cards, int32_t n_vars, void **plan);
int pgm_pair_plan_destroy(void *plan);
/* offsets: n_vars + 1 entries; tile_pairs: 2 * n_tile_pairs entries (ti, tj); groups: 3 * n_groups entries
 * (I, J, check: bit 0 the A side, bit 1 the B side verifies its codes); any output may be NULL */
int pgm_pair_plan_info(void *plan, pgm_pair_info_t *info, int64_t *offsets, int32_t *tile_pairs, int32_t *groups);
int pgm_pair_plan_set_slice(void *plan, int64_t slice_rows);
/* the launch a count over this window makes: rows per slice, slices, and whether the 16-byte loads apply */
int pgm_pair_count_info(void *plan, const void *codes, int64_t ld, int64_t row0, int64_t n_rows, int32_t n_strata,
                        int64_t *slice_rows, int64_t *n_slices, int32_t *vec16);
int pgm_pair_count(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                   int32_t strat_col, int32_t n_strata, int64_t *counts, void *stream);
int pgm_pair_mi(void *plan, const int64_t *counts, int32_t n_strata, double *mi, double *hu, double *hv, int64_t *n,
                void *stream);
int pgm_pair_emi(void *plan, const int64_t *counts, int32_t n_strata, double *emi, void *stream);

/* ---------------------------------------------------------------- linear-Gaussian networks
 * LinearGaussianBayesianNetwork (models/LinearGaussianBayesianNetwork.py) on a resident fp64 value
 * matrix X[col * ld + row] (n_cols columns of ld rows, column-major like the codes; a call works on the
 * rows [row0, row0 + n_rows)).  An extension of ABI 25.
 *
 * THE GRAM HANDLE (pgm_lg_gram_plan_*, pgm_lg_colsum, pgm_lg_gram) is made over d distinct columns
 * cols[0 .. d).  The OLS fit of every node of any DAG over them is a function of the centred Gram matrix
 * S = (X - mu)^T (X - mu), which two passes give:
 *   pgm_lg_colsum writes sums[j] = the fp64 sum of column cols[j] over the window and counts[j] = n_rows.
 *     A workgroup adds PGM_LG_COLSUM_CHUNK-row pieces (its work-items stride the piece, then a fixed
 *     tree); a second kernel adds the pieces of a column in index order.  No floating-point atomics.
 *   pgm_lg_gram takes a shift c[0 .. d) (device; the caller divides the sums, so c is within rounding of
 *     the mean) and writes the symmetric (d + 1) x (d + 1) matrix `out` (device, row-major) of the columns
 *     x_j - c_j with a column of ones appended at index d:
 *       out[j][k] = sum (x_j - c_j)(x_k - c_k),  out[j][d] = sum (x_j - c_j),  out[d][d] = n_rows.
 *     S_jk = out[j][k] - out[j][d] out[k][d] / n is exact algebra whatever c is, and harmless numerically
 *     because c is the mean up to rounding; raw moments (c = 0) or a shift by the first row lose every
 *     digit when |mu| >> sigma.  The upper triangle is computed, the lower one mirrored from it.
 * The d + 1 columns are cut into tiles of PGM_LG_TILE = 16 and super-tiles of PGM_LG_SUPER = 4 tiles; a
 * group is super-tile I against super-tile J (I <= J): up to 4 x 4 accumulators of 16 x 16 fp64 fed by
 * v_mfma_f64_16x16x4_f64, one wave per (group, row slice).  A diagonal group forms one fragment per tile
 * and uses it on both sides (10 accumulators); with d + 1 <= 64 it is the only group, so the data is
 * read from memory exactly once.  Lane (i = lane & 15, q = lane >> 4) loads the PGM_LG_ROWS_PER_LANE = 4
 * consecutive rows r + 4 q .. r + 4 q + 3 of its column of a PGM_LG_STEP = 16-row step, and MFMA s of the
 * step uses the s-th of them on both sides: a sum over rows does not depend on which k slot a row takes
 * as long as both operands agree, and a lane then reads 32 contiguous bytes (two 16-byte loads) instead
 * of 8.  The 16-byte loads need X, ld * 8 and row0 * 8 to be multiples of 16; any other window takes
 * 8-byte loads (pgm_lg_gram_info tells which).  The shift is subtracted in registers; a row at or past
 * the window's end contributes zero AFTER the shift; the ones column is a constant, not a load; no load
 * leaves the window of a column the plan names.
 * Rows are cut into slices of slice_rows rows (a multiple of PGM_LG_STEP, chosen so that a launch has
 * about PGM_LG_TARGET_BLOCKS waves and a slice at least PGM_LG_SLICE_MIN rows; pgm_lg_gram_plan_set_slice
 * forces a length, 0: automatic).  The handle keeps max_slices = max(4, PGM_LG_TARGET_BLOCKS / n_groups)
 * slice partials; a forced length that would need more is raised to ceil(n_rows / max_slices) rounded up.
 * Each (slice, group) writes its partial with plain stores and a second kernel adds the slices in slice
 * order: an entry is bit-identical from run to run and, for a fixed slice length, whatever other columns
 * the handle has and wherever its own two columns stand in it.
 * A NaN or Inf cell makes the entries of its column's row and column of `out` non-finite (the pair with
 * the ones column included) and no other; no bit pattern is used as an index.
 * pgm_lg_colsum and pgm_lg_gram with n_rows == 0 return PGM_OK, launch nothing and write nothing.
 *
 * THE NETWORK HANDLE (pgm_lg_net_*) is made over families in a topological order: family f owns
 * fam_cols[fam_off[f] .. fam_off[f + 1]), the node's column first, then its parents' in the CPD's order.
 * Refused (PGM_EINVAL): a parent that is not the node of an earlier family, a column that is the node
 * of two families or listed twice in one, more than PGM_LG_MAX_PARENTS parents.  The coefficients of a
 * call are a device array `coef` of n_coef = fam_off[n] + n entries: family f at fam_off[f] + f holds
 * beta_0, beta_1 .. beta_p (the parents' order) and sigma.  They are read with wave-uniform (scalar)
 * loads, so the limit on p is a bound on a kernel's loop, not on a register or LDS array.
 *   pgm_lg_sample: one lane per row, families in order, x_v = beta_0 + sum_i beta_i x_{p_i} + sigma_v z.
 *     z is the normal of stream row first_row + r and COLUMN col_v: columns 2 k and 2 k + 1 share the
 *     Philox4x32-10 call of forward sampling (counter (row lo, row hi, k, 0), key = seed); with u0 the
 *     53-bit uniform of words (x0, x1) and u1 that of (x2, x3), rho = sqrt(-2 log(1 - u0)),
 *     z_{2k} = rho cospi(2 u1), z_{2k+1} = rho sinpi(2 u1).  A row depends on (seed, stream row) alone,
 *     not on the window, the batch or the launch geometry.  A lane re-reads only what it wrote itself.
 *   pgm_lg_logpdf: logp[r] (n_rows entries, r counted from row0) = sum over f in order of konst[f] - 0.5 ((x_v - m_f) / sigma_f)^2, m_f
 *     = beta_0 + sum_i beta_i x_{p_i} added in the parents' order; konst[f] = -log sigma_f - 0.5 log 2 pi
 *     comes from the host (device array, n entries).  total = the sum of the window's logp: per workgroup
 *     of PGM_LG_BLOCK rows a fixed tree, then one workgroup adds the partials in a fixed order (as
 *     pgm_fit_logprob).  logp or total may be NULL, not both.  At most PGM_LG_MAX_BLOCKS * PGM_LG_BLOCK
 *     rows per call.  A non-finite cell gives a non-finite logp for its row only (and total).
 *   pgm_lg_affine needs no handle: out[j * ld_out + r] = c[j] + sum_i W[j * n_in + i] X[in_cols[i] * ld +
 *     row0 + r], i ascending; W, c device, in_cols a HOST array that travels in the kernel arguments,
 *     PGM_LG_AFFINE_CHUNK columns per launch (later launches add to out in the same order).
 *
 * Every argument is checked on the host before any HIP call; the plan create / info / set_slice calls
 * and pgm_lg_gram_info need no device.  The handles follow the rules of the plan handles (parameter
 * learning, above). */
#define PGM_LG_TILE 16
#define PGM_LG_SUPER 4
#define PGM_LG_ROWS_PER_LANE 4
#define PGM_LG_STEP 16            /* rows of one step: 4 k slots x PGM_LG_ROWS_PER_LANE */
#define PGM_LG_TARGET_BLOCKS 1024 /* waves a Gram launch aims at: four per CU of a 256-CU device */
#define PGM_LG_SLICE_MIN 1024     /* rows of the shortest automatic slice of a window longer than that */
#define PGM_LG_COLSUM_CHUNK 4096  /* rows of one piece of a column sum (more when a column has > 1024 pieces) */
#define PGM_LG_COLSUM_MAX_CHUNKS 1024
#define PGM_LG_MAX_PARENTS 4096
#define PGM_LG_BLOCK 256          /* rows (and work-items) per workgroup of sample / logpdf / affine */
#define PGM_LG_MAX_BLOCKS 65536   /* workgroups of one pgm_lg_logpdf call */
#define PGM_LG_AFFINE_CHUNK 256
typedef struct {
  int32_t d;           /* columns of the handle */
  int32_t n_cols;      /* 1 + the largest column read */
  int32_t n_tiles;     /* ceil((d + 1) / 16) */
  int32_t n_super;     /* ceil(n_tiles / 4) */
  int32_t single_wave; /* 1: d + 1 <= 64, one diagonal group reads the data once */
  int32_t reserved;
  int64_t n_groups;    /* super-tile pairs I <= J: grid.x of the Gram launch */
  int64_t n_tile_pairs; /* 16 x 16 accumulators (ti <= tj) that hold part of the upper triangle */
  int64_t out_size;    /* (d + 1)^2 doubles */
  int64_t max_slices;  /* slice partials the handle keeps */
  int64_t slice_rows;  /* the forced slice length, 0: automatic */
} pgm_lg_gram_info_t;
int pgm_lg_gram_plan_create(const int32_t *cols, int32_t d, void **plan);
int pgm_lg_gram_plan_destroy(void *plan);
/* groups: 2 * n_groups entries (I, J); any output may be NULL */
int pgm_lg_gram_plan_info(void *plan, pgm_lg_gram_info_t *info, int32_t *groups);
int pgm_lg_gram_plan_set_slice(void *plan, int64_t slice_rows);
/* the launch a Gram over this window makes: rows per slice, slices, and whether the 16-byte loads apply */
int pgm_lg_gram_info(void *plan, const void *X, int64_t ld, int64_t row0, int64_t n_rows, int64_t *slice_rows,
                     int64_t *n_slices, int32_t *vec16);
int pgm_lg_colsum(void *plan, const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, double *sums,
                  int64_t *counts, void *stream);
int pgm_lg_gram(void *plan, const double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                const double *shift, double *out, void *stream);
typedef struct {
  int32_t n_families;
  int32_t n_cols;      /* 1 + the largest column read or written */
  int32_t max_parents; /* of the plan's families */
  int32_t reserved;
  int64_t n_coef;      /* fam_off[n] + n entries of coef */
} pgm_lg_net_info_t;
int pgm_lg_net_create(const int32_t *fam_off, const int32_t *fam_cols, int32_t n_families, void **plan);
int pgm_lg_net_destroy(void *plan);
/* coef_off: n_families entries, where a family's beta_0 stands in coef; may be NULL */
int pgm_lg_net_info(void *plan, pgm_lg_net_info_t *info, int64_t *coef_off);
int pgm_lg_sample(void *plan, const double *coef, double *X, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows,
                  int64_t first_row, uint64_t seed, void *stream);
int pgm_lg_logpdf(void *plan, const double *coef, const double *konst, const double *X, int32_t n_cols, int64_t ld,
                  int64_t row0, int64_t n_rows, double *logp, double *total, void *stream);
int pgm_lg_affine(const double *W, const double *c, const int32_t *in_cols, int32_t n_in, int32_t n_out, const double *X,
                  int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, double *out, int64_t ld_out, void *stream);

/* ---------------------------------------------------------------- Gaussian structure learning
 * Partial correlations (estimators/CITests.py pearsonr, GaussCITester) and the Gaussian structure scores
 * (estimators/StructureScore.py LogLikelihoodGauss, BICGauss, AICGauss) from the moment matrix pgm_lg_gram
 * leaves on the device: G [(d + 1) x (d + 1)], the ones column at index d, and its shift c[0 .. d).  Nothing
 * reads the n rows again.  An extension of ABI 25.
 *
 * A JOB is a conditioning set K and 1 .. PGM_LGS_MAX_TARGETS targets T, all indices 0 .. d into G; its
 * result is a function of the Schur complement T|K = M_TT - M_TK M_KK^-1 M_KT, the residual cross-products
 * of the targets after least squares on K (which does not depend on the least-squares solution taken, so
 * a collinear K only needs dropped pivots).  Conditioning on column d is "with an intercept".
 *
 * THE JOB BATCH HANDLE (pgm_lgs_jobs_*) is made once per batch from HOST arrays: job j owns
 * job_cols[job_off[j] .. job_off[j + 1]), its K first, then its n_targets[j] targets.  Refused
 * (PGM_EINVAL) before any HIP call: an index outside 0 .. d, a column listed twice in a job, a target
 * that is also in K, n_targets outside 1 .. 3, more than PGM_LGS_MAX_COND conditioning columns.  The
 * handle sorts the jobs into buckets by (|K|, n_targets), each in the batch's own order, so a launch has
 * uniform trip counts: one launch per bucket, the outputs in the batch's order.  An empty batch
 * (n_jobs = 0) is a valid handle whose calls return PGM_OK and launch nothing.
 *
 * The two calls read G, shift (device) and n = G[d][d], and write device arrays of n_jobs entries:
 *   pgm_lgs_pcorr: with intercept = 0 every job is (K without column d; X, Y, d): the reference regresses X
 *     and Y on Z WITHOUT an intercept and centres the residuals afterwards, so with R = T|K,
 *     cov_ab = R_ab - R_a1 R_b1 / n.  With intercept = 1 every job is (K with column d; X, Y) and cov = R.
 *     A batch whose jobs have another shape is refused.  coef = cov_XY / sqrt(cov_XX cov_YY) clipped to
 *     [-1, 1]; pvalue = I_{1 - coef^2}((n - 2) / 2, 1 / 2) (csrc/pgm_ibeta.h), the two-sided Student t with
 *     n - 2 degrees of freedom, NOT reduced by |K|, as the reference.
 *     NaN coef and pvalue, for that job only: n <= 2; a non-finite entry of G among the job's columns; a
 *     target without residual variance, that is one constant to rounding (centred variance at or below
 *     n (64 u c)^2, u = 2^-53) or whose own pivot would be dropped (cov_aa <= RCOND times its centred
 *     variance).  rank is still written.
 *   pgm_lgs_score: every job is (K with column d; v).  rss = T|K, df = the kept pivots among K's columns other
 *     than d, llf = -n/2 (log(2 pi rss / n) + 1) (statsmodels' Gaussian GLM llf), and score = llf
 *     (PGM_LGS_LL), llf - (df + 2) / 2 log n (PGM_LGS_BIC) or llf - (df + 2) (PGM_LGS_AIC).  rss <= 0:
 *     score +inf, as the closed form gives.  A non-finite entry: score and rss NaN.
 *   rank: the pivots kept among K (the ones column counts).
 * One device routine serves both: gather the lower triangle of the (|K| + t)^2 block; when K is not empty
 * and has no ones column turn it into raw moments, M_uv = G_uv + c_u G_v1 + c_v G_u1 + n c_u c_v (c_d = 0;
 * the cancellation this brings when |mean| >> sd is a property of what the reference computes); scale K
 * to unit diagonal, a column whose diagonal is not positive being dropped; Cholesky in outer-product form
 * WITHOUT pivoting, in K's order, where a pivot at or below RCOND = 1e-11 drops its column; the trailing
 * t x t block is T|K.
 * Two paths, chosen by a job's own |K| alone:
 *   lane path, |K| <= PGM_LGS_LANE_MAX: one job per lane, |K| and t template parameters, every loop
 *     unrolled, the packed triangle in registers (no scratch; DESIGN.md has the register counts);
 *   wave path, up to PGM_LGS_MAX_COND: one wave (a 64-lane workgroup) per job, the triangle in LDS with an
 *     odd row length, one lane per row of an elimination step, a barrier between steps.  (|K| + t)
 *     ((|K| + t) | 1) + 3 (|K| + t) doubles: 37,520 bytes at the cap, four workgroups per CU.  The cap of 64
 *     is one row per lane; the LDS budget would allow more.
 * The order of a job's arithmetic is fixed by its own columns, every store is a plain store and there are
 * no atomics: a job's outputs are bit-identical whatever else is in the batch, wherever it stands in it
 * and from run to run (not across permutations of its columns).
 * pgm_lgs_jobs_create, pgm_lgs_jobs_info and pgm_lgs_ibeta_half (the host build of the p-value's
 * I_{1 - y}(a, 1/2)) need no device.  The handle follows the rules of the plan handles. */
#define PGM_LGS_MAX_COND 64
#define PGM_LGS_LANE_MAX 7
#define PGM_LGS_MAX_TARGETS 3
#define PGM_LGS_LL 0
#define PGM_LGS_BIC 1
#define PGM_LGS_AIC 2
typedef struct {
  int32_t n_jobs;
  int32_t d;
  int32_t n_buckets;      /* distinct (|K|, n_targets): launches of one call */
  int32_t max_cond;       /* the largest |K| */
  int64_t n_lane_jobs;    /* jobs with |K| <= PGM_LGS_LANE_MAX */
  int64_t n_wave_jobs;
  int64_t wave_lds_bytes; /* LDS of a workgroup of the largest wave-path bucket, 0: none */
} pgm_lgs_info_t;
int pgm_lgs_jobs_create(const int32_t *job_off, const int32_t *job_cols, const int32_t *n_targets, int32_t n_jobs, int32_t d,
                        void **handle);
int pgm_lgs_jobs_destroy(void *handle);
/* buckets: 4 * n_buckets entries (|K|, n_targets, first, count); order: n_jobs job indices, bucket by bucket;
 * any output may be NULL */
int pgm_lgs_jobs_info(void *handle, pgm_lgs_info_t *info, int32_t *buckets, int32_t *order);
int pgm_lgs_pcorr(void *handle, const double *G, const double *shift, int32_t d, int32_t intercept, double *coef, double *pvalue,
                  int32_t *rank, void *stream);
int pgm_lgs_score(void *handle, const double *G, const double *shift, int32_t d, int32_t kind, double *score, double *rss,
                  int32_t *rank, void *stream);
/* *out = I_{1 - y}(a, 1/2) by the host build of the device's function (csrc/pgm_ibeta.h) */
int pgm_lgs_ibeta_half(double a, double y, double *out);

/* ---------------------------------------------------------------- dynamic Bayesian networks
 * Filtering, smoothing and the log-likelihood of MANY evidence sequences under one two-slice network
 * (DynamicBayesianNetwork / DBNInference, which rebuilds and calibrates a junction tree per slice of one
 * sequence) in one launch: a sequence is a row, its state lives in LDS.  An extension of ABI 25.
 *
 * DATA.  codes[(T + 1) n, ld], uint8, column-major: column t n + v is node v of slice t, a row is a
 * sequence, PGM_EV_MISSING is "not observed in this cell".  The call reads rows [row0, row0 + n_rows).
 *
 * THE PLAN is made on the host from the n slice nodes' cardinalities, a `clamped` and a `queried` flag
 * per node, the slice-0 families and the transition families (pgm_fit_family: the node, then its parents,
 * the table in the CPD's layout).  A slice-0 family's columns are 0 .. n - 1.  A transition family's node
 * is a column n .. 2n - 1 (slice t + 1) and its parents are columns 0 .. n - 1 (slice t) or n .. 2n - 1.
 * Every node has exactly one family in each set.  The tables of a set lie end to end in the order given
 * (pgm_dbn_info: off0 / off1), as in a fit plan, so the values of a fitted network are used as they are.
 * A CLAMPED node is observed in every cell of the batch and enters only as a table offset read from the
 * codes; a FREE node may be observed or missing per cell.  The enumerated state of a slice is the joint x
 * of the free nodes (the last fastest), J = prod card(free) <= PGM_DBN_MAX_CONFIGS; the message between
 * slices is over the free INTERFACE nodes (free nodes that are a slice-t parent of a transition family),
 * S = prod of their cardinalities, S divides J.  Refused (PGM_EINVAL) before any HIP call: n outside
 * 1 .. 255, a cardinality outside 1 .. 255, J above the cap, a family column out of range or listed
 * twice, a cardinality that differs from the node's, a slice-t parent whose node has no slice-0 family, a
 * node without or with two families in a set, a table or a set of tables of 2^31 entries or more.
 *
 * THE RECURSION, per sequence, forward in time (a_t the message, I(x) the interface part of x):
 *   alpha_0(x)  = 1[e_0(x)] prod_v P0(x_v | pa)                       c_0 = sum alpha_0, alpha_0 /= c_0
 *   a_t(i)      = sum_{x : I(x) = i} alpha_t(x)
 *   alpha_t+1(x') = 1[e_t+1(x')] prod_{v: no free slice-t parent} P(x'_v | pa)
 *                   sum_i a_t(i) prod_{v: a free slice-t parent} P(x'_v | pa(i, x')),  divided by c_t+1
 *   loglik = sum_t log c_t = log P(e_0:T);  filter_t(v) = the marginal of alpha_t.
 * The first product does not depend on i and is taken once per x'; an x' that contradicts the cell's
 * evidence is 0 without being evaluated.  Backward, with beta_T = 1:
 *   gamma_t(x) = alpha_t(x) beta_t(I(x)) / (its sum);  smooth_t(v) = the marginal of gamma_t
 *   beta_t-1(i) = sum_x' Phi_t(i, x') beta_t(I(x')) / c_t,   Phi_t the summand of alpha_t.
 * Only a_t (S doubles) and c_t are kept per slice, in the caller's scratch of n_rows (T + 1) (S + 1)
 * doubles; alpha_t is recomputed from a_t-1 on the way back.  Scratch is needed for smooth only; a
 * scratch that is too small is PGM_EINVAL (the caller splits the batch by rows).
 *
 * MAPPING.  One wave per workgroup.  J <= 64: 64 / pow2ceil(J) sequences share a wave, one x' per lane;
 * J > 64: one sequence per wave, the lanes stride over x'.  alpha, a and beta live in LDS (8 (J + 2 S)
 * + 6 n bytes per sequence; fewer sequences per wave when that would pass 160 KiB), the CPD tables and
 * the plan's offset tables are read from global memory.  Every sum is taken in an order fixed by (J, S,
 * card) alone, a lane's own terms in ascending order and then a butterfly over the sequence's lanes;
 * the factors of a product are multiplied in node order, whatever order the families were given in;
 * there are no atomics on values: a sequence's outputs are bit-identical whatever else is in the batch
 * and wherever it stands in it.
 *
 * OUTPUTS, each optional (NULL): filter, smooth [n_rows, T + 1, Q] fp64 with Q = sum card(queried), the
 * queried nodes in node order, a sequence's block contiguous; loglik [n_rows]; impossible [n_rows] uint8.
 * A clamped queried node yields its indicator.  A sequence whose evidence has probability 0 (some c_t =
 * 0) gets impossible = 1, loglik = -inf, NaN filter marginals from that slice on and NaN smooth marginals
 * at every slice; nothing else in the batch is affected.  PGM_EV_MISSING in a clamped column, or a code
 * >= its cardinality anywhere, never indexes a table and makes the call return PGM_EINVAL (a device flag
 * read back after the launch: the call synchronises the stream).  n_rows = 0 is PGM_OK and launches
 * nothing.  pgm_dbn_plan_create and pgm_dbn_info need no device; pgm_dbn_run checks every argument on the
 * host before any HIP call (null plan / codes / values, an fp64 pointer that is not 8-byte aligned,
 * n_cols != n_slices n, n_slices outside 1 .. 65535, a row window outside ld).  The handle follows the
 * rules of the plan handles. */
#define PGM_DBN_MAX_CONFIGS 4096
typedef struct {
  int32_t n;              /* slice nodes */
  int32_t n_free;
  int32_t n_configs;      /* J */
  int32_t n_interface;    /* S */
  int32_t n_prev_families; /* transition families with a free slice-t parent: evaluated per (i, x') */
  int32_t n_cur_families;  /* transition families without one: evaluated once per x' */
  int32_t seq_per_wave;
  int32_t block;          /* work-items per workgroup */
  int32_t n_query;        /* Q */
  int32_t reserved;
  int64_t lds_bytes;      /* LDS of a workgroup */
  int64_t values0;        /* entries of the slice-0 / the transition value buffer */
  int64_t values1;
  int64_t scratch_per_slice; /* doubles of scratch per sequence and slice: S + 1 */
} pgm_dbn_info_t;
int pgm_dbn_plan_create(const int32_t *card, const uint8_t *clamped, const uint8_t *queried, int32_t n,
                        const pgm_fit_family *families0, int32_t n_families0, const pgm_fit_family *families1,
                        int32_t n_families1, void **plan);
int pgm_dbn_plan_destroy(void *plan);
/* off0 / off1: the table offset of every family of the set; any output may be NULL */
int pgm_dbn_info(void *plan, pgm_dbn_info_t *info, int64_t *off0, int64_t *off1);
int pgm_dbn_run(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int32_t n_slices,
                const double *values0, const double *values1, double *filter, double *smooth, double *loglik,
                uint8_t *impossible, double *scratch, int64_t scratch_bytes, void *stream);

/* ---------------------------------------------------------------- dynamic Bayesian networks: MAP sequences
 * pgm_dbn_viterbi: the single most probable completion of every sequence of the batch, in one launch, on
 * the plan, the data layout and the mapping of pgm_dbn_run (the queried flags are not used).  One more
 * extension symbol of ABI 25; pgm_dbn_info_t and the other pgm_dbn_* calls are as they were.
 *
 * THE RECURSION, per sequence: the forward one with max for sum, and a backpointer per state.
 *   delta_0(x)    = 1[e_0(x)] prod_v P0(x_v | pa)                  c_0 = max_x delta_0, delta_0 /= c_0
 *   m_t(i)        = max_{x : I(x) = i} delta_t(x);   argx_t(i) = the lowest such x that attains it
 *   delta_t+1(x') = 1[e_t+1(x')] prod_{v: no free slice-t parent} P(x'_v | pa)
 *                   max_i m_t(i) prod_{v: a free slice-t parent} P(x'_v | pa(i, x'))
 *   psi_t+1(x')   = the lowest i that attains that max;   bp_t+1(x') = argx_t(psi_t+1(x'))
 *   c_t+1 = max_x' delta_t+1, delta_t+1 /= c_t+1;   logmap = sum_t log c_t
 *   backtrack: x*_T = the lowest x that attains max delta_T;   x*_t-1 = bp_t(x*_t).
 * logmap = log max_x P(x_0:T, e_0:T): the joint with the evidence, not the conditional.  An x' that
 * contradicts its cell's evidence is 0 without a table read; the factors of a product are multiplied in node
 * order.  Marginal MAP over a subset of the nodes is not this: every free cell is maximised over.
 *
 * TIES go to the lowest index everywhere: a lane keeps its first maximum (strict >) over its ascending
 * indices; the lanes of a sequence are combined by a butterfly over (value, index) in which the larger
 * value wins and the lower index on equality, an operation that commutes, so every lane holds the same
 * pair.  No atomics on values.  A sequence's outputs are bit-identical whatever else is in the batch,
 * wherever it stands in it and however the caller splits the batch by rows.
 *
 * SCRATCH: the backpointers, full states as uint16 (J <= 4096): n_rows T J 2 bytes for T + 1 = n_slices
 * slices (slice 0 has none), 2-byte aligned; the layout is private to the kernel.  A scratch that is too
 * small is PGM_EINVAL (the caller splits the batch by rows); n_slices = 1 needs none.  LDS is the plan's
 * lds_bytes: delta in alpha's place, m in the message's, argx in beta's.
 *
 * OUTPUTS.  path, uint8, column-major [(T + 1) n, ld_out] like codes: column t n + v, row row0_out + r for
 * row r of the window; a free node gets its digit of x*_t (the evidence wherever the cell was observed), a
 * clamped node its code, so path is a complete code matrix.  logmap [n_rows] fp64 and impossible [n_rows]
 * uint8, each optional (NULL).  A sequence whose evidence has probability 0 (some c_t not > 0): impossible
 * = 1, logmap = -inf, PGM_EV_MISSING in every free cell of its path, its clamped cells copied; nothing
 * else in the batch is affected.  Bad codes are treated as in pgm_dbn_run: they never index a table and
 * the call returns PGM_EINVAL after the launch.  Checked on the host before any HIP call (PGM_EINVAL): a
 * null plan / codes / values / path, an fp64 pointer that is not 8-byte aligned, n_cols != n_slices n,
 * n_slices outside 1 .. 65535, a codes or a path row window outside its leading dimension, a scratch that
 * is too small.  n_rows = 0 is PGM_OK and launches nothing. */
int pgm_dbn_viterbi(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int32_t n_slices,
                    const double *values0, const double *values1, uint8_t *path, int64_t ld_out, int64_t row0_out,
                    double *logmap, uint8_t *impossible, void *scratch, int64_t scratch_bytes, void *stream);

/* ---------------------------------------------------------------- dynamic Bayesian networks: expected counts
 * pgm_dbn_estep: the E-step of Baum-Welch for every sequence of the batch, in one launch, on the plan, the
 * data layout, the clamped / free split and the mapping of pgm_dbn_run (the queried flags are not used).
 * Two more extension symbols of ABI 25; pgm_dbn_info_t and the other pgm_dbn_* calls are as they were.
 *
 * THE RECURSION, per sequence.  Forward: pgm_dbn_run's, a_t and c_t kept in the caller's scratch of n_rows
 * (T + 1) (S + 1) doubles (the same rule and the same PGM_EINVAL for a scratch that is too small).  Backward,
 * slice by slice, with gamma_t(x) = alpha_t(x) beta_t(I(x)) as pgm_dbn_run computes it and gs its sum:
 *   t = 0, every slice-0 family f:       tables0[entry of f at x]       += gamma_0(x) / gs
 *   t >= 1, f without a free slice-t parent: tables1[entry of f at x']  += gamma_t(x') / gs
 *   t >= 1, f with a free slice-t parent:    tables1[entry of f at (i, x')] += xi_t(i, x') / gs
 *   xi_t(i, x') = local(x') (a_t-1(i) prod(i, x')) / c_t beta_t(I(x')),   sum_i xi_t(i, x') = gamma_t(x').
 * The entry of a family is the one pgm_dbn_run reads its factor from: tables0 / tables1 are device fp64
 * buffers in the layout of values0 / values1, so pgm_fit_finish | PGM_FIT_WEIGHTED over the same family
 * lists is the M-step.  The tables are ADDED TO, not overwritten, as pgm_fit_estep does.  Slice-0 tables get
 * slice 0 only, the transition tables slices 1 .. T: the maximum-likelihood statistics of the unrolled
 * network.  A term of xi is built by the operations of the matching term of gamma, in the same order (the
 * message times the factors in node order, then local, / c_t, * beta) and weighted by a division by gs:
 * where one (i, x') survives the evidence its weight is g / g = 1.0, and a fully observed batch gives
 * exact integers.  An x' that contradicts its cell's evidence, or a term that is 0, is never added.
 *
 * ACCUMULATION.  PGM_DBN_ESTEP_TILE: an fp64 copy of both table sets lives in LDS behind the sequences'
 * state (when lds_bytes rounded up to 8, + 8 (values0 + values1) <= 160 KiB); the adds are LDS atomics;
 * workgroups take groups of seq_per_wave sequences in a grid-stride loop, the grid capped at max_blocks
 * (256 CUs x the workgroups whose LDS fits a CU, 32 at most), and a workgroup adds the non-zero entries
 * of its tile to the tables once, at its end, one global atomic each.  PGM_DBN_ESTEP_DIRECT (taken when
 * the tile does not fit, or forced by the flag of that name): one workgroup per group, every add a global
 * atomic.  The tables are sums of fp64 atomics in no fixed order: they are NOT bit-identical from run to
 * run (a sum of n non-negative terms is within (n - 1) 2^-53 relative in any order).  loglik and
 * impossible involve no atomics and are bit-identical to pgm_dbn_run's.
 *
 * loglik [n_rows] and impossible [n_rows] are optional (NULL) and as in pgm_dbn_run.  An impossible
 * sequence (some c_t not > 0) adds nothing to any table.  Bad codes are treated as in pgm_dbn_run: they
 * never index a table, the call returns PGM_EINVAL after the launch and the tables are then unspecified.
 * Checked on the host before any HIP call (PGM_EINVAL): everything pgm_dbn_run checks for a smoother, null
 * tables0 / tables1, a table pointer that is not 8-byte aligned, unknown flag bits.  n_rows = 0 is PGM_OK
 * and launches nothing.  pgm_dbn_estep_info needs no device: the path a call with `flags` takes. */
#define PGM_DBN_ESTEP_DIRECT 1u /* flags: every add a global atomic, whether or not the tile fits */
#define PGM_DBN_ESTEP_TILE 0    /* pgm_dbn_estep_info_t.path */
typedef struct {
  int32_t path;          /* PGM_DBN_ESTEP_TILE, or PGM_DBN_ESTEP_DIRECT */
  int32_t tile_fits;     /* whether the tile fits in LDS beside the sequences' state */
  int32_t blocks_per_cu; /* tile path: workgroups whose LDS fits a CU (32 at most); direct: 0 */
  int32_t reserved;
  int64_t lds_bytes;     /* LDS of a workgroup on the path taken */
  int64_t tile_bytes;    /* 8 (values0 + values1) */
  int64_t max_blocks;    /* tile path: grid = min(groups of sequences, max_blocks); direct: 0, one workgroup per group */
} pgm_dbn_estep_info_t;
int pgm_dbn_estep_info(void *plan, uint32_t flags, pgm_dbn_estep_info_t *info);
int pgm_dbn_estep(void *plan, const uint8_t *codes, int32_t n_cols, int64_t ld, int64_t row0, int64_t n_rows, int32_t n_slices,
                  const double *values0, const double *values1, double *tables0, double *tables1, double *loglik,
                  uint8_t *impossible, double *scratch, int64_t scratch_bytes, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PGMHIP_H */

// pgmrows_plan.cpp — the host side of the fused row plan: everything that is arithmetic on a
// pgm_rows_plan and needs no device.  No HIP include: a plain C++17 compiler builds this unit, and
// tools/rows_plan_selftest.cpp links it alone (under ASan/UBSan too).
//
//   rows_plan_source / rows_jit_source  the generator of the plan-specialised kernel source (hipRTC)
//   rows2_aligned / rows_jit2_ok        which specialised kernel a launch may run
//   rows_plan_compile                   pgm_rows_plan -> RowsPlan (validation + descriptor buffer)
//
// The kernels that read the descriptors, the handle and the pgm_rows_* C-ABI: pgmrows.hip.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pgmhip.h"
#include "pgm_internal.h"
#include "pgm_rows.h"

// ----------------------------------------------------------------------------- plan-specialised row kernel
// For plans whose components each have one query variable and no hidden variable (the batched
// predict shape, munin C3), pgm_rows_plan_create also writes a kernel source with every column,
// stride, base offset and cardinality as a literal; hipRTC compiles it for gfx950 on first use.
// One thread per evidence row, 256-row workgroups: the CPT values are staged in LDS with every
// load issued before any LDS write, all evidence codes are loaded once per distinct column, and
// each component's products stay in registers between the mass and the stores.  No descriptor
// loads, no inter-wave exchange, a few hundred bytes of code.  Arithmetic order is exactly the
// generic kernels' (factor products left to right, masses summed in state order, components'
// masses multiplied in order), so results are bit-identical to k_rows_affine / k_rows.
void pgmi_appendf(std::string &o, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  o += buf;
}

// workgroup size of the specialised row kernels (tuning knob PGM_ROWS_JIT_WG: a multiple of 64, <= 1024).
// 512 (r02br, MI355X, C3 = 100k-row launches on 4 queues, two rows per thread): 98 blocks of 1,024
// rows per launch — one CPT staging per 1,024 rows and a quarter of the workgroup dispatches of
// 256 x one row — 26.4 -> 29.1-31.1 G rows/s at 20 steps, 36.2 -> 47.1 G at 400; one queue and
// 1M-row launches unchanged (profiles/r02bq_c3_wg_rowform_sweep.txt, r02br_c3_wg_rowform_confirm.txt)
// r04 (96 resident batches, the HBM regime: profiles/r04e, r04f): 320 — 157 blocks of 640 rows per
// 100 k-row launch keep more CUs streaming than 98 x 1,024 once the outputs go to HBM instead of the
// Infinity Cache; three interleaved repeats, 20 steps: 26.6 / 26.7 / 27.9 G rows/s against 27.3 / 25.1 /
// 25.3 G at 512 (192: 27.0 / 26.7 / 26.0; 128: 25.7 / 25.6 / 26.6; 1,024: 25.5 / 24.7 / 25.5)
// r06 (one 157-block launch never covers the 256 CUs): 192 — 261 blocks of 384 rows per
// 100 k-row launch, every CU a block from each launch; three interleaved repeats at the driver's 20 steps
// (profiles/r06b/): 26.29 / 26.82 / 26.04 G rows/s, frac 0.607 / 0.613 / 0.612, against 25.20 / 26.20 /
// 25.74 G, frac 0.572 / 0.606 / 0.588 at 320; the 400-batch ring is unchanged (0.70-0.71).  A/B knob
// PGM_ROWS_JIT_WG (a multiple of 64 in [64, 1024]), read once.
int jit_wg() {
  static const int wg = [] {
    const char *e = getenv("PGM_ROWS_JIT_WG");
    const int v = e ? atoi(e) : 0;
    return (v >= 64 && v <= 1024 && v % 64 == 0) ? v : 192;
  }();
  return wg;
}

// Every output store of the generated kernels is write-through under every policy (PGM_WT4 / PGM_WT8 /
// PGM_WT16, emit_rows_prelude; why, and what it buys: kRowsJitWriteThrough in pgm_rows.h).

// the distinct evidence columns of a plan, each loaded once per row
static std::vector<int> rows_cols(const pgm_rows_plan *pl) {
  std::vector<int> cols;
  for (int j = 0; j < pl->n_ev; ++j)
    if (std::find(cols.begin(), cols.end(), pl->ev_col[j]) == cols.end()) cols.push_back(pl->ev_col[j]);
  return cols;
}

// the row's evidence codes (row rc of the columns at C + row0, leading dimension ldc): e<i>_<u>
// coherent: system-scope relaxed loads (past every non-coherent cache, no invalidation needed) — the
// ring kernel's codes, which may be written after the launch started
// pol.nt_loads: the plain loads carry the nontemporal hint (codes are read once per launch; the coherent
// form is left alone: nothing shows that `nt` keeps a system-scope load's freshness)
static void emit_rows_code_loads(std::string &o, const std::vector<int> &cols, int R, const RowsPolicy &pol,
                                 bool coherent = false) {
  if (!cols.empty()) o += "  const unsigned char *cr = C + row0 + rc;\n";
  for (size_t i = 0; i < cols.size(); ++i) {
    if (R == 1) {
      if (pol.nt_loads) pgmi_appendf(o, "  const unsigned e%zu_0 = __builtin_nontemporal_load(&cr[%dLL * ldc]);\n", i, cols[i]);
      else pgmi_appendf(o, "  const unsigned e%zu_0 = cr[%dLL * ldc];\n", i, cols[i]);
    } else if (coherent) {
      pgmi_appendf(o, "  const unsigned w%zu = __hip_atomic_load((__attribute__((address_space(1))) unsigned short *)(cr + %dLL * ldc), __ATOMIC_RELAXED, "
                   "__HIP_MEMORY_SCOPE_SYSTEM);\n", i, cols[i]);
      pgmi_appendf(o, "  const unsigned e%zu_0 = w%zu & 255u, e%zu_1 = w%zu >> 8;\n", i, i, i, i);
    } else {
      if (pol.nt_loads)
        pgmi_appendf(o, "  const unsigned w%zu = __builtin_nontemporal_load((const unsigned short *)(cr + %dLL * ldc));\n", i, cols[i]);
      else
        pgmi_appendf(o, "  const unsigned w%zu = *(const unsigned short *)(cr + %dLL * ldc);\n", i, cols[i]);
      pgmi_appendf(o, "  const unsigned e%zu_0 = w%zu & 255u, e%zu_1 = w%zu >> 8;\n", i, i, i, i);
    }
  }
}

// the row's sum-product, normalisation and stores (r, rc, n, M, ldo, MP, G, E, mode, rsM / rsG and the
// loaded codes in scope; VAL(i) = CPT value i); rows past n leave through `leave` ("return" in a grid
// kernel, "break" inside the ring kernel's do-while)
static void emit_rows_compute(std::string &o, const pgm_rows_plan *pl, int R, const std::vector<int> &cols,
                              const char *leave) {
  o += "  unsigned bad = 0u;\n";
  const int NC = pl->n_comp;
  for (int u = 0; u < R; ++u) {
    for (int c = 0; c < NC; ++c) {
      const int lb = pl->comp_loop_begin[c], nq = pl->comp_n_query[c];
      const int fb = pl->comp_fac_begin[c], fe = pl->comp_fac_end[c];
      const int P = nq == 1 ? pl->loop_card[lb] : 1;
      for (int f = fb; f < fe; ++f) {
        pgmi_appendf(o, "  int o%d_%d_%d = %d;\n", c, f - fb, u, pl->fac_base[f]);
        for (int j = pl->fac_ev_begin[f]; j < pl->fac_ev_end[f]; ++j) {
          const int ci = (int)(std::find(cols.begin(), cols.end(), pl->ev_col[j]) - cols.begin());
          const unsigned cd = (unsigned)pl->ev_card[j];
          pgmi_appendf(o, "  { const unsigned x = e%d_%d; bad |= (unsigned)(x >= %uu); o%d_%d_%d += (x >= %uu ? 0 : (int)x) * %d; }\n",
                  ci, u, cd, c, f - fb, u, cd, pl->ev_stride[j]);
        }
      }
      for (int q = 0; q < P; ++q) {
        pgmi_appendf(o, "  const double p%d_%d_%d = ", c, q, u);
        if (fe == fb) o += "1.0";
        for (int f = fb; f < fe; ++f) {
          const int qs = nq == 1 ? pl->fac_stride[f][lb] : 0;
          pgmi_appendf(o, "%sVAL(o%d_%d_%d + %d)", f > fb ? " * " : "", c, f - fb, u, q * qs);
        }
        o += ";\n";
      }
      pgmi_appendf(o, "  const double m%d_%d = p%d_0_%d", c, u, c, u);
      for (int q = 1; q < P; ++q) pgmi_appendf(o, " + p%d_%d_%d", c, q, u);
      o += ";\n";
    }
    pgmi_appendf(o, "  const double z_%d = ", u);
    if (NC == 1) pgmi_appendf(o, "m0_%d", u);
    else {
      o += "1.0";
      for (int c = 0; c < NC; ++c) pgmi_appendf(o, " * m%d_%d", c, u);
    }
    pgmi_appendf(o, ";\n  const bool dead_%d = !(z_%d > 0.0);\n", u, u);
  }
  pgmi_appendf(o, "  if (bad && r < n && E) atomicOr(E, 1);\n  if (r >= n) %s;\n", leave);
  o += "  if (mode & 1) {\n";
  for (int c = 0; c < NC; ++c) {
    const int lb = pl->comp_loop_begin[c], nq = pl->comp_n_query[c];
    if (nq != 1) continue;
    o += "    {";
    for (int u = 0; u < R; ++u)
      pgmi_appendf(o, " const double iv_%d = dead_%d ? __builtin_nan(\"\") : 1.0 / m%d_%d;", u, u, c, u);
    o += "\n";
    for (int q = 0; q < pl->loop_card[lb]; ++q) {
      const int mo = pl->loop_marg_off[lb] + q;
      if (R == 1)
        pgmi_appendf(o, "      PGM_WT8(double, &M[%dLL * ldo + r], p%d_%d_0 * iv_0);\n", mo, c, q);
      else
        pgmi_appendf(o, "      PGM_WT16(rsM, %dLL * ldo + r, p%d_%d_0 * iv_0, p%d_%d_1 * iv_1);\n", mo, c, q, c, q);
    }
    o += "    }\n";
  }
  o += "  }\n  if (mode & 12) {\n";
  for (int u = 0; u < R; ++u) {
    pgmi_appendf(o, "    int m_%d = 0;\n    double mg_%d = 1.0;\n", u, u);
    for (int c = 0; c < NC; ++c) {
      const int lb = pl->comp_loop_begin[c], nq = pl->comp_n_query[c];
      const int P = nq == 1 ? pl->loop_card[lb] : 1;
      const int ms = nq == 1 ? pl->loop_map_stride[lb] : 0;
      o += "    { double b = -1.0, s = -1.0; int bs = 0;\n";
      for (int q = 0; q < P; ++q)
        pgmi_appendf(o, "      if (p%d_%d_%d > b) { s = b; b = p%d_%d_%d; bs = %d; } else if (p%d_%d_%d > s) { s = p%d_%d_%d; }\n",
                c, q, u, c, q, u, q, c, q, u, c, q, u);
      pgmi_appendf(o, "      m_%d += bs * %d;\n", u, ms);
      if (P > 1)
        o += "      const double g = b > 0.0 ? (b - (s < 0.0 ? 0.0 : s)) / b : 0.0;\n";
      else
        o += "      const double g = 1.0;\n";
      pgmi_appendf(o, NC == 1 ? "      mg_%d = g; }\n" : "      mg_%d = fmin(mg_%d, g); }\n", u, u);
    }
  }
  if (R == 1) {
    o += "    if (MP) PGM_WT4(int, &MP[r], dead_0 ? 0 : m_0);\n"
         "    if ((mode & 8) && G) PGM_WT8(double, &G[r], dead_0 ? 0.0 : mg_0);\n  }\n";
  } else {
    o += "    if (MP) PGM_WT8(unsigned long long, (unsigned long long *)(MP + r), "
         "((unsigned long long)(unsigned)(dead_1 ? 0 : m_1) << 32) | (unsigned)(dead_0 ? 0 : m_0));\n";
    o += "    if ((mode & 8) && G) PGM_WT16(rsG, r, dead_0 ? 0.0 : mg_0, dead_1 ? 0.0 : mg_1);\n  }\n";
  }
}

// whether pgm_rows_jit / jit2 stage the nv CPT values (trailing 1.0 included) in LDS
static bool jit_values_lds(int nv) { return nv * 8 <= 48 * 1024; }

// R rows per thread (1, or 2 with 16-B marginal stores / 2-byte code loads); names carry the row's suffix
static void emit_rows_kernel(std::string &o, const pgm_rows_plan *pl, int R, const RowsPolicy &pol) {
  const int NV = pl->n_values + 1;  // + trailing 1.0
  // CPT values staged in LDS when they fit (else gathered straight from global memory through L1/L2)
  const bool lds = jit_values_lds(NV);
  const int WG = jit_wg();
  pgmi_appendf(o, "extern \"C\" __global__ void __launch_bounds__(%d) pgm_rows_jit%s(const double *__restrict__ V, "
             "const unsigned char *__restrict__ C, long long ldc, long long row0, long long n, "
             "double *__restrict__ M, long long ldo, int *__restrict__ MP, double *__restrict__ G, "
             "int *__restrict__ E, int mode) {\n", WG, R == 2 ? "2" : "");
  o += "  const int t = threadIdx.x;\n";
  pgmi_appendf(o, "  const long long r = ((long long)blockIdx.x * %d + t) * %d;\n", WG, R);
  pgmi_appendf(o, "  const long long rc = r < n ? r : n - %d;\n", R);
  if (R == 2)
    o += "  const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(M, 0, 0x7fffffff, 0x00020000);\n"
         "  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(G, 0, 0x7fffffff, 0x00020000);\n";
  const int K = (NV + WG - 1) / WG;
  if (lds) {
    pgmi_appendf(o, "  __shared__ double S[%d];\n", K * WG);
    for (int i = 0; i < K; ++i) pgmi_appendf(o, "  const double s%d = V[t + %d < %d ? t + %d : %d];\n", i, WG * i, NV, WG * i, NV - 1);
  }
  const std::vector<int> cols = rows_cols(pl);
  emit_rows_code_loads(o, cols, R, pol);
  if (lds) {
    for (int i = 0; i < K; ++i) pgmi_appendf(o, "  S[t + %d < %d ? t + %d : %d] = s%d;\n", WG * i, NV, WG * i, NV - 1, i);
    o += "  __syncthreads();\n#define VAL(i) S[i]\n";
  } else {
    o += "#define VAL(i) V[i]\n";
  }
  emit_rows_compute(o, pl, R, cols, "return");
  o += "}\n#undef VAL\n";
}

// ---------------------------------------------------------------------------------------- ring kernel
// pgm_rows_ring: the plan-specialised two-rows-per-thread body run by a RESIDENT grid over a stream of
// row batches (pgm_rows_ring_*).  One launch consumes n_batches batches of n rows; batch b reads and
// writes the buffers of slot b % n_slots (descriptor table D in device memory).  The host publishes
// batches by raising a counter in pinned host memory (ctl[0] = batches posted); the launch may start
// before the first post.  Work item = 128 rows (one wave, two rows per lane) of one batch; item j
// goes to wave j mod W (W = resident waves), so consecutive batches overlap across the chip instead of
// each paying a dispatch.
// Learning that a batch is posted, three levels deep so the host counter sees ONE reader at a time
// (reads of host memory from the GPU are serialised: 768 concurrent first polls cost ~150 us, r03a):
//   1. the count the wave's workgroup last saw (LDS seen_s);
//   2. one wave per workgroup (LDS token) reads the device-memory mirror g[0];
//   3. one wave on the chip (token g[1], agent scope) reads ctl[0] with a system-scope acquire and
//      raises the mirror.
// No acquire fences (an L2 invalidation per workgroup serialises per XCD: ~100 us per launch, r03b):
// the counters are read with relaxed system/agent-scope atomics, and the evidence codes with
// system-scope loads, which go past every non-coherent cache — so codes written (by DMA) after the
// launch started but before their batch was posted are read fresh.  Exit conditions every wave reaches:
// all items done; ctl[1] (cancel) set by the host; or `timeout` ticks of the constant 100 MHz wall
// clock without the needed batch (ctl[2] |= 2); either of the last two raises g[2] (stop) for all.
// The CPT values are staged in LDS once per workgroup for the whole stream.
static void emit_rows_ring(std::string &o, const pgm_rows_plan *pl, const RowsPolicy &pol) {
  const int NV = pl->n_values + 1;
  const int WG = ring_wg();
  const int K = (NV + WG - 1) / WG;
  // the ring's waiting waves back off: the workgroup's token wave reads the chip-wide poll token before
  // trying to take it, and sleeps longer the longer it has waited (4 -> 12 -> 32 x 64 clocks).  768 token
  // waves retrying one atomic every ~0.1 us while the ring idles saturate that address and delay the one
  // wave that reads the host counter (r03: ring-ready 20 steps 17.1 -> 29.5-30.8 G rows/s)
  o += "#define BACKOFF 1\n";
  o += "struct pgm_ring_slot { const unsigned char *C; long long ldc, row0; double *M; long long ldo; int *MP; "
       "double *G; long long pad; };\n";
  pgmi_appendf(o, "extern \"C\" __global__ void __launch_bounds__(%d) pgm_rows_ring(const double *__restrict__ V, "
             "const pgm_ring_slot *__restrict__ D, unsigned n_slots, unsigned *ctl, unsigned *g, unsigned n_batches, "
             "unsigned base, long long n, int *__restrict__ E, int mode, unsigned long long timeout, int signal) {\n", WG);
  o += "  const int t = threadIdx.x;\n";
  pgmi_appendf(o, "  __shared__ double S[%d];\n  __shared__ unsigned seen_s, token_s, stop_s;\n", K * WG);
  for (int i = 0; i < K; ++i) pgmi_appendf(o, "  const double s%d = V[t + %d < %d ? t + %d : %d];\n", i, WG * i, NV, WG * i, NV - 1);
  for (int i = 0; i < K; ++i) pgmi_appendf(o, "  S[t + %d < %d ? t + %d : %d] = s%d;\n", WG * i, NV, WG * i, NV - 1, i);
  o += "  if (t == 0) { seen_s = base; token_s = 0u; stop_s = 0u; }\n  __syncthreads();\n#define VAL(i) S[i]\n";
  // readiness (pgm_rows_ring_wait_ready): every workgroup counts itself in g[4..5] (64-bit, never reset:
  // each launch adds exactly gridDim.x) once its CPT copy is staged; the last one raises ctl[3] for the host
  o += "  if (signal && t == 0) {\n"
       "    const unsigned long long s = atomicAdd((unsigned long long *)(g + 4), 1ull) + 1ull;\n"
       "    if (s % gridDim.x == 0ull) __hip_atomic_store(&ctl[3], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);\n"
       "  }\n";
  pgmi_appendf(o, "  const unsigned long long W = (unsigned long long)gridDim.x * %d;\n", WG / 64);
  pgmi_appendf(o, "  const unsigned long long wv0 = (unsigned long long)blockIdx.x * %d + (t >> 6);\n", WG / 64);
  o += "  const unsigned long long chunks = (unsigned long long)(n + 127) / 128;\n"
       "  const unsigned long long items = chunks * n_batches;\n"
       "  const unsigned long long t0 = wall_clock64();\n"
       "  const bool lead = (t & 63) == 0;\n"
       "  unsigned seen = base;  /* counts are absolute over the ring's lifetime */\n"
       "  for (unsigned long long j = wv0; j < items; j += W) {\n"
       "    const unsigned bt = (unsigned)(j / chunks);\n"
       "    const unsigned ab = base + bt;  /* the batch's absolute number: posted once ctl[0] > ab */\n"
       "    bool stop = false;\n"
       "    while (ab >= seen) {\n"
       "      const unsigned sl = __hip_atomic_load(&seen_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);\n"
       "      if (sl > seen) { seen = sl; continue; }\n"
       "      if (__hip_atomic_load(&stop_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) { stop = true; break; }\n"
       "      unsigned mine = 0u;\n"
       "      if (lead) mine = atomicCAS(&token_s, 0u, 1u) == 0u ? 1u : 0u;\n"
       "      mine = __builtin_amdgcn_readfirstlane(mine);\n"
       "      if (!mine) {\n"
       "        if (wall_clock64() - t0 > timeout) { stop = true; break; }\n"
       "        __builtin_amdgcn_s_sleep(2);\n"
       "        continue;\n"
       "      }\n"
       "      unsigned nap = 0u;\n"
       "      for (;;) {  /* this wave speaks for its workgroup */\n"
       "        unsigned m = __hip_atomic_load(&g[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
       "        if (m <= ab) {\n"
       "          if (__hip_atomic_load(&g[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { stop = true; break; }\n"
       "          unsigned poll = 0u;\n"
       "          if (lead && (!BACKOFF || __hip_atomic_load(&g[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u))\n"
       "            poll = atomicCAS(&g[1], 0u, 1u) == 0u ? 1u : 0u;\n"
       "          poll = __builtin_amdgcn_readfirstlane(poll);\n"
       "          if (poll) {  /* the one reader of the host counter */\n"
       "            const unsigned p = __hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);\n"
       "            if (p > m && lead) __hip_atomic_fetch_max(&g[0], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
       "            if (p > m) m = p;\n"
       "            if (m <= ab) {\n"
       "              const bool cancel = __hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;\n"
       "              const bool late = wall_clock64() - t0 > timeout;\n"
       "              if ((cancel || late) && lead) {\n"
       "                if (late) __hip_atomic_fetch_or(&ctl[2], 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);\n"
       "                __hip_atomic_store(&g[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
       "              }\n"
       "              stop = cancel || late;\n"
       "            }\n"
       "            if (lead) __hip_atomic_store(&g[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);\n"
       "            if (stop) break;\n"
       "          } else if (wall_clock64() - t0 > timeout) {\n"
       "            stop = true;\n"
       "            break;\n"
       "          }\n"
       "        }\n"
       "        if (m > ab) {\n"
       "          seen = m;\n"
       "          if (lead) atomicMax(&seen_s, m);\n"
       "          break;\n"
       "        }\n"
       "        if (!BACKOFF || ++nap <= 2u) __builtin_amdgcn_s_sleep(4);\n"
       "        else if (nap <= 8u) __builtin_amdgcn_s_sleep(12);\n"
       "        else __builtin_amdgcn_s_sleep(32);\n"
       "      }\n"
       "      if (stop && lead) atomicExch(&stop_s, 1u);\n"
       "      if (lead) atomicExch(&token_s, 0u);\n"
       "      if (stop) break;\n"
       "    }\n"
       "    if (stop) break;\n"
       "    const pgm_ring_slot d = D[bt % n_slots];\n"
       "    const unsigned char *__restrict__ C = d.C;\n"
       "    const long long ldc = d.ldc, row0 = d.row0, ldo = d.ldo;\n"
       "    double *__restrict__ M = d.M;\n"
       "    int *__restrict__ MP = d.MP;\n"
       "    double *__restrict__ G = d.G;\n"
       "    const long long r = (long long)(j - (unsigned long long)bt * chunks) * 128 + (t & 63) * 2;\n"
       "    const long long rc = r < n ? r : n - 2;\n"
       "    const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(M, 0, 0x7fffffff, 0x00020000);\n"
       "    const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(G, 0, 0x7fffffff, 0x00020000);\n"
       "    do {\n";
  const std::vector<int> cols = rows_cols(pl);
  emit_rows_code_loads(o, cols, 2, pol, true);
  emit_rows_compute(o, pl, 2, cols, "break");
  o += "    } while (0);\n  }\n}\n#undef VAL\n";
}

// the dispatch floor of a plan (PGM_ROWS_FLOOR, measurement only): the row kernel's grid (R rows per
// thread, as pgm_rows_jit / pgm_rows_jit2), its evidence-column loads and its output stores (same
// addresses, same widths, same cache policy), with the CPT staging, gathers and arithmetic replaced by
// one conversion of the loaded codes
static void emit_rows_floor(std::string &o, const pgm_rows_plan *pl, int R, const RowsPolicy &pol) {
  const int WG = jit_wg();
  pgmi_appendf(o, "extern \"C\" __global__ void __launch_bounds__(%d) pgm_rows_floor%s(const double *__restrict__ V, "
             "const unsigned char *__restrict__ C, long long ldc, long long row0, long long n, "
             "double *__restrict__ M, long long ldo, int *__restrict__ MP, double *__restrict__ G, "
             "int *__restrict__ E, int mode) {\n", WG, R == 2 ? "2" : "");
  pgmi_appendf(o, "  const long long r = ((long long)blockIdx.x * %d + threadIdx.x) * %d;\n  if (r >= n) return;\n", WG, R);
  if (R == 2)
    o += "  const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(M, 0, 0x7fffffff, 0x00020000);\n"
         "  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(G, 0, 0x7fffffff, 0x00020000);\n";
  const std::vector<int> cols = rows_cols(pl);
  o += "  unsigned x = 0u;\n";
  if (!cols.empty()) o += "  const unsigned char *cr = C + row0 + r;\n";
  for (size_t i = 0; i < cols.size(); ++i) {
    if (R == 1 && pol.nt_loads) pgmi_appendf(o, "  x += __builtin_nontemporal_load(&cr[%dLL * ldc]);\n", cols[i]);
    else if (R == 1) pgmi_appendf(o, "  x += cr[%dLL * ldc];\n", cols[i]);
    else if (pol.nt_loads) pgmi_appendf(o, "  x += __builtin_nontemporal_load((const unsigned short *)(cr + %dLL * ldc));\n", cols[i]);
    else pgmi_appendf(o, "  x += *(const unsigned short *)(cr + %dLL * ldc);\n", cols[i]);
  }
  o += "  const double v = (double)x;\n  if (mode & 1) {\n";
  for (int c = 0; c < pl->n_comp; ++c) {
    const int lb = pl->comp_loop_begin[c];
    if (pl->comp_n_query[c] != 1) continue;
    for (int q = 0; q < pl->loop_card[lb]; ++q) {
      const int mo = pl->loop_marg_off[lb] + q;
      if (R == 2) pgmi_appendf(o, "    PGM_WT16(rsM, %dLL * ldo + r, v, v);\n", mo);
      else pgmi_appendf(o, "    PGM_WT8(double, &M[%dLL * ldo + r], v);\n", mo);
    }
  }
  o += "  }\n  if (mode & 12) {\n";
  if (R == 2)
    o += "    if (MP) PGM_WT8(unsigned long long, (unsigned long long *)(MP + r), (unsigned long long)x);\n"
         "    if ((mode & 8) && G) PGM_WT16(rsG, r, v, v);\n  }\n}\n";
  else
    o += "    if (MP) PGM_WT4(int, &MP[r], (int)x);\n    if ((mode & 8) && G) PGM_WT8(double, &G[r], v);\n  }\n}\n";
}

// the store macros of a source.  Default policy: 4/8 B as relaxed agent-scope atomic stores (global_store
// ... sc1), 16 B as a buffer store with the sc1 cache bit (element offset into the resource's base, bytes
// < 2 GiB).  Streaming policies: the same stores, write-through AND nontemporal — no builtin gives a
// global store both bits, so 4/8 B are the instruction itself (sc1 nt, or sc0 sc1 nt); the 16-B buffer
// store takes them in its aux operand (sc0 = 1, nt = 2, sc1 = 16)
static void emit_rows_prelude(std::string &o, const RowsPolicy &pol) {
  o += "typedef unsigned int pgm_u32x4 __attribute__((ext_vector_type(4)));\n";
  if (pol.stores == RowsPolicy::kStoreSc1) {
    o += "#define PGM_WT4(T, p, v) __hip_atomic_store((__attribute__((address_space(1))) T *)(p), (v), "
         "__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)\n"
         "#define PGM_WT8(T, p, v) PGM_WT4(T, p, v)\n";
  } else {
    const char *bits = pol.stores == RowsPolicy::kStoreSc0Sc1Nt ? "sc0 sc1 nt" : "sc1 nt";
    pgmi_appendf(o, "#define PGM_WT4(T, p, v) do { const T s_ = (v); asm volatile(\"global_store_dword %%0, %%1, off %s\" "
                    ":: \"v\"((__attribute__((address_space(1))) T *)(p)), \"v\"(s_) : \"memory\"); } while (0)\n", bits);
    pgmi_appendf(o, "#define PGM_WT8(T, p, v) do { const T s_ = (v); asm volatile(\"global_store_dwordx2 %%0, %%1, off %s\" "
                    ":: \"v\"((__attribute__((address_space(1))) T *)(p)), \"v\"(s_) : \"memory\"); } while (0)\n", bits);
  }
  const int aux = pol.stores == RowsPolicy::kStoreSc1 ? 16 : pol.stores == RowsPolicy::kStoreSc1Nt ? 18 : 19;
  pgmi_appendf(o, "#define PGM_WT16(rs, off, a, b) do { const double2 v_ = make_double2((a), (b)); pgm_u32x4 w_; "
                  "__builtin_memcpy(&w_, &v_, 16); __builtin_amdgcn_raw_buffer_store_b128(w_, rs, (int)((off) * 8), 0, %d); } "
                  "while (0)\n", aux);
}

// the whole source of a plan: both row kernels, both floor kernels, the ring kernel.  The policy changes
// how memory is touched and nothing else: the default one emits the text the golden files pin
static std::string rows_jit_source(const pgm_rows_plan *pl, const RowsPolicy &pol = RowsPolicy()) {
  std::string o;
  emit_rows_prelude(o, pol);
  emit_rows_kernel(o, pl, 1, pol);
  o += "\n";
  emit_rows_kernel(o, pl, 2, pol);
  o += "\n";
  emit_rows_floor(o, pl, 1, pol);
  o += "\n";
  emit_rows_floor(o, pl, 2, pol);
  o += "\n";
  emit_rows_ring(o, pl, pol);
  return o;
}

// the alignment / addressing contract of the two-rows-per-lane body (pgm_rows_jit2, pgm_rows_ring)
bool rows2_aligned(int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0, int64_t n_rows,
                   const double *marg, int64_t ld_out, const int32_t *map, const double *gap, int n_marg) {
  if (n_rows % 2 || ld_codes % 2 || row0 % 2 || ((uintptr_t)codes & 1)) return false;
  if ((mode & PGM_ROWS_MARGINALS) && (((uintptr_t)marg & 15) || ld_out % 2)) return false;
  if (map && ((uintptr_t)map & 7)) return false;
  if ((mode & PGM_ROWS_MAPGAP) && gap && ((uintptr_t)gap & 15)) return false;
  // the write-through 16-B stores address outputs as 32-bit byte offsets below 2 GiB
  if ((mode & PGM_ROWS_MARGINALS) && (uint64_t)(n_marg + 1) * (uint64_t)ld_out * 8 >= (1ull << 31)) return false;
  if ((uint64_t)n_rows * 8 >= (1ull << 31)) return false;
  return true;
}

bool rows_jit2_ok(int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0, int64_t n_rows,
                  const double *marg, int64_t ld_out, const int32_t *map, const double *gap, int n_marg) {
  // measured (MI355X): two rows with 16-B stores once the launch is HBM-bound (4M rows: 110 vs 126 us)
  // and, since the 512-thread workgroups and concurrent queues, at 100k rows too (one queue: equal,
  // 3.9 us; four queues: 2.7 -> 2.1 us per launch of GPU span, r02br); one row below 50k rows
  static constexpr int64_t min_rows = 50000;
  if (n_rows < min_rows) return false;
  return rows2_aligned(mode, codes, ld_codes, row0, n_rows, marg, ld_out, map, gap, n_marg);
}

// ----------------------------------------------------------------------------- launch choice
bool rows_jit_mode(int32_t mode) {
  return !(mode & (PGM_ROWS_JOINT | PGM_ROWS_GENERIC | PGM_ROWS_NO_JIT | PGM_ROWS_VALUES_GLOBAL | PGM_ROWS_ONE_GROUP));
}

int rows_launch_check(const RowsPlan &p, int32_t mode, const uint8_t *codes, int64_t n_rows, const double *marg,
                      const double *joint, int64_t ld_out, const int32_t *map, const double *gap) {
  if (p.max_nt > 0 && !codes) return pgmi_failf(PGM_EINVAL, "rows_plan_run: null codes");
  if ((mode & PGM_ROWS_MARGINALS) && !marg) return pgmi_failf(PGM_EINVAL, "rows_plan_run: marginals requested, marg is null");
  if ((mode & PGM_ROWS_JOINT) && !joint) return pgmi_failf(PGM_EINVAL, "rows_plan_run: joint requested, joint is null");
  if ((mode & PGM_ROWS_JOINT) && p.k.n_comp != 1)
    return pgmi_failf(PGM_EINVAL, "rows_plan_run: joint output needs a single-component plan");
  if ((mode & PGM_ROWS_MAP) && !map) return pgmi_failf(PGM_EINVAL, "rows_plan_run: MAP requested, map is null");
  if ((mode & PGM_ROWS_MAPGAP) && !gap) return pgmi_failf(PGM_EINVAL, "rows_plan_run: MAP gap requested, gap is null");
  if ((mode & (PGM_ROWS_MARGINALS | PGM_ROWS_JOINT)) && ld_out < n_rows)
    return pgmi_failf(PGM_EINVAL, "rows_plan_run: ld_out %lld < n_rows %lld", (long long)ld_out, (long long)n_rows);
  return PGM_OK;
}

int rows_launch_choose(const RowsPlan &p, int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0,
                       int64_t n_rows, const double *marg, int64_t ld_out, const int32_t *map, const double *gap,
                       bool jit, pgm_rows_launch_info_t *info) {
  memset(info, 0, sizeof *info);
  info->kernel = PGM_RK_NONE;
  if (n_rows <= 0) return PGM_OK;
  const RowsK &k = p.k;
  info->rg = 1;
  if (jit) {
    const bool two = rows_jit2_ok(mode, codes, ld_codes, row0, n_rows, marg, ld_out, map, gap, k.n_marg);
    const uint64_t rpb = (uint64_t)jit_wg() * (two ? 2 : 1);  // rows per block
    const uint64_t jblocks = ((uint64_t)n_rows + rpb - 1) / rpb;
    if (jblocks > 0x7fffffffull) return pgmi_failf(PGM_EINVAL, "rows_plan_run: too many rows");
    info->kernel = two ? PGM_RK_JIT2 : PGM_RK_JIT;
    info->values_lds = jit_values_lds(k.n_values);
    info->blocks = (uint32_t)jblocks;
    info->wg = (uint32_t)jit_wg();
    info->lds_bytes = info->values_lds ? (uint32_t)((k.n_values + jit_wg() - 1) / jit_wg() * jit_wg() * 8) : 0;
    return PGM_OK;
  }
  // one workgroup = 64 rows x RG row groups; one wave per component
  const size_t kLds = 64 * 1024;
  size_t vals_bytes = (size_t)((k.n_values + 1) & ~1) * sizeof(double);
  const bool vals_lds = vals_bytes <= 40 * 1024 && !(mode & PGM_ROWS_VALUES_GLOBAL);
  if (!vals_lds) vals_bytes = 0;
  const uint64_t groups = ((uint64_t)n_rows + 63) / 64;
  // amortise the LDS staging of the CPT values over several row groups once the grid is large
  int32_t RG = 1;
  if (vals_lds && !(mode & PGM_ROWS_ONE_GROUP)) RG = (int32_t)std::max<uint64_t>(1, std::min<uint64_t>(8, groups / 4096));
  const uint64_t blocks = (groups + RG - 1) / RG;
  if (blocks > 0x7fffffffull) return pgmi_failf(PGM_EINVAL, "rows_plan_run: too many rows");
  info->values_lds = vals_lds;
  info->rg = RG;
  info->blocks = (uint32_t)blocks;
  info->wg = (uint32_t)(64 * k.n_comp);
  if (p.all_affine && !(mode & PGM_ROWS_JOINT) && !(mode & PGM_ROWS_GENERIC)) {
    const bool do_map = (mode & (PGM_ROWS_MAP | PGM_ROWS_MAPGAP)) != 0;
    // exchange slots: masses only, unless MAP digits / gaps are combined too
    const size_t x_aff = k.n_comp > 1 ? (size_t)k.n_comp * 64 * (do_map ? 2 * sizeof(double) + sizeof(int32_t) : sizeof(double)) : 0;
    info->kernel = PGM_RK_AFFINE;
    info->nf = p.max_nf <= 1 ? 1 : p.max_nf <= 2 ? 2 : 4;
    info->nt = p.max_nt <= 4 ? 4 : 8;
    info->map = do_map;
    info->lds_bytes = (uint32_t)(vals_bytes + x_aff);
    return PGM_OK;
  }
  const size_t x_bytes = (size_t)k.n_comp * 64 * (2 * sizeof(double) + sizeof(int32_t));
  const size_t acc_bytes = (size_t)k.n_marg * 64 * sizeof(double);
  const bool acc_lds = (mode & PGM_ROWS_MARGINALS) && p.any_table && vals_bytes + x_bytes + acc_bytes <= kLds;
  info->kernel = PGM_RK_TABLE;
  info->acc_lds = acc_lds;
  info->maxfc = p.max_nf <= 2 ? 2 : p.max_nf <= 4 ? 4 : p.max_nf <= 8 ? 8 : PGM_ROWS_MAX_FAC;
  info->maxt = p.max_nt <= 4 ? 4 : p.max_nt <= 8 ? 8 : PGM_ROWS_MAX_EV;
  info->lds_bytes = (uint32_t)(vals_bytes + x_bytes + (acc_lds ? acc_bytes : 0));
  return PGM_OK;
}

int rows_launch_info(const pgm_rows_plan *pl, int32_t mode, const uint8_t *codes, int64_t ld_codes, int64_t row0,
                     int64_t n_rows, const double *marg, const double *joint, int64_t ld_out, const int32_t *map,
                     const double *gap, bool jit_available, pgm_rows_launch_info_t *info) {
  if (!pl || !info) return pgmi_failf(PGM_EINVAL, "rows_launch_info: null argument");
  RowsPlan plan;
  int st = rows_plan_compile(pl, plan);
  if (st != PGM_OK) return st;
  if (n_rows > 0) {
    st = rows_launch_check(plan, mode, codes, n_rows, marg, joint, ld_out, map, gap);
    if (st != PGM_OK) return st;
  }
  const bool jit = jit_available && !plan.jit_src.empty() && rows_jit_mode(mode);
  return rows_launch_choose(plan, mode, codes, ld_codes, row0, n_rows, marg, ld_out, map, gap, jit, info);
}

int rows_plan_source(const pgm_rows_plan *pl, std::string &src, const RowsPolicy &pol) {
  if (!pl) return pgmi_failf(PGM_EINVAL, "rows_plan_source: null plan");
  if (pl->n_comp < 1 || pl->n_comp > PGM_ROWS_MAX_COMP || pl->n_fac < 0 || pl->n_fac > PGM_ROWS_MAX_FAC ||
      pl->n_ev < 0 || pl->n_ev > PGM_ROWS_MAX_EV || pl->n_loop < 0 || pl->n_loop > PGM_ROWS_MAX_LOOP)
    return pgmi_failf(PGM_EINVAL, "rows_plan_source: plan out of range");
  for (int c = 0; c < pl->n_comp; ++c)
    if (pl->comp_n_query[c] > 1 || pl->comp_loop_end[c] - pl->comp_loop_begin[c] != pl->comp_n_query[c])
      return pgmi_failf(PGM_EINVAL, "rows_plan_source: component %d is not specialisable (query dims %d, loop dims %d)", c,
                        pl->comp_n_query[c], pl->comp_loop_end[c] - pl->comp_loop_begin[c]);
  src = rows_jit_source(pl, pol);
  return PGM_OK;
}

// ----------------------------------------------------------------------------- plan compiler
int rows_plan_compile(const pgm_rows_plan *pl, RowsPlan &out) {
  if (pl->n_loop < 0 || pl->n_loop > PGM_ROWS_MAX_LOOP || pl->n_query < 0 || pl->n_query > pl->n_loop ||
      pl->n_fac < 0 || pl->n_fac > PGM_ROWS_MAX_FAC || pl->n_ev < 0 || pl->n_ev > PGM_ROWS_MAX_EV ||
      pl->n_values < 0 || pl->n_comp < 1 || pl->n_comp > PGM_ROWS_MAX_COMP || pl->n_marg < 0 ||
      pl->n_marg > PGM_ROWS_MAX_MARG)
    return pgmi_failf(PGM_EINVAL, "rows_plan_create: plan out of range (loop %d query %d fac %d ev %d comp %d marg %d)",
                      pl->n_loop, pl->n_query, pl->n_fac, pl->n_ev, pl->n_comp, pl->n_marg);
  RowsK k;
  memset(&k, 0, sizeof k);
  k.one_idx = pl->n_values;  // a trailing 1.0 multiplies into the products of unused factor slots
  k.n_values = pl->n_values + 1;
  k.n_marg = pl->n_marg;
  k.n_joint = pl->n_joint;
  k.n_comp = pl->n_comp;
  // factors: value ranges and evidence ownership
  std::vector<int64_t> fac_hi(pl->n_fac);
  for (int f = 0; f < pl->n_fac; ++f) {
    if (pl->fac_ev_begin[f] < 0 || pl->fac_ev_end[f] > pl->n_ev || pl->fac_ev_begin[f] > pl->fac_ev_end[f])
      return pgmi_failf(PGM_EINVAL, "rows_plan_create: factor %d evidence range", f);
    int64_t mx = pl->fac_base[f];
    for (int kk = 0; kk < pl->n_loop; ++kk) mx += (int64_t)(pl->loop_card[kk] - 1) * pl->fac_stride[f][kk];
    for (int j = pl->fac_ev_begin[f]; j < pl->fac_ev_end[f]; ++j) mx += (int64_t)(pl->ev_card[j] - 1) * pl->ev_stride[j];
    if (mx >= pl->n_values || pl->fac_base[f] < 0)
      return pgmi_failf(PGM_EINVAL, "rows_plan_create: factor %d reads past values", f);
    fac_hi[f] = mx + 1;
  }
  std::vector<int> ev_owner(pl->n_ev, -1);
  for (int f = 0; f < pl->n_fac; ++f)
    for (int j = pl->fac_ev_begin[f]; j < pl->fac_ev_end[f]; ++j) {
      if (ev_owner[j] != -1) return pgmi_failf(PGM_EINVAL, "rows_plan_create: evidence term %d feeds two factors", j);
      ev_owner[j] = f;
    }
  std::vector<RowsComp> comps(pl->n_comp);
  std::vector<int32_t> tab;
  int covered_loop = 0, covered_fac = 0, nq_total = 0, max_nf = 1, max_nt = 0;
  bool any_table = false;
  for (int c = 0; c < pl->n_comp; ++c) {
    const int lb = pl->comp_loop_begin[c], nq = pl->comp_n_query[c], le = pl->comp_loop_end[c];
    const int fb = pl->comp_fac_begin[c], fe = pl->comp_fac_end[c];
    if (lb != covered_loop || nq < 0 || lb + nq > le || le > pl->n_loop || fb != covered_fac || fe < fb ||
        fe > pl->n_fac)
      return pgmi_failf(PGM_EINVAL, "rows_plan_create: component %d ranges (loops [%d,%d,%d) factors [%d,%d))", c, lb,
                        lb + nq, le, fb, fe);
    covered_loop = le;
    covered_fac = fe;
    uint64_t P = 1, H = 1;
    for (int kk = lb; kk < le; ++kk) {
      if (pl->loop_card[kk] <= 0) return pgmi_failf(PGM_EINVAL, "rows_plan_create: loop_card[%d] <= 0", kk);
      (kk < lb + nq ? P : H) *= (uint64_t)pl->loop_card[kk];
      if (kk < lb + nq && (pl->loop_marg_off[kk] < 0 || pl->loop_marg_off[kk] + pl->loop_card[kk] > pl->n_marg))
        return pgmi_failf(PGM_EINVAL, "rows_plan_create: loop %d marginal rows out of range", kk);
    }
    const int nf = fe - fb;
    if (P * H * (uint64_t)std::max(nf, 1) + tab.size() >= (1ull << 26))
      return pgmi_failf(PGM_EINVAL, "rows_plan_create: component %d index space too large for the fused kernel", c);
    for (int f = fb; f < fe; ++f)
      for (int kk = 0; kk < pl->n_loop; ++kk)
        if ((kk < lb || kk >= le) && pl->fac_stride[f][kk] != 0)
          return pgmi_failf(PGM_EINVAL, "rows_plan_create: factor %d strides a loop dim outside its component", f);
    max_nf = std::max(max_nf, nf);
    RowsComp &cd = comps[c];
    memset(&cd, 0, sizeof cd);
    cd.nf = nf;
    cd.nq = nq;
    cd.P = (int32_t)P;
    cd.H = (int32_t)H;
    cd.q_lo = nq_total;
    for (int kk = lb; kk < lb + nq; ++kk) {
      k.q_marg_off[nq_total] = pl->loop_marg_off[kk];
      k.q_card[nq_total] = pl->loop_card[kk];
      ++nq_total;
    }
    cd.q_hi = nq_total;
    cd.marg0 = nq >= 1 ? pl->loop_marg_off[lb] : 0;
    cd.simple = (nq <= 1 && H == 1) ? 1 : 0;
    any_table |= !cd.simple;
    cd.mstride = nq == 1 ? pl->loop_map_stride[lb] : 0;
    int64_t vlo = pl->n_values, vhi = 0;
    for (int j = 0; j < PGM_ROWS_MAX_FAC; ++j) cd.fbase[j] = k.one_idx;
    for (int f = fb; f < fe; ++f) {
      cd.fbase[f - fb] = pl->fac_base[f];
      cd.fstride[f - fb] = nq == 1 ? pl->fac_stride[f][lb] : 0;
      vlo = std::min<int64_t>(vlo, pl->fac_base[f]);
      vhi = std::max<int64_t>(vhi, fac_hi[f]);
    }
    cd.val_lo = vlo < vhi ? (int32_t)vlo : 0;
    cd.val_hi = vlo < vhi ? (int32_t)vhi : 0;
    // evidence terms: one contiguous run per component
    int lo = pl->n_ev, hi = 0;
    for (int f = fb; f < fe; ++f)
      if (pl->fac_ev_end[f] > pl->fac_ev_begin[f]) {
        lo = std::min(lo, pl->fac_ev_begin[f]);
        hi = std::max(hi, pl->fac_ev_end[f]);
      }
    if (lo >= hi) lo = hi = pl->n_ev;
    for (int j = lo; j < hi; ++j)
      if (ev_owner[j] < fb || ev_owner[j] >= fe)
        return pgmi_failf(PGM_EINVAL, "rows_plan_create: component %d evidence terms are not contiguous", c);
    cd.ev_lo = lo;
    cd.nt = hi - lo;
    max_nt = std::max(max_nt, hi - lo);
    for (int j = 0; j < 8; ++j) {
      cd.a_col[j] = hi > lo ? pl->ev_col[lo] : 0;
      cd.a_card[j] = 256;
    }
    if (hi - lo <= 8)
      for (int j = lo; j < hi; ++j) {
        cd.a_col[j - lo] = pl->ev_col[j];
        cd.a_card[j - lo] = pl->ev_card[j];
        if (ev_owner[j] - fb < 4) cd.a_S[j - lo][ev_owner[j] - fb] = pl->ev_stride[j];
      }
    if (cd.simple) continue;
    // per-entry tables, entries in C-order over [query dims..., hidden dims...] (last fastest)
    const int nl = le - lb;
    std::vector<int32_t> dig(nl, 0);
    cd.off_base = (int32_t)tab.size();
    for (uint64_t e = 0; e < P * H; ++e) {
      uint64_t t = e;
      for (int d = nl - 1; d >= 0; --d) {
        dig[d] = (int32_t)(t % (uint64_t)pl->loop_card[lb + d]);
        t /= (uint64_t)pl->loop_card[lb + d];
      }
      for (int f = fb; f < fe; ++f) {
        int64_t o = 0;
        for (int d = 0; d < nl; ++d) o += (int64_t)dig[d] * pl->fac_stride[f][lb + d];
        tab.push_back((int32_t)o);
      }
    }
    cd.marg_base = (int32_t)tab.size();
    for (uint64_t qi = 0; qi < P; ++qi) {
      uint64_t t = qi;
      for (int d = nq - 1; d >= 0; --d) {
        dig[d] = (int32_t)(t % (uint64_t)pl->loop_card[lb + d]);
        t /= (uint64_t)pl->loop_card[lb + d];
      }
      for (int d = 0; d < nq; ++d) tab.push_back(pl->loop_marg_off[lb + d] + dig[d]);
    }
    cd.map_base = (int32_t)tab.size();
    for (uint64_t qi = 0; qi < P; ++qi) {
      uint64_t t = qi;
      int64_t m = 0;
      for (int d = nq - 1; d >= 0; --d) {
        m += (int64_t)(t % (uint64_t)pl->loop_card[lb + d]) * pl->loop_map_stride[lb + d];
        t /= (uint64_t)pl->loop_card[lb + d];
      }
      tab.push_back((int32_t)m);
    }
  }
  if (covered_loop != pl->n_loop || covered_fac != pl->n_fac || nq_total != pl->n_query)
    return pgmi_failf(PGM_EINVAL, "rows_plan_create: components do not cover the loop dims / factors");
  // descriptor buffer: [RowsComp x n_comp][RowsTerm blocks][tables].  Each component's terms are
  // padded with no-op terms to the kernel's static term count (4 or 8) when they fit it.
  const int padt = max_nt <= 4 ? 4 : max_nt <= 8 ? 8 : 0;
  std::vector<RowsTerm> terms;
  for (int c = 0; c < pl->n_comp; ++c) {
    RowsComp &cd = comps[c];
    const int lo = cd.ev_lo, nt = cd.nt, fb = pl->comp_fac_begin[c];
    cd.ev_lo = (int32_t)terms.size();
    for (int j = lo; j < lo + nt; ++j)
      terms.push_back(RowsTerm{pl->ev_col[j], pl->ev_stride[j], pl->ev_card[j], ev_owner[j] - fb});
    if (nt > 0)
      for (int j = nt; j < padt; ++j) terms.push_back(RowsTerm{pl->ev_col[lo], 0, 256, -1});
  }
  terms.push_back(RowsTerm{0, 0, 256, -1});
  std::vector<int32_t> &buf = out.desc;
  buf.assign(comps.size() * (sizeof(RowsComp) / 4), 0);
  if (!comps.empty()) memcpy(buf.data(), comps.data(), comps.size() * sizeof(RowsComp));
  k.terms_off = (int32_t)buf.size();
  buf.resize(buf.size() + terms.size() * 4);
  memcpy(buf.data() + k.terms_off, terms.data(), terms.size() * sizeof(RowsTerm));
  k.tab_off = (int32_t)buf.size();
  buf.insert(buf.end(), tab.begin(), tab.end());
  buf.push_back(0);
  out.k = k;
  out.max_nf = max_nf;
  out.max_nt = max_nt;
  out.any_table = any_table;
  out.all_affine = !any_table && max_nf <= 4 && max_nt <= 8;
  out.n_cols = 0;
  for (int j = 0; j < pl->n_ev; ++j) out.n_cols = std::max(out.n_cols, pl->ev_col[j] + 1);
  out.cols.assign(pl->ev_col, pl->ev_col + pl->n_ev);
  std::sort(out.cols.begin(), out.cols.end());
  out.cols.erase(std::unique(out.cols.begin(), out.cols.end()), out.cols.end());
  out.jit_src = any_table ? std::string() : rows_jit_source(pl);
  return PGM_OK;
}

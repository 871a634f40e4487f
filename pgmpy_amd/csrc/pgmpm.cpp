// pgmpm.cpp — the run-time half of the plan-specialised batched-BP steps (host code): the fused product +
// marginal, n-ary products, separator marginals and two-marginal passes of a batched calibration (pgmpy
// ExactInference.py:770-805), merged per dependency level into one launch, and the specialised contraction
// batches.  pgmpm_gen.cpp (host only, pgm_pm.h) plans a step, chooses its specialisation and writes the
// source; this unit compiles it for gfx950 (hipRTC, the on-disk code-object cache shared with the
// specialised row kernels of pgmrows.hip), keeps the loaded kernels, and binds and launches them.
// C-ABI: include/pgmhip.h (pgm_product_n_marginal_bind, pgm_pm_*), thin: plan -> specialise -> source -> bound.
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "pgm_hip_common.h"
#include "pgm_pm.h"

static std::mutex g_rtc_mu;  // PGM_RTC_SERIAL=1: one hipRTC compile at a time

// ----------------------------------------------------------------------------- code-object cache
// On-disk cache of specialised code objects: directory PGM_KERNEL_CACHE (default
// $XDG_CACHE_HOME/pgmpy_amd or ~/.cache/pgmpy_amd; "0" disables), one file per source hash holding
// the full source (compared on load, so a hash collision only misses) and the gfx950 code object.
static std::string rtc_cache_dir() {
  static const std::string dir = [] {
    const char *e = getenv("PGM_KERNEL_CACHE");
    if (e) return std::string(strcmp(e, "0") == 0 ? "" : e);
    const char *x = getenv("XDG_CACHE_HOME");
    if (x && *x) return std::string(x) + "/pgmpy_amd";
    const char *h = getenv("HOME");
    return h && *h ? std::string(h) + "/.cache/pgmpy_amd" : std::string();
  }();
  return dir;
}

static const char *const kRtcOpts[] = {"--offload-arch=gfx950", "-O3"};

// what else decides the code object besides the source: the hipRTC (compiler) version, the target
// and the options; folded into the cache key so an upgraded compiler never reuses an old object
static const std::string &rtc_toolchain_tag() {
  static const std::string tag = [] {
    int major = 0, minor = 0;
    if (hiprtcVersion(&major, &minor) != HIPRTC_SUCCESS) major = minor = -1;
    std::string t = "hiprtc " + std::to_string(major) + "." + std::to_string(minor);
    for (const char *o : kRtcOpts) t += std::string(" ") + o;
    return t;
  }();
  return tag;
}

static std::string rtc_cache_path(const std::string &src) {
  const std::string dir = rtc_cache_dir();
  if (dir.empty()) return dir;
  uint64_t h = 1469598103934665603ull;  // FNV-1a over the source, the toolchain tag and the ABI version
  for (unsigned char c : src) h = (h ^ c) * 1099511628211ull;
  for (unsigned char c : rtc_toolchain_tag()) h = (h ^ c) * 1099511628211ull;
  h = (h ^ (uint64_t)pgm_version()) * 1099511628211ull;
  char name[64];
  snprintf(name, sizeof name, "/k%016llx.co", (unsigned long long)h);
  return dir + name;
}

static bool rtc_cache_load(const std::string &path, const std::string &src, std::vector<char> &code) {
  if (path.empty()) return false;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  uint64_t n = 0, m = 0;
  bool ok = fread(&n, 8, 1, f) == 1 && n == src.size();
  std::string s2;
  if (ok) {
    s2.resize(n);
    ok = fread(&s2[0], 1, n, f) == n && s2 == src && fread(&m, 8, 1, f) == 1 && m > 0 && m < (1ull << 30);
  }
  if (ok) {
    code.resize(m);
    ok = fread(code.data(), 1, m, f) == m;
  }
  fclose(f);
  return ok;
}

static void rtc_cache_store(const std::string &path, const std::string &src, const std::vector<char> &code) {
  if (path.empty()) return;
  const std::string dir = path.substr(0, path.rfind('/'));
  // mkdir -p: create each component
  for (size_t i = 1; i <= dir.size(); ++i)
    if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
  const std::string tmp = path + ".tmp." + std::to_string((long long)getpid());
  FILE *f = fopen(tmp.c_str(), "wb");
  if (!f) return;
  const uint64_t n = src.size(), m = code.size();
  const bool ok = fwrite(&n, 8, 1, f) == 1 && fwrite(src.data(), 1, n, f) == n && fwrite(&m, 8, 1, f) == 1 &&
                  fwrite(code.data(), 1, m, f) == m;
  if (fclose(f) == 0 && ok) (void)rename(tmp.c_str(), path.c_str());
  else (void)remove(tmp.c_str());
}

// gfx950 code object of a specialised kernel source: the disk cache, else hipRTC (then cached)
bool pgmi_rtc_code(const std::string &src, const char *what, std::vector<char> &code) {
  const std::string path = rtc_cache_path(src);
  // the stored header holds the toolchain tag and the source; both must match on load
  const std::string keyed = rtc_toolchain_tag() + "\n" + src;
  if (rtc_cache_load(path, keyed, code)) return true;
  // hipRTC programs compile concurrently from several threads (pgm_pm_prepare); PGM_RTC_SERIAL=1
  // serialises every compile
  static const bool serial = getenv("PGM_RTC_SERIAL") && atoi(getenv("PGM_RTC_SERIAL")) != 0;
  std::unique_lock<std::mutex> lk(g_rtc_mu, std::defer_lock);
  if (serial) lk.lock();
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "pgm_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) return false;
  if (hiprtcCompileProgram(prog, (int)(sizeof kRtcOpts / sizeof kRtcOpts[0]), (const char **)kRtcOpts) != HIPRTC_SUCCESS) {
    size_t n = 0;
    hiprtcGetProgramLogSize(prog, &n);
    std::string log(n, '\0');
    if (n) hiprtcGetProgramLog(prog, &log[0]);
    fprintf(stderr, "pgmhip: %s did not compile (generic kernel used):\n%s\n", what, log.c_str());
    hiprtcDestroyProgram(&prog);
    return false;
  }
  size_t sz = 0;
  hiprtcGetCodeSize(prog, &sz);
  code.resize(sz);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);
  rtc_cache_store(path, keyed, code);
  return true;
}

// ----------------------------------------------------------------------------- bound launches
// a bound launch: one step, or several independent steps merged into one kernel (pgm_pm_merge:
// body i runs on blocks [start_i, start_i + total_i), starts padded to multiples of 8 so each body's
// XCD grouping holds)
struct PMBound {
  hipFunction_t fn = nullptr;  // compiled lazily: pgm_pm_prepare (in parallel) or the first run
  std::string src;
  unsigned blocks = 0;
  std::vector<PMSpec> specs;
  std::vector<const double *> ptrs;  // per body: its n_ops operands, then C, M
  unsigned threads = 256;  // workitems per workgroup (a specialised contraction chain: 1,024)
  // a contraction batch over the kernel-argument budget: its pointers in device memory, ptrs = {table}
  void *table = nullptr;
  PMBound() = default;
  PMBound(const PMBound &) = delete;
  PMBound &operator=(const PMBound &) = delete;
  ~PMBound() {
    if (table) (void)hipFree(table);
  }
};

// source -> loaded kernel and its code object (process lifetime; the code object is what a direct AQL
// dispatch loads into its own HSA executable, pgm_dq_bind_pm)
struct PMLoaded {
  std::string src;
  hipFunction_t fn;
  std::vector<char> code;
};
static std::mutex g_pm_mu;
static std::vector<PMLoaded> g_pm_cache;

static const PMLoaded *pm_entry(const std::string &src) {  // caller holds g_pm_mu
  for (auto &e : g_pm_cache)
    if (e.src == src) return &e;
  return nullptr;
}

static hipFunction_t pm_cached(const std::string &src) {  // caller holds g_pm_mu
  const PMLoaded *e = pm_entry(src);
  return e ? e->fn : nullptr;
}

static hipFunction_t pm_load(const std::string &src, const std::vector<char> &code) {  // caller holds g_pm_mu
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  if (hipModuleLoadData(&mod, code.data()) != hipSuccess || hipModuleGetFunction(&fn, mod, "pgm_pm") != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  g_pm_cache.push_back(PMLoaded{src, fn, code});
  return fn;
}

static hipFunction_t pm_compile(const std::string &src) {
  std::lock_guard<std::mutex> lk(g_pm_mu);
  if (hipFunction_t f = pm_cached(src)) return f;
  std::vector<char> code;
  if (!pgmi_rtc_code(src, "specialised product+marginal kernel", code)) return nullptr;
  return pm_load(src, code);
}

// compile every bound step's kernel that is not loaded yet: distinct sources on up to
// PGM_RTC_THREADS threads (default 1: hipRTC serialises compiles internally — pathfinder's 20 kernels
// take 2.5 s on 1 thread and 2.6 s on 16), then load the modules
static int pm_prepare(PMBound *const *bs, int n) {
  std::vector<std::string> todo;
  {
    std::lock_guard<std::mutex> lk(g_pm_mu);
    for (int i = 0; i < n; ++i) {
      if (!bs[i] || bs[i]->fn) continue;
      if (hipFunction_t f = pm_cached(bs[i]->src)) {
        bs[i]->fn = f;
        continue;
      }
      if (std::find(todo.begin(), todo.end(), bs[i]->src) == todo.end()) todo.push_back(bs[i]->src);
    }
  }
  if (!todo.empty()) {
    std::vector<std::vector<char>> codes(todo.size());
    std::vector<char> ok(todo.size(), 0);
    const char *te = getenv("PGM_RTC_THREADS");
    const size_t nt = std::max<size_t>(1, std::min<size_t>(todo.size(), te ? (size_t)atoi(te) : 1));
    std::atomic<size_t> next(0);
    auto work = [&] {
      for (size_t i; (i = next.fetch_add(1)) < todo.size();)
        ok[i] = pgmi_rtc_code(todo[i], "specialised product+marginal kernel", codes[i]) ? 1 : 0;
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    std::lock_guard<std::mutex> lk(g_pm_mu);
    for (size_t i = 0; i < todo.size(); ++i) {
      if (!ok[i] || (!pm_cached(todo[i]) && !pm_load(todo[i], codes[i])))
        return pgmi_failf(PGM_EDEVICE, "specialised product+marginal kernel: compile / load failed");
    }
    for (int i = 0; i < n; ++i)
      if (bs[i] && !bs[i]->fn) bs[i]->fn = pm_cached(bs[i]->src);
  }
  return PGM_OK;
}


// ============================================================================= C-ABI
extern "C" {

// PGM_PM_JIT=0 / PGM_NO_JIT keep the generic kernels (the specialised steps' reference path)
static bool pm_jit_on() {
  static const bool on = !getenv("PGM_NO_JIT") && (!getenv("PGM_PM_JIT") || atoi(getenv("PGM_PM_JIT")) != 0);
  return on;
}

// a bound launch of `src` (kernel pgm_pm, `blocks` workgroups) over the bodies `specs` and their pointers
static int pm_bound_new(const char *who, const std::string &src, uint64_t blocks, const std::vector<PMSpec> &specs,
                        const std::vector<const double *> &ptrs, void **bound) {
  PMBound *b = new (std::nothrow) PMBound;
  if (!b) return pgmi_failf(PGM_ENOMEM, "%s: out of host memory", who);
  b->src = src;
  b->blocks = (unsigned)blocks;
  b->specs = specs;
  b->ptrs = ptrs;
  *bound = b;
  return PGM_OK;
}

static int pm_bind(const pgm_productn_desc *d, const double *const *ops, double *C, const int64_t *marg_s,
                   int32_t reduce, double *M, void **bound, std::string *src_out, bool has_m = true) {
  *bound = nullptr;
  if (reduce != PGM_RED_SUM && reduce != PGM_RED_MAX)
    return pgmi_failf(PGM_EINVAL, "product_n_marginal: reduce must be PGM_RED_SUM or PGM_RED_MAX");
  ProdMK k;
  uint32_t g[3];
  const int r = pgmi_plan_product_marg(d, ops, C, marg_s, M, k, g);
  if (r < 0) return r;
  if (r == 0)
    return pgmi_failf(PGM_EINVAL, "product_n_marginal: shape not supported by the fused kernel "
                            "(pgm_product_n_marginal_ok is 0: run pgm_product_n + pgm_contract)");
  PMSpec sp;
  if (!pm_jit_on() || !pm_specialise(k, reduce, C != nullptr, has_m, sp)) return PGM_OK;  // *bound NULL: generic kernel
  std::vector<uint64_t> starts;
  uint64_t blocks = 0;
  const std::string src = pm_source({sp}, starts, &blocks);
  if (src_out) {
    *src_out = src;
    return PGM_OK;
  }
  std::vector<const double *> ptrs(k.ops, k.ops + k.n_ops);
  ptrs.push_back(C);
  ptrs.push_back(M);
  return pm_bound_new("product_n_marginal_bind", src, blocks, {sp}, ptrs, bound);
}

int pgm_product_n_marginal_bind(const pgm_productn_desc *d, const double *const *ops, double *C,
                                const int64_t *marg_s, int32_t reduce, double *M, void **bound) {
  STALE_PROBE();
  if (!bound) return pgmi_failf(PGM_EINVAL, "product_n_marginal_bind: null bound");
  return pm_bind(d, ops, C, marg_s, reduce, M, bound, nullptr);
}

int pgm_product_n_bind(const pgm_productn_desc *d, const double *const *ops, double *C, void **bound) {
  STALE_PROBE();
  if (!bound || !d || !C) return pgmi_failf(PGM_EINVAL, "product_n_bind: null argument");
  *bound = nullptr;
  if (d->n_keep < 1 || d->n_keep > PGM_MAX_DIMS) return pgmi_failf(PGM_EINVAL, "product_n_bind: n_keep out of range");
  // the product as a fused step whose every dim is kept (no reduced entries) and no marginal stored
  int64_t ms[PGM_MAX_DIMS];
  for (int i = 0; i < d->n_keep; ++i) ms[i] = d->keep_sc[i] ? d->keep_sc[i] : 1;
  ProdMK k;
  uint32_t g[3];
  const int r = pgmi_plan_product_marg(d, ops, C, ms, C, k, g);
  if (r <= 0) return r < 0 ? r : PGM_OK;  // shape not handled: *bound NULL, the generic kernel runs
  return pm_bind(d, ops, C, ms, PGM_RED_SUM, C, bound, nullptr, false);
}

int pgm_product_n_marginals_bind(const pgm_productn_desc *d, const double *const *ops, const int64_t *marg_s1,
                                 double *M1, const int64_t *marg_s2, double *M2, int32_t reduce, void **bound) {
  STALE_PROBE();
  if (!bound) return pgmi_failf(PGM_EINVAL, "product_n_marginals_bind: null bound");
  *bound = nullptr;
  if (reduce != PGM_RED_SUM && reduce != PGM_RED_MAX)
    return pgmi_failf(PGM_EINVAL, "product_n_marginals: reduce must be PGM_RED_SUM or PGM_RED_MAX");
  if (!pm_jit_on()) return PGM_OK;
  PMSpec sp;
  const int r = plan_two_marginals(d, ops, marg_s1, marg_s2, M1, M2, reduce, sp);
  if (r <= 0) return r;
  std::vector<uint64_t> starts;
  uint64_t blocks = 0;
  const std::string src = pm_source({sp}, starts, &blocks);
  std::vector<const double *> ptrs(ops, ops + d->n_ops);
  ptrs.push_back(M1);  // the C slot
  ptrs.push_back(M2);  // the M slot
  return pm_bound_new("product_n_marginals_bind", src, blocks, {sp}, ptrs, bound);
}

int pgm_product_n_marginal_source(const pgm_productn_desc *d, const double *const *ops, double *C,
                                  const int64_t *marg_s, int32_t reduce, double *M, char *buf, size_t len) {
  STALE_PROBE();
  if (!buf || len == 0) return pgmi_failf(PGM_EINVAL, "product_n_marginal_source: null buffer");
  void *unused = nullptr;
  std::string src;
  const int r = pm_bind(d, ops, C, marg_s, reduce, M, &unused, &src);
  if (r < 0) return r;
  const size_t n = std::min(len - 1, src.size());
  memcpy(buf, src.data(), n);
  buf[n] = 0;
  return (int)src.size();
}

int pgm_pm_bound_run(void *bound, void *stream) {
  STALE_PROBE();
  PMBound *b = (PMBound *)bound;
  if (!b) return pgmi_failf(PGM_EINVAL, "pm_bound_run: null bound");
  if (!b->fn) {
    const int r = pm_prepare(&b, 1);
    if (r != PGM_OK) return r;
  }
  size_t sz = b->ptrs.size() * sizeof(void *);
  void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, (void *)b->ptrs.data(), HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                   HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(b->fn, b->blocks, 1, 1, b->threads, 1, 1, 0, S(stream), nullptr, extra));
  return PGM_OK;
}

int pgm_pm_merge(void *const *bounds, int32_t n, void **merged) {
  STALE_PROBE();
  if (!bounds || !merged || n < 1 || n > kPmMaxBodies) return pgmi_failf(PGM_EINVAL, "pm_merge: 1..%d bound steps", kPmMaxBodies);
  *merged = nullptr;
  std::vector<PMSpec> specs;
  std::vector<const double *> ptrs;
  for (int i = 0; i < n; ++i) {
    const PMBound *b = (const PMBound *)bounds[i];
    if (!b) return pgmi_failf(PGM_EINVAL, "pm_merge: null bound %d", i);
    if (b->specs.empty()) return pgmi_failf(PGM_EINVAL, "pm_merge: bound %d is a specialised contraction batch", i);
    specs.insert(specs.end(), b->specs.begin(), b->specs.end());
    ptrs.insert(ptrs.end(), b->ptrs.begin(), b->ptrs.end());
  }
  if (specs.size() > (size_t)kPmMaxBodies) return pgmi_failf(PGM_EINVAL, "pm_merge: more than %d bodies", kPmMaxBodies);
  if (ptrs.size() > kPmMaxArgPtrs) return PGM_OK;  // kernel arguments over 4 KB: keep the separate launches
  std::vector<uint64_t> starts;
  uint64_t blocks = 0;
  const std::string src = pm_source(specs, starts, &blocks);
  if (blocks >= (1ull << 31)) return PGM_OK;  // too large for one grid: keep the separate launches
  return pm_bound_new("pm_merge", src, blocks, specs, ptrs, merged);
}

int pgm_pm_bound_source(void *bound, char *buf, size_t len) {
  STALE_PROBE();
  const PMBound *b = (const PMBound *)bound;
  if (!b || !buf || len == 0) return pgmi_failf(PGM_EINVAL, "pm_bound_source: null argument");
  const size_t n = std::min(len - 1, b->src.size());
  memcpy(buf, b->src.data(), n);
  buf[n] = 0;
  return (int)b->src.size();
}

int pgm_pm_prepare(void *const *bounds, int32_t n) {
  STALE_PROBE();
  if (!bounds || n < 0) return pgmi_failf(PGM_EINVAL, "pm_prepare: null bounds");
  return pm_prepare((PMBound *const *)bounds, n);
}

// a bound specialised launch as a direct AQL dispatch sees it (pgmdq.cpp): its code object, kernel name,
// grid and explicit argument segment (the flat pointer array)
int pgmi_pm_bound_jit(void *bound, pgmi_jit_launch *out) {
  PMBound *b = (PMBound *)bound;
  if (!b || !out) return pgmi_failf(PGM_EINVAL, "pm_bound_jit: null argument");
  if (!b->fn) {
    const int r = pm_prepare(&b, 1);
    if (r != PGM_OK) return r;
  }
  std::lock_guard<std::mutex> lk(g_pm_mu);
  const PMLoaded *e = pm_entry(b->src);
  if (!e || e->code.empty()) return pgmi_failf(PGM_EINVAL, "pm_bound_jit: no code object kept for this launch");
  out->code = e->code.data();
  out->code_size = e->code.size();
  out->kernel = "pgm_pm";
  out->args = b->ptrs.data();
  out->args_size = b->ptrs.size() * sizeof(void *);
  out->blocks = b->blocks;
  out->wg = b->threads;
  out->owner = b;
  out->write_through = 0;
  return PGM_OK;
}

int pgm_pm_bound_destroy(void *bound) {
  STALE_PROBE();
  delete (PMBound *)bound;
  return PGM_OK;
}

}  // extern "C"

// a plan-specialised kernel for a batch of contraction jobs (its source and geometry: cs_source), bound to its
// pointers; over the kernel-argument budget they go through a table in device memory
int pgmi_cs_bind(const pgmi_cs_job *jobs, int n, const uint32_t *level_off, int n_levels, int one_wg, void **bound) {
  *bound = nullptr;
  static const bool no_jit = getenv("PGM_NO_JIT") != nullptr;
  CSBatch cs;
  if (no_jit || !cs_source(jobs, n, level_off, n_levels, one_wg, cs)) return PGM_OK;
  const int r = pm_bound_new("batch_specialise", cs.src, cs.blocks, {}, cs.ptrs, bound);
  if (r != PGM_OK) return r;
  PMBound *b = (PMBound *)*bound;
  b->threads = cs.threads;
  if (cs.table) {
    const size_t bytes = b->ptrs.size() * sizeof(void *);
    hipError_t e = hipMalloc(&b->table, bytes);
    if (e == hipSuccess) e = hipMemcpy(b->table, b->ptrs.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      delete b;
      *bound = nullptr;
      return pgmi_failf(e == hipErrorOutOfMemory ? PGM_ENOMEM : PGM_EDEVICE, "batch_specialise: pointer table: %s",
                        hipGetErrorString(e));
    }
    b->ptrs.assign(1, (const double *)b->table);
  }
  return PGM_OK;
}

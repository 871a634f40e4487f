// plan_dev_selftest.cpp — the device side of a plan handle (pgmpy_amd/csrc/pgm_plan_dev.h) with stubbed
// device operations, on the CPU: first use, the lazy stages, the device change, a failure of every
// allocation and every copy of a build, zero-length sources and release.  Meant for a plain and for a
// sanitizer build:
//   c++ -std=c++17 -g [-fsanitize=address,undefined] -I pgmpy_amd/csrc tools/plan_dev_selftest.cpp -o plan_dev_selftest
// Exit status 0 and "plan_dev_selftest ok" when every check holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pgm_plan_dev.h"

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

// ---------------------------------------------------------------------------- the stubbed device
static int g_device = 0;
static int g_allocs = 0, g_frees = 0, g_copies = 0;
static int g_fail_alloc = 0, g_fail_copy = 0;  // k > 0: the k-th call from now fails (once)
static constexpr int kNoMem = 3, kDevice = 4;  // what PGM_ENOMEM / PGM_EDEVICE stand for here

static int stub_current(int *device) {
  *device = g_device;
  return 0;
}
// "device memory" is host memory (a leak or a double free shows under AddressSanitizer), tagged with the
// device it was allocated on
static int stub_alloc(void **p, size_t bytes) {
  if (g_fail_alloc > 0 && --g_fail_alloc == 0) return kNoMem;
  if (bytes == 0) return kDevice;  // a zero-byte request yields no pointer on a device
  int *base = (int *)malloc(sizeof(int64_t) + bytes);
  *base = g_device;
  *p = (char *)base + sizeof(int64_t);
  ++g_allocs;
  return 0;
}
static int stub_copy(void *dst, const void *src, size_t bytes) {
  if (g_fail_copy > 0 && --g_fail_copy == 0) return kDevice;
  memcpy(dst, src, bytes);
  ++g_copies;
  return 0;
}
static void stub_free(void *p) {
  free((char *)p - sizeof(int64_t));
  ++g_frees;
}
static const pgmdev::DevOps kStub = {stub_current, stub_alloc, stub_copy, stub_free};

static int device_of(const void *p) { return *(const int *)((const char *)p - sizeof(int64_t)); }

// ---------------------------------------------------------------------------- a handle like the library's
// three base slots (two uploads, one scratch) and two stages of two slots (an upload, a scratch) each
struct Handle {
  std::vector<int64_t> a{1, 2, 3};
  std::vector<int32_t> b{4, 5};
  std::vector<int64_t> s0{6, 7, 8, 9}, s1;  // stage 1 uploads an empty list
  pgmdev::PlanDev dev;
  const int64_t *d_a = nullptr;
  const int32_t *d_b = nullptr;
  uint8_t *d_buf = nullptr;
  const int64_t *d_s0 = nullptr, *d_s1 = nullptr;
  double *d_p0 = nullptr, *d_p1 = nullptr;

  int use(int stage = -1) {
    using pgmdev::scratch;
    using pgmdev::upload;
    const pgmdev::Slot base[] = {upload(d_a, a), upload(d_b, b), scratch(d_buf, 5)};
    if (stage == 0) {
      const pgmdev::Slot st[] = {upload(d_s0, s0), scratch(d_p0, 7)};
      return dev.use(kStub, base, 0, st);
    }
    if (stage == 1) {
      const pgmdev::Slot st[] = {upload(d_s1, s1), scratch(d_p1, 7)};
      return dev.use(kStub, base, 1, st);
    }
    return dev.use(kStub, base);
  }
  bool base_ok(int device) const {
    return dev.device() == device && dev.flag() && device_of(dev.flag()) == device && d_a && device_of(d_a) == device &&
           memcmp(d_a, a.data(), a.size() * sizeof(int64_t)) == 0 && d_b && memcmp(d_b, b.data(), b.size() * sizeof(int32_t)) == 0 &&
           d_buf && device_of(d_buf) == device;
  }
  bool stage0_ok(int device) const {
    return d_s0 && device_of(d_s0) == device && memcmp(d_s0, s0.data(), s0.size() * sizeof(int64_t)) == 0 && d_p0 &&
           device_of(d_p0) == device;
  }
  bool stage1_ok(int device) const { return d_s1 && device_of(d_s1) == device && d_p1 && device_of(d_p1) == device; }
  bool stage0_empty() const { return !d_s0 && !d_p0; }
  bool stage1_empty() const { return !d_s1 && !d_p1; }
  bool empty() const {
    return dev.device() == -1 && dev.owned() == 0 && !dev.flag() && !d_a && !d_b && !d_buf && stage0_empty() && stage1_empty();
  }
};

// what an undisturbed build does: the flag word + 3 slots, 2 copies; a stage: 2 slots, 1 copy (stage 1: none)
static constexpr int kBaseAllocs = 4, kBaseCopies = 2, kStageAllocs = 2;

static int test_first_use_and_stages() {
  g_device = 0;
  Handle h;
  CHECK(h.empty());
  const int a0 = g_allocs, f0 = g_frees, c0 = g_copies;
  CHECK(h.use() == 0 && h.base_ok(0));
  CHECK(g_allocs - a0 == kBaseAllocs && g_copies - c0 == kBaseCopies && g_frees == f0);
  CHECK(h.stage0_empty() && h.stage1_empty());
  CHECK(h.use() == 0 && g_allocs - a0 == kBaseAllocs && g_copies - c0 == kBaseCopies && g_frees == f0);  // no operation
  // a stage only when first asked for
  CHECK(h.use(1) == 0 && h.stage1_ok(0) && h.stage0_empty());
  CHECK(g_allocs - a0 == kBaseAllocs + kStageAllocs && g_copies - c0 == kBaseCopies);  // the empty list is not copied
  CHECK(h.use(1) == 0 && g_allocs - a0 == kBaseAllocs + kStageAllocs);
  CHECK(h.use(0) == 0 && h.stage0_ok(0) && h.stage1_ok(0) && h.base_ok(0));
  CHECK(g_allocs - a0 == kBaseAllocs + 2 * kStageAllocs && g_copies - c0 == kBaseCopies + 1 && g_frees == f0);
  CHECK(h.use(0) == 0 && h.use() == 0 && g_allocs - a0 == kBaseAllocs + 2 * kStageAllocs && g_copies - c0 == kBaseCopies + 1);
  // another device: everything is freed, stages included; the base is built there, a stage on its next ask
  g_device = 1;
  CHECK(h.use() == 0 && h.base_ok(1) && h.stage0_empty() && h.stage1_empty());
  CHECK(g_frees - f0 == kBaseAllocs + 2 * kStageAllocs && g_allocs - a0 == 2 * kBaseAllocs + 2 * kStageAllocs);
  CHECK(h.use(0) == 0 && h.stage0_ok(1) && h.stage1_empty());
  // and back, asking for a stage at once
  g_device = 0;
  CHECK(h.use(1) == 0 && h.base_ok(0) && h.stage1_ok(0) && h.stage0_empty());
  h.dev.release(kStub);
  CHECK(h.empty() && g_allocs - a0 == g_frees - f0);
  h.dev.release(kStub);  // twice
  CHECK(h.empty() && g_allocs - a0 == g_frees - f0);
  Handle never;
  never.dev.release(kStub);  // a handle that never touched a device
  CHECK(never.empty());
  return 0;
}

// fail allocation k, then copy k, for every k of the build of the base (stage -1) or of a stage over a built base
static int fail_each(int stage, int n_allocs, int n_copies) {
  for (int pass = 0; pass < 2; ++pass)
    for (int k = 1; k <= (pass == 0 ? n_allocs : n_copies); ++k) {
      g_device = 0;
      const int a0 = g_allocs, f0 = g_frees;
      {
        Handle h;
        if (stage >= 0) CHECK(h.use() == 0);
        const int before = g_allocs - g_frees;
        (pass == 0 ? g_fail_alloc : g_fail_copy) = k;
        CHECK(h.use(stage) == (pass == 0 ? kNoMem : kDevice));
        CHECK(g_fail_alloc == 0 && g_fail_copy == 0);
        // nothing of the failed group is left, what was built before it stays
        CHECK(g_allocs - g_frees == before);
        if (stage < 0) CHECK(h.empty());
        else CHECK(h.base_ok(0) && h.stage0_empty() && h.stage1_empty());
        // the next call starts the group over and ends as an undisturbed build does
        CHECK(h.use(stage) == 0 && h.base_ok(0));
        CHECK(stage != 0 || (h.stage0_ok(0) && h.stage1_empty()));
        CHECK(stage != 1 || (h.stage1_ok(0) && h.stage0_empty()));
        CHECK(h.dev.owned() == (size_t)(kBaseAllocs + (stage >= 0 ? kStageAllocs : 0)));
        h.dev.release(kStub);
        CHECK(h.empty());
      }
      CHECK(g_allocs - a0 == g_frees - f0);
    }
  return 0;
}

static int test_failures() {
  CHECK(!fail_each(-1, kBaseAllocs, kBaseCopies));
  CHECK(!fail_each(0, kStageAllocs, 1));
  CHECK(!fail_each(1, kStageAllocs, 0));
  // a failure while moving to another device leaves nothing on either; the next call builds there
  g_device = 0;
  Handle h;
  CHECK(h.use(0) == 0);
  g_device = 1;
  g_fail_alloc = 3;
  CHECK(h.use(0) == kNoMem && h.empty());
  CHECK(h.use(0) == 0 && h.base_ok(1) && h.stage0_ok(1));
  h.dev.release(kStub);
  return 0;
}

static int test_zero_length() {
  g_device = 0;
  Handle h;
  h.a.clear();
  CHECK(h.use(1) == 0);
  CHECK(h.d_a && h.d_s1 && device_of(h.d_a) == 0);  // valid allocations the kernels may be handed
  h.dev.release(kStub);
  return 0;
}

int main() {
  if (test_first_use_and_stages() || test_failures() || test_zero_length()) return 1;
  CHECK(g_allocs == g_frees && g_allocs > 0);
  printf("plan_dev_selftest ok\n");
  return 0;
}

// pgm_plan_dev.h — what a plan handle (FitHandle, SampleHandle, GibbsHandle) keeps on a device: the device
// it lives on, the allocations it owns, the one int32 flag word its kernels raise, and stages that only
// some entry points need.  Host-only bookkeeping without a HIP call of its own: asking for the current
// device, allocating, copying host to device and freeing are the caller's DevOps, so a stand-alone CPU
// program can exercise every path with stubs (tools/plan_dev_selftest.cpp).  The .hip units pass
// pgm_hip_common.h's kHipDevOps.
#pragma once

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

// internal to the library: nothing of it is in the dynamic symbol table
namespace pgmdev __attribute__((visibility("hidden"))) {

// every operation returns 0 or the status the entry point hands on (PGM_ENOMEM, PGM_EDEVICE)
struct DevOps {
  int (*current)(int *device);
  int (*alloc)(void **p, size_t bytes);
  int (*copy)(void *dst, const void *src, size_t bytes);  // host to device, complete on return
  void (*free)(void *p);
};

// one allocation and the handle's typed pointer that receives it; src == nullptr: scratch, not copied
struct Slot {
  void *field;
  void (*set)(void *field, void *p);
  const void *src;
  size_t bytes;
};
template <class T>
Slot scratch(T *&field, size_t count) {
  return {&field, [](void *f, void *p) { *static_cast<T **>(f) = static_cast<T *>(p); }, nullptr, count * sizeof(T)};
}
// the upload of a host vector (an empty one still gets an allocation: the kernels take the pointer)
template <class T>
Slot upload(const T *&field, const std::vector<T> &src) {
  Slot s = scratch(field, src.size());
  s.src = src.data();
  return s;
}
struct Slots {
  const Slot *p = nullptr;
  size_t n = 0;
  Slots() = default;
  template <size_t N>
  Slots(const Slot (&a)[N]) : p(a), n(N) {}
};

// The base (the descriptors every launch reads, and the flag word) is built by the first use() on the
// current device; a use() on another device releases everything, stages included, and builds the base
// there.  Stage k is built by the first use() that asks for it, on the device of the base.  A group (the
// base or a stage) counts as built only once its last copy succeeded: a failure frees what the group had
// allocated so far and clears its pointers, and the next use() starts that group over.  An allocation is
// on the owned list from the moment it exists, so release() reaches it whatever happened since.
class PlanDev {
 public:
  static constexpr int kStages = 3;

  // the base, and stage k of it when k >= 0, on the current device; 0, or the failed operation's status
  int use(const DevOps &ops, Slots base, int k = -1, Slots stage = Slots()) {
    int dev = 0;
    if (const int st = ops.current(&dev)) return st;
    std::lock_guard<std::mutex> lk(mu_);
    if (device_ != dev) {
      release_locked(ops);
      const Slot flag[] = {scratch(flag_, 1)};
      if (const int st = build(ops, -1, flag)) return st;
      if (const int st = build(ops, -1, base)) return st;
      device_ = dev;
    }
    if (k < 0 || built_[k]) return 0;
    if (const int st = build(ops, k, stage)) return st;
    built_[k] = true;
    return 0;
  }

  // free everything; harmless on a handle that never touched a device, and twice
  void release(const DevOps &ops) {
    std::lock_guard<std::mutex> lk(mu_);
    release_locked(ops);
  }

  int device() const { return device_; }  // -1: nothing uploaded
  int32_t *flag() const { return flag_; }
  size_t owned() const { return owned_.size(); }

 private:
  struct Owned {
    void *p;
    int group;  // -1: the base; else the stage
    void *field;
    void (*set)(void *field, void *p);
  };

  // allocate every slot, then copy every source; on a failure the whole group is dropped
  int build(const DevOps &ops, int group, Slots slots) {
    for (size_t i = 0; i < slots.n; ++i) {
      const Slot &s = slots.p[i];
      void *p = nullptr;
      if (const int st = ops.alloc(&p, s.bytes ? s.bytes : 1)) {
        drop(ops, group);
        return st;
      }
      owned_.push_back(Owned{p, group, s.field, s.set});
      s.set(s.field, p);
    }
    for (size_t i = 0; i < slots.n; ++i) {
      const Slot &s = slots.p[i];
      if (!s.src || !s.bytes) continue;
      void *dst = owned_[owned_.size() - slots.n + i].p;
      if (const int st = ops.copy(dst, s.src, s.bytes)) {
        drop(ops, group);
        return st;
      }
    }
    return 0;
  }

  void drop(const DevOps &ops, int group) {
    size_t kept = 0;
    for (const Owned &o : owned_) {
      if (o.group != group) {
        owned_[kept++] = o;
        continue;
      }
      ops.free(o.p);
      o.set(o.field, nullptr);
    }
    owned_.resize(kept);
  }

  void release_locked(const DevOps &ops) {
    for (int g = -1; g < kStages; ++g) drop(ops, g);
    for (bool &b : built_) b = false;
    device_ = -1;
  }

  std::mutex mu_;
  int device_ = -1;
  int32_t *flag_ = nullptr;
  bool built_[kStages] = {};
  std::vector<Owned> owned_;
};

}  // namespace pgmdev

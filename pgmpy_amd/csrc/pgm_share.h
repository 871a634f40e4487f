// pgm_share.h — what direct launches of one plan share (pgmdq.cpp): the loaded code object and the
// memory their kernarg segments are carved from.  Host-only bookkeeping without a HIP or HSA call of its
// own: loading, unloading and allocating are the caller's callbacks, so a stand-alone CPU program can
// exercise both classes with stubs (tools/share_selftest.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <list>
#include <mutex>
#include <vector>

namespace pgmshare {

// FNV-1a, 64 bit
inline uint64_t content_hash(const void *p, size_t n) {
  const unsigned char *b = (const unsigned char *)p;
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

// One loaded value (an HSA executable) per (agent, code-object size, content hash), reference counted.
// The entry owns a copy of the blob: the loader reads from it for as long as the value lives (the plan
// that brought the blob may be destroyed while another plan with the same code still holds the entry),
// and a hit is confirmed byte for byte, so a hash collision loads a second entry and never aliases two
// different code objects.  Never keyed by a plan pointer, which the allocator reuses.
template <class T>
class CodeRegistry {
 public:
  struct Entry {
    uint64_t agent = 0, hash = 0;
    std::vector<char> blob;
    int refs = 0;
    T value{};
  };

  // the entry for (agent, blob), loaded with load(entry) -> 0 on success on a miss; *loaded tells which.
  // Loads are serialised with every other acquire and release.
  template <class Load>
  int acquire(uint64_t agent, const void *blob, size_t n, Load load, Entry **out, bool *loaded = nullptr) {
    const uint64_t h = content_hash(blob, n);
    std::lock_guard<std::mutex> lk(mu_);
    for (Entry &e : entries_)
      if (e.agent == agent && e.hash == h && e.blob.size() == n && memcmp(e.blob.data(), blob, n) == 0) {
        ++e.refs;
        *out = &e;
        if (loaded) *loaded = false;
        return 0;
      }
    entries_.emplace_back();
    Entry &e = entries_.back();
    e.agent = agent;
    e.hash = h;
    e.blob.assign((const char *)blob, (const char *)blob + n);
    const int rc = load(e);
    if (rc != 0) {
      entries_.pop_back();
      return rc;
    }
    e.refs = 1;
    *out = &e;
    if (loaded) *loaded = true;
    return 0;
  }

  // drop one reference; the last one calls unload(entry) and forgets the entry (returns true)
  template <class Unload>
  bool release(Entry *e, Unload unload) {
    std::lock_guard<std::mutex> lk(mu_);
    if (--e->refs > 0) return false;
    unload(*e);
    for (auto it = entries_.begin(); it != entries_.end(); ++it)
      if (&*it == e) {
        entries_.erase(it);
        break;
      }
    return true;
  }

  int refs(const Entry *e) {
    std::lock_guard<std::mutex> lk(mu_);
    return e->refs;
  }

  size_t size() {
    std::lock_guard<std::mutex> lk(mu_);
    return entries_.size();
  }

  // for an entry's own lazily filled members (its kernel symbol cache)
  std::mutex &mutex() { return mu_; }

 private:
  std::mutex mu_;
  std::list<Entry> entries_;  // stable addresses
};

// Kernarg segments as runs of 256-byte slots carved from chunks of at least 64 KiB.  A request takes the
// lowest free run that fits (so a freed slot is the next one handed out, and the segments of launches
// bound together lie side by side); when none fits the slab grows by one whole chunk from alloc(bytes).
// Chunks stay for the life of the slab.  Not thread safe: the caller locks.
class KernargSlab {
 public:
  static constexpr size_t kSlot = 256, kChunk = 64 * 1024;

  template <class Alloc>
  void *take(size_t bytes, Alloc alloc) {
    const size_t need = bytes ? (bytes + kSlot - 1) / kSlot : 1;
    for (Chunk &c : chunks_) {
      const size_t at = c.find(need);
      if (at != kNone) return c.mark(at, need, true);
    }
    const size_t slots = need > kChunk / kSlot ? need : kChunk / kSlot;
    void *base = alloc(slots * kSlot);
    if (!base) return nullptr;
    chunks_.push_back(Chunk{(char *)base, std::vector<uint8_t>(slots, 0)});
    return chunks_.back().mark(0, need, true);
  }

  // give back what take(bytes) returned; false when p is not a segment of this slab
  bool give(void *p, size_t bytes) {
    const size_t need = bytes ? (bytes + kSlot - 1) / kSlot : 1;
    for (Chunk &c : chunks_) {
      if ((char *)p < c.base || (char *)p >= c.base + c.used.size() * kSlot) continue;
      const size_t at = (size_t)((char *)p - c.base) / kSlot;
      if ((size_t)((char *)p - c.base) % kSlot || at + need > c.used.size()) return false;
      for (size_t i = at; i < at + need; ++i)
        if (!c.used[i]) return false;
      c.mark(at, need, false);
      return true;
    }
    return false;
  }

  size_t chunks() const { return chunks_.size(); }

  size_t slots_in_use() const {
    size_t n = 0;
    for (const Chunk &c : chunks_)
      for (uint8_t u : c.used) n += u;
    return n;
  }

  // hand every chunk to free_chunk(base) and forget it (a caller that owns plain host memory)
  template <class Free>
  void drop_chunks(Free free_chunk) {
    for (Chunk &c : chunks_) free_chunk((void *)c.base);
    chunks_.clear();
  }

 private:
  static constexpr size_t kNone = (size_t)-1;
  struct Chunk {
    char *base;
    std::vector<uint8_t> used;  // per slot
    size_t find(size_t need) const {
      size_t run = 0;
      for (size_t i = 0; i < used.size(); ++i) {
        run = used[i] ? 0 : run + 1;
        if (run == need) return i + 1 - need;
      }
      return kNone;
    }
    void *mark(size_t at, size_t need, bool on) {
      for (size_t i = at; i < at + need; ++i) used[i] = on ? 1 : 0;
      return base + at * kSlot;
    }
  };
  std::vector<Chunk> chunks_;
};

}  // namespace pgmshare

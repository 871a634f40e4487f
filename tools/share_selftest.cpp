// share_selftest.cpp — the code-object registry and the kernarg slab (pgmpy_amd/csrc/pgm_share.h) with
// stubbed load / unload / allocate callbacks, on the CPU.  Meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I pgmpy_amd/csrc tools/share_selftest.cpp -o share_selftest
// Exit status 0 and "share_selftest ok" when every check holds.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "pgm_share.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

struct Fake {
  int *live = nullptr;  // stands for the executable: leaks under ASan unless unloaded
};

static int loads = 0, unloads = 0;

static int run() {
  using Reg = pgmshare::CodeRegistry<Fake>;
  Reg reg;
  auto load = [](Reg::Entry &e) {
    e.value.live = new int((int)e.blob.size());
    ++loads;
    return 0;
  };
  auto unload = [](Reg::Entry &e) {
    delete e.value.live;
    e.value.live = nullptr;
    ++unloads;
  };
  std::string a(33000, 'a'), b(33000, 'a');
  b[17000] = 'b';
  Reg::Entry *e1 = nullptr, *e2 = nullptr, *e3 = nullptr, *e4 = nullptr;
  bool fresh = false;
  {
    std::string tmp = a;  // the caller's blob may go away: the entry keeps its own copy
    CHECK(reg.acquire(1, tmp.data(), tmp.size(), load, &e1, &fresh) == 0 && fresh);
  }
  CHECK(reg.acquire(1, a.data(), a.size(), load, &e2, &fresh) == 0 && !fresh && e2 == e1);
  CHECK(reg.refs(e1) == 2 && loads == 1);
  CHECK(reg.acquire(1, b.data(), b.size(), load, &e3, &fresh) == 0 && fresh && e3 != e1);  // same size, other bytes
  CHECK(reg.acquire(2, a.data(), a.size(), load, &e4, &fresh) == 0 && fresh && e4 != e1);  // other agent
  CHECK(reg.size() == 3 && loads == 3);
  CHECK(e1->blob == std::vector<char>(a.begin(), a.end()));
  CHECK(!reg.release(e1, unload) && unloads == 0);
  CHECK(reg.release(e2, unload) && unloads == 1 && reg.size() == 2);
  CHECK(reg.acquire(1, a.data(), a.size(), load, &e1, &fresh) == 0 && fresh && loads == 4);  // loads again
  Reg::Entry *bad = nullptr;
  CHECK(reg.acquire(3, a.data(), a.size(), [](Reg::Entry &) { return 7; }, &bad) == 7 && bad == nullptr);
  CHECK(reg.size() == 3);
  // concurrent binds and destroys of one blob: one entry at a time, every load unloaded
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; ++t)
    ts.emplace_back([&] {
      for (int i = 0; i < 200; ++i) {
        Reg::Entry *e = nullptr;
        if (reg.acquire(9, b.data(), b.size(), load, &e) == 0) reg.release(e, unload);
      }
    });
  for (auto &t : ts) t.join();
  CHECK(reg.release(e1, unload) && reg.release(e3, unload) && reg.release(e4, unload));
  CHECK(reg.size() == 0 && loads == unloads);

  pgmshare::KernargSlab slab;
  size_t allocs = 0, asked = 0;
  auto alloc = [&](size_t n) {
    ++allocs;
    asked = n;
    return malloc(n);
  };
  std::vector<char *> p;
  for (int i = 0; i < 256; ++i) p.push_back((char *)slab.take(256, alloc));
  CHECK(allocs == 1 && asked == 64 * 1024 && slab.chunks() == 1 && slab.slots_in_use() == 256);
  for (int i = 1; i < 256; ++i) CHECK(p[i] == p[0] + 256 * i);
  for (int i = 0; i < 256; ++i) memset(p[i], i, 256);  // every slot writable, none past the chunk
  char *q = (char *)slab.take(84, alloc);  // the chunk is full: grows by one chunk
  CHECK(q && allocs == 2 && slab.chunks() == 2);
  CHECK(slab.give(p[5], 256) && slab.give(p[6], 256) && slab.give(p[9], 256));
  CHECK(!slab.give(p[5], 256));       // not twice
  CHECK(!slab.give(p[7] + 8, 256));   // not a slot
  CHECK(slab.take(512, alloc) == p[5]);  // a run of two: the lowest that fits
  CHECK(slab.take(256, alloc) == p[9]);  // a freed slot is reused
  char *big = (char *)slab.take(100 * 1024, alloc);  // larger than a chunk: a chunk of its own size
  CHECK(big && allocs == 3 && asked == 100 * 1024);
  memset(big, 1, 100 * 1024);
  CHECK(slab.give(big, 100 * 1024) && slab.take(256, alloc) == q + 256);
  slab.drop_chunks([](void *c) { free(c); });
  CHECK(slab.chunks() == 0);
  return 0;
}

int main() {
  const int rc = run();
  if (rc == 0) puts("share_selftest ok");
  return rc;
}

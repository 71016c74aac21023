// Stand-alone driver for demodel_amd/csrc/resource_cache.h with malloc/free
// callbacks.  Built and run by test_resource_cache_host.py under
// AddressSanitizer+UBSan and under ThreadSanitizer; exits 0 when every
// check holds, prints the failed check and exits 1 otherwise.

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "resource_cache.h"

using demodel::CacheStats;
using demodel::ResourceCache;
using demodel::round_up_size_class;

static int g_failed = 0;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__,      \
                   __LINE__, #cond);                                  \
      g_failed = 1;                                                   \
    }                                                                 \
  } while (0)

static const uint64_t MiB = 1ull << 20;

// every block the callbacks have handed out and not yet taken back
static std::mutex g_mu;
static std::set<void*> g_allocated;
static std::atomic<uint64_t> g_allocs{0}, g_frees{0};

static void* do_alloc(int, uint64_t size_class) {
  void* p = std::malloc(size_class ? size_class : 1);
  std::memset(p, 0, size_class < 64 ? size_class : 64);
  std::lock_guard<std::mutex> g(g_mu);
  if (!g_allocated.insert(p).second) g_failed = 1;
  ++g_allocs;
  return p;
}

static void do_free(int, uint64_t, void* p) {
  {
    std::lock_guard<std::mutex> g(g_mu);
    if (g_allocated.erase(p) != 1) {  // double free or foreign block
      std::fprintf(stderr, "free of a block that is not out\n");
      g_failed = 1;
      return;
    }
    ++g_frees;
  }
  std::free(p);
}

static size_t outstanding() {
  std::lock_guard<std::mutex> g(g_mu);
  return g_allocated.size();
}

static void test_rounding() {
  const uint64_t G = 2 * MiB;
  CHECK(round_up_size_class(1, G) == G);
  CHECK(round_up_size_class(G, G) == G);
  CHECK(round_up_size_class(G + 1, G) == 2 * G);
  CHECK(round_up_size_class(32 * MiB, G) == 32 * MiB);
  CHECK(round_up_size_class(32 * MiB - 13, G) == 32 * MiB);
  CHECK(round_up_size_class(0, G) == G);
  CHECK(round_up_size_class(12345, 0) == 12345);
}

static void test_hit_miss_accounting() {
  ResourceCache<void*> c(do_alloc, do_free, 64 * MiB);
  const uint64_t G = 2 * MiB;
  // two requests of different sizes in the same class share a free list
  uint64_t k1 = round_up_size_class(3 * MiB, G);
  uint64_t k2 = round_up_size_class(4 * MiB - 5, G);
  CHECK(k1 == k2 && k1 == 4 * MiB);
  void* a = c.take(0, k1, k1);
  CacheStats s = c.stats();
  CHECK(s.hits == 0 && s.misses == 1);
  CHECK(s.bytes_live == k1 && s.bytes_cached == 0);
  CHECK(c.release(0, k1, k1, a));
  s = c.stats();
  CHECK(s.bytes_live == 0 && s.bytes_cached == k1);
  void* b = c.take(0, k2, k2);
  CHECK(b == a);  // the same block comes back
  s = c.stats();
  CHECK(s.hits == 1 && s.misses == 1);
  CHECK(s.bytes_live == k1 && s.bytes_cached == 0);
  // another class and another device both miss
  void* d = c.take(0, 2 * MiB, 2 * MiB);
  void* e = c.take(1, k1, k1);
  s = c.stats();
  CHECK(s.hits == 1 && s.misses == 3);
  CHECK(s.bytes_live == 2 * k1 + 2 * MiB);
  c.release(0, k2, k2, b);
  c.release(0, 2 * MiB, 2 * MiB, d);
  c.release(1, k1, k1, e);
  // device 1's block is not handed to device 0
  void* f = c.take(0, k1, k1);
  CHECK(f == b);
  c.release(0, k1, k1, f);
  // a block released as not reusable is freed, never cached
  void* g = c.take(0, 6 * MiB, 6 * MiB);
  uint64_t frees = g_frees;
  CHECK(!c.release(0, 6 * MiB, 6 * MiB, g, false));
  CHECK(g_frees == frees + 1);
  s = c.stats();
  CHECK(s.bytes_live == 0);
  CHECK(s.bytes_cached == 2 * k1 + 2 * MiB);
  CHECK(c.trim() == 2 * k1 + 2 * MiB);
  CHECK(outstanding() == 0);
}

static void test_cap() {
  const uint64_t S = 4 * MiB;
  {
    ResourceCache<void*> c(do_alloc, do_free, 2 * S);
    void* p[3];
    for (auto& x : p) x = c.take(0, S, S);
    CHECK(c.release(0, S, S, p[0]));
    CHECK(c.release(0, S, S, p[1]));
    uint64_t frees = g_frees;
    CHECK(!c.release(0, S, S, p[2]));  // over the cap: freed
    CHECK(g_frees == frees + 1);
    CacheStats s = c.stats();
    CHECK(s.bytes_cached == 2 * S && s.bytes_live == 0 && s.freed == 1);
    CHECK(s.cap_bytes == 2 * S);
    CHECK(outstanding() == 2);
    c.trim();
  }
  {
    ResourceCache<void*> c(do_alloc, do_free, 0);  // cap 0 never caches
    for (int i = 0; i < 4; i++) {
      void* x = c.take(0, S, S);
      CHECK(!c.release(0, S, S, x));
      CHECK(outstanding() == 0);
    }
    CacheStats s = c.stats();
    CHECK(s.hits == 0 && s.misses == 4 && s.bytes_cached == 0);
    CHECK(s.freed == 4 && s.bytes_live == 0);
    CHECK(c.trim() == 0);
  }
  CHECK(outstanding() == 0);
}

static void test_trim() {
  const uint64_t S = 2 * MiB;
  ResourceCache<void*> c(do_alloc, do_free, 64 * MiB);
  void* a = c.take(0, S, S);
  void* b = c.take(0, S, S);
  void* d = c.take(2, 2 * S, 2 * S);
  c.release(0, S, S, a);
  c.release(2, 2 * S, 2 * S, d);
  CHECK(outstanding() == 3);
  CHECK(c.trim() == 3 * S);  // only idle blocks go; b is still live
  CHECK(outstanding() == 1);
  CacheStats s = c.stats();
  CHECK(s.bytes_cached == 0 && s.bytes_live == S);
  void* e = c.take(0, S, S);  // a miss again after the trim
  s = c.stats();
  CHECK(s.misses == 4 && s.hits == 0);
  c.release(0, S, S, b);
  c.release(0, S, S, e);
  CHECK(c.trim() == 2 * S);
  CHECK(c.trim() == 0);
  CHECK(outstanding() == 0);
}

// 8 threads x 1000 mixed cycles.  Each held block carries its owner's tag;
// a block handed to two owners at once shows as a clobbered tag (and as a
// data race under ThreadSanitizer), a lost block as a leak at the end.
static void test_threads() {
  const int T = 8, N = 1000;
  const uint64_t classes[3] = {64, 256, 1024};
  // cap between one and all threads' worth, so both paths of release run
  ResourceCache<void*> c(do_alloc, do_free, 6 * 1024);
  std::atomic<int> bad{0};
  const uint64_t allocs0 = g_allocs;
  struct Held {
    void* p;
    uint64_t k;
    int dev;
  };
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++) {
    th.emplace_back([&, t] {
      unsigned seed = 12345u + 977u * (unsigned)t;
      std::vector<Held> held;
      for (int i = 0; i < N; i++) {
        seed = seed * 1664525u + 1013904223u;
        unsigned r = seed >> 16;
        if (held.size() < 4 && (held.empty() || (r & 1))) {
          uint64_t k = classes[(r >> 1) % 3];
          int dev = (int)((r >> 3) & 1);
          void* p = c.take(dev, k, k);
          uint64_t tag = ((uint64_t)(t + 1) << 32) | (unsigned)i;
          std::memcpy(p, &tag, sizeof tag);
          std::memcpy((char*)p + k - sizeof tag, &tag, sizeof tag);
          held.push_back({p, k, dev});
        } else {
          size_t j = (r >> 1) % held.size();
          void* p = held[j].p;
          uint64_t k = held[j].k;
          int dev = held[j].dev;
          uint64_t t0, t1;
          std::memcpy(&t0, p, sizeof t0);
          std::memcpy(&t1, (char*)p + k - sizeof t1, sizeof t1);
          if (t0 != t1 || (t0 >> 32) != (uint64_t)(t + 1)) ++bad;
          held.erase(held.begin() + (long)j);
          c.release(dev, k, k, p, (r & 0x700) != 0);  // 1 in 8 not reusable
        }
      }
      for (auto& h : held) c.release(h.dev, h.k, h.k, h.p);
    });
  }
  for (auto& x : th) x.join();
  CHECK(bad == 0);
  CacheStats s = c.stats();
  CHECK(s.bytes_live == 0);
  CHECK(s.bytes_cached <= 6 * 1024);
  CHECK(s.misses == g_allocs - allocs0);  // one allocation per miss
  CHECK(s.hits > 0);
  // blocks still out == blocks idle in the cache: none lost, none doubled
  uint64_t idle_blocks = outstanding();
  uint64_t bytes = c.trim();
  CHECK(bytes == s.bytes_cached);
  CHECK(outstanding() == 0);
  CHECK(idle_blocks > 0);
  s = c.stats();
  CHECK(s.bytes_cached == 0 && s.bytes_live == 0);
}

int main() {
  test_rounding();
  test_hit_miss_accounting();
  test_cap();
  test_trim();
  uint64_t a0 = g_allocs, f0 = g_frees;
  CHECK(a0 == f0);
  test_threads();
  CHECK(g_allocs == g_frees);  // every allocated block was freed once
  CHECK(outstanding() == 0);
  if (g_failed) return 1;
  std::puts("resource_cache OK");
  return 0;
}

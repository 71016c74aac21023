// Thread-safe free-list cache for expensive runtime resources (pinned host
// slabs, streams, events).  Host-only: no HIP includes, so it compiles and
// is tested with a plain C++ compiler; hip_core.cpp supplies the allocate
// and free callbacks.
//
// Resources are keyed by (device, size class).  `cost` is what one resource
// of a class counts against the byte cap: the class itself for memory, 1 for
// handles such as streams and events.
//
// Contract for callers: release() a resource only when nothing on the GPU
// still uses it.  A resource whose state is in doubt is released with
// reusable=false and is freed instead of cached.

#pragma once

#include <cstdint>
#include <functional>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace demodel {

inline uint64_t round_up_size_class(uint64_t nbytes, uint64_t granule) {
  if (granule == 0) return nbytes;
  if (nbytes == 0) return granule;
  return (nbytes + granule - 1) / granule * granule;
}

struct CacheStats {
  uint64_t hits = 0;          // take() served from the free list
  uint64_t misses = 0;        // take() that had to allocate
  uint64_t bytes_cached = 0;  // idle in the free lists
  uint64_t bytes_live = 0;    // handed out and not yet released
  uint64_t freed = 0;         // released resources that were not kept
  uint64_t cap_bytes = 0;
};

template <class Handle>
class ResourceCache {
 public:
  using AllocFn = std::function<Handle(int device, uint64_t size_class)>;
  using FreeFn = std::function<void(int device, uint64_t size_class, Handle)>;

  ResourceCache(AllocFn alloc, FreeFn free_fn, uint64_t cap_bytes)
      : alloc_(std::move(alloc)), free_(std::move(free_fn)), cap_(cap_bytes) {}

  // Never frees what it still holds: process-lifetime caches are leaked on
  // purpose (the runtime may be gone by static-destruction time); others
  // call trim() first.
  ~ResourceCache() = default;
  ResourceCache(const ResourceCache&) = delete;
  ResourceCache& operator=(const ResourceCache&) = delete;

  // A cached resource of this class, or a fresh one.  The allocate callback
  // runs outside the lock and may throw; nothing is accounted then.
  Handle take(int device, uint64_t size_class, uint64_t cost) {
    {
      std::lock_guard<std::mutex> g(mu_);
      auto it = free_lists_.find(Key(device, size_class));
      if (it != free_lists_.end() && !it->second.empty()) {
        Handle h = it->second.back();
        it->second.pop_back();
        ++stats_.hits;
        stats_.bytes_cached -= cost;
        stats_.bytes_live += cost;
        return h;
      }
    }
    Handle h = alloc_(device, size_class);
    std::lock_guard<std::mutex> g(mu_);
    ++stats_.misses;
    stats_.bytes_live += cost;
    return h;
  }

  // Hand a resource back.  It is cached when reusable and under the cap,
  // and freed otherwise.  Returns true when it was cached.
  bool release(int device, uint64_t size_class, uint64_t cost, Handle h,
               bool reusable = true) {
    {
      std::lock_guard<std::mutex> g(mu_);
      stats_.bytes_live -= cost;
      if (reusable && cap_ > 0 && stats_.bytes_cached + cost <= cap_) {
        free_lists_[Key(device, size_class)].push_back(h);
        stats_.bytes_cached += cost;
        return true;
      }
      ++stats_.freed;
    }
    free_(device, size_class, h);
    return false;
  }

  // Free everything idle; returns the bytes let go.
  uint64_t trim() {
    std::map<Key, std::vector<Handle>> drop;
    uint64_t bytes;
    {
      std::lock_guard<std::mutex> g(mu_);
      drop.swap(free_lists_);
      bytes = stats_.bytes_cached;
      stats_.bytes_cached = 0;
    }
    for (auto& kv : drop)
      for (Handle h : kv.second) {
        free_(kv.first.first, kv.first.second, h);
        std::lock_guard<std::mutex> g(mu_);
        ++stats_.freed;
      }
    return bytes;
  }

  void set_cap(uint64_t cap_bytes) {
    std::lock_guard<std::mutex> g(mu_);
    cap_ = cap_bytes;
  }

  uint64_t cap() const {
    std::lock_guard<std::mutex> g(mu_);
    return cap_;
  }

  CacheStats stats() const {
    std::lock_guard<std::mutex> g(mu_);
    CacheStats s = stats_;
    s.cap_bytes = cap_;
    return s;
  }

 private:
  using Key = std::pair<int, uint64_t>;

  AllocFn alloc_;
  FreeFn free_;
  mutable std::mutex mu_;
  uint64_t cap_;
  std::map<Key, std::vector<Handle>> free_lists_;
  CacheStats stats_;
};

}  // namespace demodel

// demodel_amd._hip — the MI355X landing-pipeline runtime.
//
// Native equivalent of the data plane the reference left inside goproxy's
// io.Copy loop (reference cmd/demodel/start.go:201-204; SURVEY.md §3.2 "HOT
// LOOP"), rebuilt for MI355X: pinned host ring slabs, hipMemcpyAsync on side
// streams, HIP events, a socket->ring->HBM landing loop that bypasses Python
// (PinnedPool::land_fd over csrc/sock_io.h), and DLPack
// export so landed HBM blobs become zero-copy torch tensors.
//
// Deliberately torch-header-free: every API takes raw pointers/handles, so
// the extension cross-compiles in seconds and has no ABI coupling.

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime.h>

#include <sys/socket.h>
#include <sys/types.h>
#include <unistd.h>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "resource_cache.h"
#include "sock_io.h"

namespace py = pybind11;

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) {                                                 \
      throw std::runtime_error(std::string("HIP error at " #expr ": ") +    \
                               hipGetErrorString(_e));                      \
    }                                                                       \
  } while (0)

// ------------------------------------------------------------------------
// kernels (defined in the .hip translation units)

extern "C" {
void launch_sha256_batch(const void* data, size_t nbytes, size_t chunk_bytes,
                         uint32_t* out_digests, int n_chunks,
                         hipStream_t stream);
void launch_sha256_chain_init(uint32_t* state, hipStream_t stream);
void launch_sha256_chain_update(uint32_t* state, const void* data,
                                size_t nblocks, hipStream_t stream);
void launch_scatter_ranges(const void* src, const uint64_t* desc,
                           int n_desc, hipStream_t stream);
void launch_cast_f32_to_bf16(const float* src, uint16_t* dst, size_t n,
                             hipStream_t stream);
void launch_fp8_block_dequant(const void* src_fp8, const void* scale,
                              int scale_dtype, void* dst, int dst_dtype,
                              int64_t rows, int64_t cols, int64_t block_rows,
                              int64_t block_cols, hipStream_t stream);
void fp8_block_dequant_pass_limits(int64_t* out);
void launch_gguf_dequant(int qtype, const void* src, uint16_t* dst_bf16,
                         int64_t n_blocks, hipStream_t stream);
void launch_inflate_streams(const uint64_t* desc, int n_streams,
                            hipStream_t stream);
void launch_zstd_frames(const uint64_t* desc, int n_frames,
                        hipStream_t stream, int window);
void launch_snappy_streams(const uint64_t* desc, int n_streams,
                           hipStream_t stream);
void launch_lz4_streams(const uint64_t* desc, int n_streams,
                        hipStream_t stream);
void launch_parquet_decode(const uint64_t* desc, int n_pages,
                           hipStream_t stream, int max_blocks);
void launch_parquet_hybrid(const uint64_t* desc, int n_streams,
                           hipStream_t stream, int max_blocks);
}

// ------------------------------------------------------------------------
// DLPack minimal ABI (dlpack.h v0.8 layout)

typedef struct {
  int32_t device_type;  // kDLROCM = 10
  int32_t device_id;
} DLDevice;

typedef struct {
  uint8_t code;  // kDLUInt = 1
  uint8_t bits;
  uint16_t lanes;
} DLDataType;

typedef struct {
  void* data;
  DLDevice device;
  int32_t ndim;
  DLDataType dtype;
  int64_t* shape;
  int64_t* strides;
  uint64_t byte_offset;
} DLTensor;

struct DLManagedTensor {
  DLTensor dl_tensor;
  void* manager_ctx;
  void (*deleter)(DLManagedTensor*);
};

// ------------------------------------------------------------------------

struct DeviceBufferImpl {
  void* ptr = nullptr;
  size_t nbytes = 0;
  int device = 0;
  ~DeviceBufferImpl() {
    if (ptr) hipFree(ptr);  // best-effort; errors unreportable in dtor
  }
};

struct DlpackCtx {
  std::shared_ptr<DeviceBufferImpl> buf;
  int64_t shape[1];
  DLManagedTensor tensor;
};

class DeviceBuffer {
 public:
  explicit DeviceBuffer(size_t nbytes) {
    impl_ = std::make_shared<DeviceBufferImpl>();
    HIP_CHECK(hipGetDevice(&impl_->device));
    HIP_CHECK(hipMalloc(&impl_->ptr, nbytes));
    impl_->nbytes = nbytes;
  }
  uintptr_t ptr() const { return (uintptr_t)impl_->ptr; }
  size_t nbytes() const { return impl_->nbytes; }

  // Export as a 1-D uint8 DLPack tensor; the capsule co-owns the buffer.
  py::capsule to_dlpack() const {
    auto* ctx = new DlpackCtx();
    ctx->buf = impl_;
    ctx->shape[0] = (int64_t)impl_->nbytes;
    DLTensor& t = ctx->tensor.dl_tensor;
    t.data = impl_->ptr;
    t.device = {10 /*kDLROCM*/, impl_->device};
    t.ndim = 1;
    t.dtype = {1 /*kDLUInt*/, 8, 1};
    t.shape = ctx->shape;
    t.strides = nullptr;
    t.byte_offset = 0;
    ctx->tensor.manager_ctx = ctx;
    ctx->tensor.deleter = [](DLManagedTensor* self) {
      delete static_cast<DlpackCtx*>(self->manager_ctx);
    };
    return py::capsule(&ctx->tensor, "dltensor", [](PyObject* cap) {
      // unconsumed capsule: free it ourselves
      if (PyCapsule_IsValid(cap, "dltensor")) {
        auto* t = static_cast<DLManagedTensor*>(
            PyCapsule_GetPointer(cap, "dltensor"));
        t->deleter(t);
      }
    });
  }

 private:
  std::shared_ptr<DeviceBufferImpl> impl_;
};

// ------------------------------------------------------------------------
// Process-lifetime caches under PinnedPool / Stream / Event.
//
// hipHostMalloc of a ring (pin + map pages for the GPU) and stream/event
// creation are driver round-trips that contend when every worker thread of
// a pull does them at once; ring geometry does not change from pull to
// pull, so the resources are parked here when their owner dies and handed
// to the next owner of the same (device, size class).
//
// DEMODEL_PINNED_CACHE_MB caps the idle pinned bytes (default 4096; the
// default geometry with workers=8 needs 16 rings x 4 x 32 MiB = 2 GiB, the
// rest is room for the proxy's prefetch landers).  0 turns all three caches
// off: every release frees, exactly as before the caches existed.
//
// DEMODEL_NATIVE_SOCK (read in Python, utils/netio.py) decides whether the
// landers call PinnedPool::land_fd below or run their Python slab loop:
// unset/1 = native receive and send loops, recv / send = that side only,
// 0 = the Python loops on both ends.

static const uint64_t kSlabGranule = 2ull << 20;
static const uint64_t kHandleCap = 4096;  // idle streams / events, each

static uint64_t pinned_cap_from_env() {
  uint64_t mb = 4096;
  if (const char* v = getenv("DEMODEL_PINNED_CACHE_MB")) {
    char* end = nullptr;
    errno = 0;
    unsigned long long x = strtoull(v, &end, 10);
    if (end != v && errno == 0 && *v != '-') mb = x;
  }
  return mb << 20;
}

struct Caches {
  demodel::ResourceCache<void*> pinned;
  demodel::ResourceCache<hipStream_t> streams;
  demodel::ResourceCache<hipEvent_t> events;
  bool on;

  explicit Caches(uint64_t cap)
      : pinned(
            [](int, uint64_t nbytes) {
              void* p = nullptr;
              HIP_CHECK(hipHostMalloc(&p, nbytes, 0));
              return p;
            },
            [](int, uint64_t, void* p) { (void)hipHostFree(p); }, cap),
        streams(
            [](int, uint64_t prio) {
              hipStream_t s = nullptr;
              HIP_CHECK(hipStreamCreateWithPriority(
                  &s, hipStreamNonBlocking, (int)(int64_t)prio));
              return s;
            },
            [](int, uint64_t, hipStream_t s) { (void)hipStreamDestroy(s); },
            cap ? kHandleCap : 0),
        events(
            [](int, uint64_t flags) {
              hipEvent_t e = nullptr;
              HIP_CHECK(hipEventCreateWithFlags(&e, (unsigned)flags));
              return e;
            },
            [](int, uint64_t, hipEvent_t e) { (void)hipEventDestroy(e); },
            cap ? kHandleCap : 0),
        on(cap > 0) {}
};

// Leaked on purpose: the HIP runtime may already be torn down when static
// destructors run, and the OS reclaims pinned memory at exit anyway.
static Caches& caches() {
  static Caches* c = new Caches(pinned_cap_from_env());
  return *c;
}

// Pinned host slabs plus the landing ring that fences their reuse: each
// slab has an event recorded after its H2D copy and a busy flag, so a slab
// is refilled only once the GPU has read it.  One thread drives a ring (the
// engine keeps one lander per worker thread); the caches below it are
// thread-safe.
//
// Slabs go back to the cache in the destructor, never to hipHostFree while
// the cache has room.  hipHostFree's implicit device synchronisation used
// to guarantee that no copy still touched a slab; here the destructor
// drains the ring's own fences, and synchronises the device when a raw
// slab pointer was handed out (copies the ring did not see).  If any of
// that fails the slabs are freed, not cached.
static std::atomic<uint64_t> g_land_fd_calls{0};

class PinnedPool {
 public:
  PinnedPool(size_t slab_bytes, int n_slabs) : slab_bytes_(slab_bytes) {
    if (n_slabs < 0) throw std::invalid_argument("n_slabs < 0");
    HIP_CHECK(hipGetDevice(&device_));
    Caches& c = caches();
    class_ = c.on ? demodel::round_up_size_class(slab_bytes, kSlabGranule)
                  : slab_bytes;
    try {
      for (int i = 0; i < n_slabs; i++) {
        slabs_.push_back(c.pinned.take(device_, class_, class_));
        events_.push_back(
            c.events.take(device_, hipEventDisableTiming, 1));
      }
    } catch (...) {
      release_all(true);  // untouched so far
      throw;
    }
    busy_.assign(n_slabs, 0);
  }
  ~PinnedPool() {
    bool clean = drain_quiet();
    if (clean && raw_used_ && caches().on) {
      int cur = -1;
      clean = hipGetDevice(&cur) == hipSuccess && cur == device_ &&
              hipDeviceSynchronize() == hipSuccess;
    }
    release_all(clean);
  }
  PinnedPool(const PinnedPool&) = delete;
  PinnedPool& operator=(const PinnedPool&) = delete;

  int n_slabs() const { return (int)slabs_.size(); }
  size_t slab_bytes() const { return slab_bytes_; }
  uintptr_t slab_ptr(int i) {
    raw_used_ = true;  // caller may queue copies the ring cannot fence
    return (uintptr_t)slabs_.at(i);
  }
  py::memoryview slab_view(int i) {
    return py::memoryview::from_memory(slabs_.at(i), slab_bytes_);
  }

  // Wait until the GPU has read slot's previous contents.
  void acquire(int slot) {
    if (busy_.at(slot)) {
      HIP_CHECK(hipEventSynchronize(events_[slot]));
      busy_[slot] = 0;
    }
  }
  // Queue slab[slot][0:nbytes) -> dst on stream and fence the slot.
  void submit(int slot, uintptr_t dst, size_t nbytes, uintptr_t stream) {
    void* src = slabs_.at(slot);
    if (nbytes > slab_bytes_)
      throw std::out_of_range("submit: nbytes exceeds the slab");
    HIP_CHECK(hipMemcpyAsync((void*)dst, src, nbytes, hipMemcpyHostToDevice,
                             (hipStream_t)stream));
    busy_[slot] = 1;  // set first: a failed record must not hide the copy
    HIP_CHECK(hipEventRecord(events_[slot], (hipStream_t)stream));
  }
  // Make `stream` wait for slot's last submitted copy.
  void stream_wait(int slot, uintptr_t stream) {
    HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, events_.at(slot), 0));
  }
  void drain() {
    for (int i = 0; i < (int)busy_.size(); i++) acquire(i);
  }

  struct LandResult {
    uint64_t landed = 0;  // bytes whose H2D copy was submitted
    int status = 0;       // sock_io.h status of the receive that ended it
    double recv_s = 0;
    uint64_t recv_calls = 0;
  };
  // The landing loop for one byte range of a plain-TCP body, run without
  // the GIL: acquire slot, receive a slab's worth, copy into the head
  // buffer while it has room, submit, next slot.  Measured on the flagship
  // (profiles/native_socket_loops_ab.md): the blocking fd takes a 32 MiB
  // slab in 1.00 recv(MSG_WAITALL) calls where the timeout-mode Python
  // socket needed 17.1 poll+recv pairs.
  //
  // The first `prefilled` bytes of slot `slot0` are already in place (body
  // bytes that arrived with the response head; the caller acquired the
  // slot).  A receive that ends short stops the loop: whole slabs landed so
  // far are counted, the broken slab is not submitted.
  LandResult land_fd(int fd, uintptr_t dst, size_t nbytes, uintptr_t stream,
                     uintptr_t head_ptr, size_t head_cap,
                     int stall_timeout_ms, int slot0, size_t prefilled) {
    LandResult res;
    const int n = (int)slabs_.size();
    if (n == 0) throw std::invalid_argument("land_fd: ring has no slabs");
    if (slot0 < 0 || slot0 >= n)
      throw std::out_of_range("land_fd: slot0 outside the ring");
    if (prefilled > slab_bytes_ || prefilled > nbytes)
      throw std::out_of_range("land_fd: prefilled exceeds the first slab");
    g_land_fd_calls++;
    demodel::RecvSession sess(fd, stall_timeout_ms);
    size_t off = 0, head_len = 0;
    int slot = slot0;
    while (off < nbytes) {
      size_t want = nbytes - off < slab_bytes_ ? nbytes - off : slab_bytes_;
      size_t got = 0;
      if (off == 0 && prefilled) {
        got = prefilled;
      } else {
        acquire(slot);
      }
      char* slab = (char*)slabs_[slot];
      if (got < want) {
        auto t0 = std::chrono::steady_clock::now();
        demodel::IoResult r =
            sess.recv(slab + got, want - got, &res.recv_calls);
        res.recv_s += std::chrono::duration<double>(
                          std::chrono::steady_clock::now() - t0).count();
        if (r.bytes < want - got) {
          res.status = r.status ? r.status : demodel::kSockEof;
          break;
        }
      }
      if (head_ptr && head_len < head_cap) {
        size_t take = want < head_cap - head_len ? want : head_cap - head_len;
        memcpy((char*)head_ptr + head_len, slab, take);
        head_len += take;
      }
      submit(slot, dst + off, want, stream);
      off += want;
      res.landed = off;
      slot = (slot + 1) % n;
    }
    return res;
  }

  // Expand (src_off, dst_ptr, nbytes) u64 triples into scatter RangeDesc
  // records of at most `piece` bytes, straight into slab `slot`.  Throws
  // when they do not fit; never writes a partial table.
  uint64_t write_scatter_descs(int slot, const uint64_t* triples,
                               size_t n_triples, uint64_t piece) {
    void* slab = slabs_.at(slot);
    int64_t n = demodel::expand_scatter_descs(
        triples, n_triples, piece, (uint64_t*)slab,
        slab_bytes_ / (demodel::kRangeDescWords * sizeof(uint64_t)));
    if (n < 0)
      throw std::out_of_range(
          "write_scatter_descs: descriptors exceed the slab");
    return (uint64_t)n;
  }

 private:
  bool drain_quiet() {
    bool ok = true;
    for (size_t i = 0; i < busy_.size(); i++)
      if (busy_[i] && hipEventSynchronize(events_[i]) != hipSuccess)
        ok = false;
    return ok;
  }
  void release_all(bool reusable) {
    Caches& c = caches();
    for (void* s : slabs_)
      c.pinned.release(device_, class_, class_, s, reusable);
    for (hipEvent_t e : events_)
      c.events.release(device_, hipEventDisableTiming, 1, e, reusable);
    slabs_.clear();
    events_.clear();
  }

  size_t slab_bytes_;
  uint64_t class_ = 0;
  int device_ = 0;
  bool raw_used_ = false;
  std::vector<void*> slabs_;
  std::vector<hipEvent_t> events_;
  std::vector<char> busy_;
};

class Stream {
 public:
  explicit Stream(int priority = 0)
      : key_((uint64_t)(int64_t)priority) {
    HIP_CHECK(hipGetDevice(&device_));
    s_ = caches().streams.take(device_, key_, 1);
  }
  ~Stream() {
    // cached only once idle; a stream that fails to synchronise is dropped
    Caches& c = caches();
    bool idle = c.on && hipStreamSynchronize(s_) == hipSuccess;
    c.streams.release(device_, key_, 1, s_, idle);
  }
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  void sync() { HIP_CHECK(hipStreamSynchronize(s_)); }
  uintptr_t handle() const { return (uintptr_t)s_; }
  hipStream_t raw() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
  uint64_t key_;
  int device_ = 0;
};

class Event {
 public:
  // timing=false (hipEventDisableTiming) for pure fences; elapsed_ms needs
  // both events created with timing.
  explicit Event(bool timing = true)
      : flags_(timing ? hipEventDefault : hipEventDisableTiming) {
    HIP_CHECK(hipGetDevice(&device_));
    e_ = caches().events.take(device_, flags_, 1);
  }
  ~Event() {
    // cached only when complete (or never recorded): the next owner's
    // sync()/query() must not observe this owner's work
    Caches& c = caches();
    bool idle = c.on && hipEventQuery(e_) == hipSuccess;
    c.events.release(device_, flags_, 1, e_, idle);
  }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  void record(uintptr_t stream) {
    HIP_CHECK(hipEventRecord(e_, (hipStream_t)stream));
  }
  void wait(uintptr_t stream) {
    HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, e_, 0));
  }
  void sync() { HIP_CHECK(hipEventSynchronize(e_)); }
  bool query() { return hipEventQuery(e_) == hipSuccess; }
  float elapsed_ms(const Event& start) {
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, start.e_, e_));
    return ms;
  }

 private:
  hipEvent_t e_ = nullptr;
  uint64_t flags_;
  int device_ = 0;
};

static py::dict stats_dict(const demodel::CacheStats& s) {
  py::dict d;
  d["hits"] = s.hits;
  d["misses"] = s.misses;
  d["bytes_cached"] = s.bytes_cached;
  d["bytes_live"] = s.bytes_live;
  d["freed"] = s.freed;
  d["cap_bytes"] = s.cap_bytes;
  return d;
}

// ------------------------------------------------------------------------
// file -> pinned reads (no GIL)

static ssize_t read_file_into(int fd, uintptr_t dst, size_t want,
                              int64_t offset) {
  char* p = (char*)dst;
  size_t got = 0;
  while (got < want) {
    ssize_t n = offset >= 0
                    ? pread(fd, p + got, want - got, offset + (int64_t)got)
                    : read(fd, p + got, want - got);
    if (n < 0) {
      if (errno == EINTR) continue;
      return -errno;
    }
    if (n == 0) break;
    got += (size_t)n;
  }
  return (ssize_t)got;
}

// ------------------------------------------------------------------------

PYBIND11_MODULE(_hip, m) {
  m.doc() = "demodel-amd MI355X pipeline runtime + CDNA4 kernels";

  m.def("device_count", [] {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    return e == hipSuccess ? n : 0;
  });
  m.def("device_probe", [] {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    return py::make_tuple(n, std::string(hipGetErrorString(e)));
  });
  m.def("set_device", [](int d) { HIP_CHECK(hipSetDevice(d)); });
  m.def("device_sync", [] { HIP_CHECK(hipDeviceSynchronize()); },
        py::call_guard<py::gil_scoped_release>());

  py::class_<DeviceBuffer>(m, "DeviceBuffer")
      .def(py::init<size_t>(), py::arg("nbytes"),
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("ptr", &DeviceBuffer::ptr)
      .def_property_readonly("nbytes", &DeviceBuffer::nbytes)
      .def("to_dlpack", &DeviceBuffer::to_dlpack);

  py::class_<PinnedPool>(m, "PinnedPool")
      .def(py::init<size_t, int>(), py::arg("slab_bytes"),
           py::arg("n_slabs"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("n_slabs", &PinnedPool::n_slabs)
      .def_property_readonly("slab_bytes", &PinnedPool::slab_bytes)
      .def("slab_ptr", &PinnedPool::slab_ptr)
      .def("slab_view", &PinnedPool::slab_view)
      .def("acquire", &PinnedPool::acquire, py::arg("slot"),
           py::call_guard<py::gil_scoped_release>(),
           "wait (no GIL) until the GPU has read the slot's last copy")
      .def("submit", &PinnedPool::submit, py::arg("slot"), py::arg("dst"),
           py::arg("nbytes"), py::arg("stream"),
           py::call_guard<py::gil_scoped_release>(),
           "H2D copy of the slot's first nbytes to dst + fence record")
      .def("stream_wait", &PinnedPool::stream_wait, py::arg("slot"),
           py::arg("stream"))
      .def("drain", &PinnedPool::drain,
           py::call_guard<py::gil_scoped_release>(),
           "wait for every busy slot")
      .def("land_fd",
           [](PinnedPool& self, int fd, uintptr_t dst, size_t nbytes,
              uintptr_t stream, uintptr_t head_ptr, size_t head_cap,
              int stall_timeout_ms, int slot0, size_t prefilled) {
             PinnedPool::LandResult r;
             {
               py::gil_scoped_release nogil;
               r = self.land_fd(fd, dst, nbytes, stream, head_ptr, head_cap,
                                stall_timeout_ms, slot0, prefilled);
             }
             return py::make_tuple(r.landed, r.status, r.recv_s,
                                   r.recv_calls);
           },
           py::arg("fd"), py::arg("dst"), py::arg("nbytes"),
           py::arg("stream"), py::arg("head_ptr"), py::arg("head_cap"),
           py::arg("stall_timeout_ms"), py::arg("slot0") = 0,
           py::arg("prefilled") = 0,
           "land nbytes of a plain-TCP body fd -> ring -> dst without the "
           "GIL -> (bytes landed, status, recv seconds, recv calls); status "
           "0 ok, -1 EOF, ETIMEDOUT stall, else errno.  The first min(nbytes"
           ", head_cap) bytes are also copied to head_ptr (0 = no head)")
      .def("write_scatter_descs",
           [](PinnedPool& self, int slot, py::buffer triples,
              uint64_t piece) {
             py::buffer_info info = triples.request();
             size_t nb = (size_t)info.size * (size_t)info.itemsize;
             if (nb % 24 || ((uintptr_t)info.ptr & 7))
               throw std::invalid_argument(
                   "write_scatter_descs: triples must be aligned u64 x 3");
             return self.write_scatter_descs(
                 slot, (const uint64_t*)info.ptr, nb / 24, piece);
           },
           py::arg("slot"), py::arg("triples"), py::arg("piece"),
           "expand (src_off, dst_ptr, nbytes) u64 triples into 32-byte "
           "scatter descriptors of <= piece bytes in the slab; returns the "
           "descriptor count, raises if they exceed the slab");

  py::class_<Stream>(m, "Stream")
      .def(py::init<int>(), py::arg("priority") = 0)
      .def("sync", &Stream::sync,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("handle", &Stream::handle);

  py::class_<Event>(m, "Event")
      .def(py::init<bool>(), py::arg("timing") = true)
      .def("record", &Event::record)
      .def("wait", &Event::wait)
      .def("sync", &Event::sync, py::call_guard<py::gil_scoped_release>())
      .def("query", &Event::query)
      .def("elapsed_ms", &Event::elapsed_ms);

  m.def("cache_stats", [] {
    Caches& c = caches();
    py::dict d;
    d["pinned"] = stats_dict(c.pinned.stats());
    d["streams"] = stats_dict(c.streams.stats());
    d["events"] = stats_dict(c.events.stats());
    return d;
  }, "hits/misses/bytes_cached/bytes_live/freed/cap_bytes of the pinned-"
     "slab, stream and event caches (streams and events count 1 each)");
  m.def("cache_trim", [] {
    Caches& c = caches();
    c.streams.trim();
    c.events.trim();
    return c.pinned.trim();
  }, py::call_guard<py::gil_scoped_release>(),
     "free everything idle in the caches; returns pinned bytes let go");

  m.def("h2d_async",
        [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t stream) {
          HIP_CHECK(hipMemcpyAsync((void*)dst, (void*)src, n,
                                   hipMemcpyHostToDevice,
                                   (hipStream_t)stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("d2h_async",
        [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t stream) {
          HIP_CHECK(hipMemcpyAsync((void*)dst, (void*)src, n,
                                   hipMemcpyDeviceToHost,
                                   (hipStream_t)stream));
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("d2d_async",
        [](uintptr_t dst, uintptr_t src, size_t n, uintptr_t stream) {
          HIP_CHECK(hipMemcpyAsync((void*)dst, (void*)src, n,
                                   hipMemcpyDeviceToDevice,
                                   (hipStream_t)stream));
        },
        py::call_guard<py::gil_scoped_release>());

  m.def("sock_stats", [] {
    demodel::SockCounters& c = demodel::sock_counters();
    py::dict d;
    d["recv_exact"] = c.recv_exact.load();
    d["recv_calls"] = c.recv_calls.load();
    d["land_fd"] = g_land_fd_calls.load();
    return d;
  }, "native landing-loop counters of this extension since import");
  m.def("read_file_into", &read_file_into, py::arg("fd"), py::arg("dst"),
        py::arg("want"), py::arg("offset") = -1,
        py::call_guard<py::gil_scoped_release>());

  // ---- kernel launches -------------------------------------------------
  m.def("sha256_batch",
        [](uintptr_t data, size_t nbytes, size_t chunk_bytes,
           uintptr_t out_digests, int n_chunks, uintptr_t stream) {
          launch_sha256_batch((const void*)data, nbytes, chunk_bytes,
                              (uint32_t*)out_digests, n_chunks,
                              (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>(),
        "SHA-256 of n_chunks independent chunks of `data` (last may be "
        "short); digests -> out (n_chunks x 8 u32, big-endian words)");
  m.def("sha256_chain_init",
        [](uintptr_t state, uintptr_t stream) {
          launch_sha256_chain_init((uint32_t*)state, (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("sha256_chain_update",
        [](uintptr_t state, uintptr_t data, size_t nblocks,
           uintptr_t stream) {
          launch_sha256_chain_update((uint32_t*)state, (const void*)data,
                                     nblocks, (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>(),
        "advance one whole-blob SHA-256 chain over nblocks 64-byte blocks "
        "already resident in HBM");
  m.def("scatter_ranges",
        [](uintptr_t src, uintptr_t desc, int n_desc, uintptr_t stream) {
          launch_scatter_ranges((const void*)src, (const uint64_t*)desc,
                                n_desc, (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>(),
        "copy n_desc (src_off,dst_ptr,len) descriptors from a landed blob "
        "into tensor storages");
  m.def("cast_f32_to_bf16",
        [](uintptr_t src, uintptr_t dst, size_t n, uintptr_t stream) {
          launch_cast_f32_to_bf16((const float*)src, (uint16_t*)dst, n,
                                  (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("fp8_block_dequant",
        [](uintptr_t src, uintptr_t scale, int scale_dtype, uintptr_t dst,
           int dst_dtype, int64_t rows, int64_t cols, int64_t block_rows,
           int64_t block_cols, uintptr_t stream) {
          if (scale_dtype < 0 || scale_dtype > 2)
            throw std::invalid_argument(
                "fp8_block_dequant: scale_dtype must be 0=f32 1=bf16 2=f16");
          if (dst_dtype < 0 || dst_dtype > 1)
            throw std::invalid_argument(
                "fp8_block_dequant: dst_dtype must be 0=bf16 1=f32");
          if (rows < 0 || cols < 0)
            throw std::invalid_argument(
                "fp8_block_dequant: negative shape");
          if (block_rows <= 0 || block_cols <= 0)
            throw std::invalid_argument(
                "fp8_block_dequant: block must be positive");
          if (cols && rows > INT64_MAX / 4 / cols)
            throw std::invalid_argument(
                "fp8_block_dequant: shape overflows");
          launch_fp8_block_dequant((const void*)src, (const void*)scale,
                                   scale_dtype, (void*)dst, dst_dtype, rows,
                                   cols, block_rows, block_cols,
                                   (hipStream_t)stream);
        },
        py::arg("src"), py::arg("scale"), py::arg("scale_dtype"),
        py::arg("dst"), py::arg("dst_dtype"), py::arg("rows"),
        py::arg("cols"), py::arg("block_rows"), py::arg("block_cols"),
        py::arg("stream"), py::call_guard<py::gil_scoped_release>(),
        "widen a row-major [rows, cols] OCP e4m3fn tensor to bf16/f32, "
        "multiplying by scale[r / block_rows][c / block_cols]");
  m.def("fp8_block_dequant_pass_limits", [] {
          int64_t lim[2];
          fp8_block_dequant_pass_limits(lim);
          return py::make_tuple(lim[0], lim[1]);
        },
        "(elements, columns of one row) that one pass of "
        "fp8_block_dequant's largest grid covers");
  m.def("gguf_dequant",
        [](int qtype, uintptr_t src, uintptr_t dst, int64_t n_blocks,
           uintptr_t stream) {
          launch_gguf_dequant(qtype, (const void*)src, (uint16_t*)dst,
                              n_blocks, (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>());
  m.def("inflate_streams",
        [](uintptr_t desc, int n_streams, uintptr_t stream) {
          launch_inflate_streams((const uint64_t*)desc, n_streams,
                                 (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>(),
        "DEFLATE-inflate n_streams descriptors (8 u64 each: src, src_len, "
        "dst, dst_cap, written, status, consumed, pad), wave per stream");
  m.def("zstd_frames",
        [](uintptr_t desc, int n_frames, uintptr_t stream, int window) {
          launch_zstd_frames((const uint64_t*)desc, n_frames,
                             (hipStream_t)stream, window);
        },
        py::call_guard<py::gil_scoped_release>(), py::arg("desc"),
        py::arg("n_frames"), py::arg("stream"), py::arg("window") = 0,
        "zstd-decompress n_frames descriptors (8 u64 each: src, src_len, "
        "dst, dst_cap, written, status, consumed, ws), wave per frame; ws "
        "needs >= 144 KiB per frame; window 0=auto/16384/65536 selects "
        "the LDS window template");
  m.def("snappy_streams",
        [](uintptr_t desc, int n_streams, uintptr_t stream) {
          launch_snappy_streams((const uint64_t*)desc, n_streams,
                                (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>(),
        "snappy-decompress n_streams descriptors (8 u64 each: src, "
        "src_len, dst, dst_cap, written, status, consumed, pad), wave "
        "per stream (parquet's default page codec)");
  m.def("lz4_streams",
        [](uintptr_t desc, int n_streams, uintptr_t stream) {
          launch_lz4_streams((const uint64_t*)desc, n_streams,
                             (hipStream_t)stream);
        },
        py::call_guard<py::gil_scoped_release>(),
        "LZ4 raw-block decompress n_streams descriptors (8 u64 each: "
        "src, src_len, dst, dst_cap, written, status, consumed, pad), "
        "wave per stream (parquet LZ4/LZ4_RAW page codecs)");
  m.def("parquet_hybrid",
        [](uintptr_t desc, int n_streams, uintptr_t stream,
           int max_blocks) {
          launch_parquet_hybrid((const uint64_t*)desc, n_streams,
                                (hipStream_t)stream, max_blocks);
        },
        py::call_guard<py::gil_scoped_release>(), py::arg("desc"),
        py::arg("n_streams"), py::arg("stream"),
        py::arg("max_blocks") = 0,
        "decode n_streams bare RLE/bit-packed hybrid streams (8 u64 "
        "each: src, src_len, dst, count, bit_width, limit, status, "
        "matched) into u32 values, wave per stream; max_blocks caps the "
        "grid (0: default)");
  m.def("parquet_decode",
        [](uintptr_t desc, int n_pages, uintptr_t stream, int max_blocks) {
          launch_parquet_decode((const uint64_t*)desc, n_pages,
                                (hipStream_t)stream, max_blocks);
        },
        py::call_guard<py::gil_scoped_release>(), py::arg("desc"),
        py::arg("n_pages"), py::arg("stream"), py::arg("max_blocks") = 0,
        "decode n_pages decompressed parquet data pages (16 u64 each: "
        "src, src_len, dict, dict_count, out_vals, out_def, out_rep, "
        "scratch, num_values, params, rep_len, def_len, status, non_null, "
        "consumed, pad) into entry-aligned typed buffers, wave per page");
}

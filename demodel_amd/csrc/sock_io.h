// Socket loops of the landing path and scatter-descriptor expansion.
// Host-only: no HIP and no Python includes, so both extensions use it and a
// plain C++ driver tests it under sanitizers (tests/sock_io_host_main.cpp).
//
// recv_exact / sendfile_exact move an exact byte count through one fd and
// report (bytes moved, status).  They work on blocking and on O_NONBLOCK
// fds:
//   * blocking: SO_RCVTIMEO / SO_SNDTIMEO is set to the stall limit for the
//     call and put back after it, so one recv(MSG_WAITALL) takes a whole
//     slab and one sendfile() up to 2 GiB;
//   * O_NONBLOCK: EAGAIN waits in poll() for the rest of the stall budget.
//     The receiver raises SO_RCVLOWAT to min(remaining, kLowat) first, so
//     poll wakes once per few MiB, not once per segment burst, and puts it
//     back to 1 on the way out.
// "Stall" means no byte moved for stall_timeout_ms; progress resets the
// clock.  A blocking fd notices a stall between one and two limits after
// the last byte (the kernel's timeout runs per call).  Bytes moved before
// a timeout, EOF or error are always reported; nothing is dropped.
//
// BlockingScope lends a non-blocking fd (Python sockets with a timeout,
// asyncio transports) to such a loop: it clears O_NONBLOCK and restores it
// on every path out.

#pragma once

#include <fcntl.h>
#include <poll.h>
#include <pthread.h>
#include <signal.h>
#include <sys/sendfile.h>
#include <sys/socket.h>
#include <sys/time.h>
#include <sys/types.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <optional>

namespace demodel {

// status values next to the byte count: 0 = all bytes moved, kSockEof = the
// peer closed (or the file ended) first, ETIMEDOUT = stalled, else errno
static const int kSockEof = -1;

static const size_t kLowat = 4u << 20;
// sendfile(2) moves at most this much per call
static const size_t kSendfileMax = 0x7ffff000;

struct IoResult {
  uint64_t bytes = 0;
  int status = 0;
};

// process-wide (per extension) syscall counters, for tests and A/B tables
struct SockCounters {
  std::atomic<uint64_t> recv_exact{0};      // recv_exact invocations
  std::atomic<uint64_t> recv_calls{0};      // recv(2) inside them
  std::atomic<uint64_t> sendfile_exact{0};  // sendfile_exact invocations
  std::atomic<uint64_t> sendfile_calls{0};  // sendfile(2) inside them
};
inline SockCounters& sock_counters() {
  static SockCounters c;
  return c;
}

inline int64_t mono_ms() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (int64_t)ts.tv_sec * 1000 + ts.tv_nsec / 1000000;
}

inline bool fd_nonblocking(int fd) {
  int fl = fcntl(fd, F_GETFL);
  return fl >= 0 && (fl & O_NONBLOCK);
}

// poll for `events` until deadline_ms (monotonic); EINTR keeps the deadline.
// >0 ready, 0 timed out, <0 -errno
inline int poll_until(int fd, short events, int64_t deadline_ms) {
  for (;;) {
    int64_t left = deadline_ms - mono_ms();
    if (left < 0) left = 0;
    struct pollfd p = {fd, events, 0};
    int r = poll(&p, 1, (int)(left > 0x7fffffff ? 0x7fffffff : left));
    if (r >= 0) return r;
    if (errno != EINTR) return -errno;
    if (left == 0) return 0;
  }
}

// Clears O_NONBLOCK for the scope and restores the flag word it found.
class BlockingScope {
 public:
  explicit BlockingScope(int fd) : fd_(fd) {
    flags_ = fcntl(fd, F_GETFL);
    if (flags_ >= 0 && (flags_ & O_NONBLOCK))
      flipped_ = fcntl(fd, F_SETFL, flags_ & ~O_NONBLOCK) == 0;
  }
  ~BlockingScope() {
    if (flipped_) (void)fcntl(fd_, F_SETFL, flags_);
  }
  BlockingScope(const BlockingScope&) = delete;
  BlockingScope& operator=(const BlockingScope&) = delete;

 private:
  int fd_;
  int flags_ = -1;
  bool flipped_ = false;
};

// Sets SO_RCVTIMEO or SO_SNDTIMEO for the scope (blocking fds only).
class SockTimeoutScope {
 public:
  SockTimeoutScope(int fd, int opt, int timeout_ms) : fd_(fd), opt_(opt) {
    socklen_t len = sizeof(old_);
    if (getsockopt(fd, SOL_SOCKET, opt, &old_, &len) != 0) return;
    struct timeval tv;
    tv.tv_sec = timeout_ms / 1000;
    tv.tv_usec = (timeout_ms % 1000) * 1000;
    if (timeout_ms <= 0) tv.tv_usec = 1000;  // 0 would mean "forever"
    set_ = setsockopt(fd, SOL_SOCKET, opt, &tv, sizeof(tv)) == 0;
  }
  ~SockTimeoutScope() {
    if (set_) (void)setsockopt(fd_, SOL_SOCKET, opt_, &old_, sizeof(old_));
  }
  SockTimeoutScope(const SockTimeoutScope&) = delete;
  SockTimeoutScope& operator=(const SockTimeoutScope&) = delete;

 private:
  int fd_;
  int opt_;
  struct timeval old_ = {0, 0};
  bool set_ = false;
};

// The receive loop proper.  `nonblock` says how the fd is; a blocking fd
// must already carry SO_RCVTIMEO = the stall limit (recv_exact and
// RecvSession arrange that).
inline IoResult recv_loop(int fd, void* dst, size_t want, int stall_timeout_ms,
                          bool nonblock, uint64_t* calls) {
  IoResult r;
  char* p = (char*)dst;
  uint64_t n_calls = 0;
  int lowat = 1;  // what we last set; 1 is the socket default
  int64_t deadline = mono_ms() + stall_timeout_ms;
  bool last_chance = false;  // poll timed out: one more recv at lowat 1
  while (r.bytes < want) {
    n_calls++;
    ssize_t n = recv(fd, p + r.bytes, want - r.bytes, MSG_WAITALL);
    if (n > 0) {
      r.bytes += (uint64_t)n;
      deadline = mono_ms() + stall_timeout_ms;
      last_chance = false;
      continue;
    }
    if (n == 0) {
      r.status = kSockEof;
      break;
    }
    if (errno == EINTR) continue;
    if (errno != EAGAIN && errno != EWOULDBLOCK) {
      r.status = errno;
      break;
    }
    if (!nonblock || last_chance) {  // SO_RCVTIMEO ran out / truly empty
      r.status = ETIMEDOUT;
      break;
    }
    size_t rem = want - r.bytes;
    int target = (int)(rem < kLowat ? rem : kLowat);
    if (target != lowat &&
        setsockopt(fd, SOL_SOCKET, SO_RCVLOWAT, &target, sizeof(target)) == 0)
      lowat = target;
    int pr = poll_until(fd, POLLIN, deadline);
    if (pr < 0) {
      r.status = -pr;
      break;
    }
    if (pr == 0) {
      // fewer than lowat bytes may sit in the queue: take them before
      // calling it a stall
      int one = 1;
      if (lowat != 1 &&
          setsockopt(fd, SOL_SOCKET, SO_RCVLOWAT, &one, sizeof(one)) == 0)
        lowat = 1;
      last_chance = true;
    }
  }
  if (lowat != 1) {
    int one = 1;
    (void)setsockopt(fd, SOL_SOCKET, SO_RCVLOWAT, &one, sizeof(one));
  }
  if (calls) *calls += n_calls;
  sock_counters().recv_calls += n_calls;
  return r;
}

// One fd prepared once for many recv_loop calls (a ring landing): makes it
// blocking with SO_RCVTIMEO = stall limit, restores both when it dies.
class RecvSession {
 public:
  RecvSession(int fd, int stall_timeout_ms)
      : fd_(fd), stall_(stall_timeout_ms), blocking_(fd),
        timeo_(fd, SO_RCVTIMEO, stall_timeout_ms) {}
  IoResult recv(void* dst, size_t want, uint64_t* calls) {
    sock_counters().recv_exact++;
    return recv_loop(fd_, dst, want, stall_, false, calls);
  }

 private:
  int fd_;
  int stall_;
  BlockingScope blocking_;
  SockTimeoutScope timeo_;
};

// Receive until `want` bytes, EOF, error or stall; the fd keeps its mode.
inline IoResult recv_exact(int fd, void* dst, size_t want,
                           int stall_timeout_ms, uint64_t* calls) {
  sock_counters().recv_exact++;
  if (fd_nonblocking(fd))
    return recv_loop(fd, dst, want, stall_timeout_ms, true, calls);
  SockTimeoutScope t(fd, SO_RCVTIMEO, stall_timeout_ms);
  return recv_loop(fd, dst, want, stall_timeout_ms, false, calls);
}

// EPIPE must come back as a status, not as SIGPIPE: the signal is blocked
// for this thread during the call and a SIGPIPE we caused is consumed.
class SigpipeScope {
 public:
  SigpipeScope() {
    sigset_t pipe_set, pending;
    sigemptyset(&pipe_set);
    sigaddset(&pipe_set, SIGPIPE);
    sigemptyset(&pending);
    sigpending(&pending);
    was_pending_ = sigismember(&pending, SIGPIPE) == 1;
    armed_ = pthread_sigmask(SIG_BLOCK, &pipe_set, &old_) == 0;
  }
  ~SigpipeScope() {
    if (!armed_) return;
    if (!was_pending_) {
      sigset_t pipe_set;
      sigemptyset(&pipe_set);
      sigaddset(&pipe_set, SIGPIPE);
      struct timespec zero = {0, 0};
      while (sigtimedwait(&pipe_set, nullptr, &zero) < 0 && errno == EINTR) {
      }
    }
    (void)pthread_sigmask(SIG_SETMASK, &old_, nullptr);
  }
  SigpipeScope(const SigpipeScope&) = delete;
  SigpipeScope& operator=(const SigpipeScope&) = delete;

 private:
  sigset_t old_;
  bool was_pending_ = false;
  bool armed_ = false;
};

// sendfile [offset, offset+length) of in_fd to the socket out_fd; same
// contract as recv_exact.  kSockEof = in_fd ended before `length`.
inline IoResult sendfile_exact(int out_fd, int in_fd, int64_t offset,
                               size_t length, int stall_timeout_ms,
                               uint64_t* calls) {
  sock_counters().sendfile_exact++;
  IoResult r;
  SigpipeScope no_sigpipe;
  bool nonblock = fd_nonblocking(out_fd);
  // only a blocking fd needs the kernel-side limit
  std::optional<SockTimeoutScope> timeo;
  if (!nonblock) timeo.emplace(out_fd, SO_SNDTIMEO, stall_timeout_ms);
  uint64_t n_calls = 0;
  off_t off = (off_t)offset;
  int64_t deadline = mono_ms() + stall_timeout_ms;
  while (r.bytes < length) {
    size_t chunk = length - r.bytes;
    if (chunk > kSendfileMax) chunk = kSendfileMax;
    n_calls++;
    ssize_t n = sendfile(out_fd, in_fd, &off, chunk);
    if (n > 0) {
      r.bytes += (uint64_t)n;
      deadline = mono_ms() + stall_timeout_ms;
      continue;
    }
    if (n == 0) {
      r.status = kSockEof;
      break;
    }
    if (errno == EINTR) continue;
    if (errno != EAGAIN && errno != EWOULDBLOCK) {
      r.status = errno;
      break;
    }
    if (!nonblock) {
      r.status = ETIMEDOUT;
      break;
    }
    int pr = poll_until(out_fd, POLLOUT, deadline);
    if (pr < 0) {
      r.status = -pr;
      break;
    }
    if (pr == 0) {
      r.status = ETIMEDOUT;
      break;
    }
  }
  if (calls) *calls += n_calls;
  sock_counters().sendfile_calls += n_calls;
  return r;
}

// ------------------------------------------------------------------------
// scatter descriptors (csrc/scatter.hip RangeDesc: src_off, dst_ptr, nbytes,
// pad; 4 x u64)

static const size_t kRangeDescWords = 4;

inline uint64_t scatter_desc_count(const uint64_t* triples, size_t n_triples,
                                   uint64_t piece) {
  uint64_t n = 0;
  for (size_t i = 0; i < n_triples; i++) {
    uint64_t nbytes = triples[3 * i + 2];
    n += nbytes / piece + (nbytes % piece ? 1 : 0);
  }
  return n;
}

// Expand (src_off, dst_ptr, nbytes) triples into records of at most `piece`
// bytes each, written to out[0 : cap_records).  Returns the record count,
// or -1 with nothing written when they do not fit (or piece is 0).
inline int64_t expand_scatter_descs(const uint64_t* triples, size_t n_triples,
                                    uint64_t piece, uint64_t* out,
                                    uint64_t cap_records) {
  if (piece == 0) return -1;
  uint64_t need = scatter_desc_count(triples, n_triples, piece);
  if (need > cap_records) return -1;
  uint64_t* w = out;
  for (size_t i = 0; i < n_triples; i++) {
    uint64_t src = triples[3 * i], dst = triples[3 * i + 1];
    uint64_t nbytes = triples[3 * i + 2];
    for (uint64_t off = 0; off < nbytes; off += piece) {
      uint64_t n = nbytes - off < piece ? nbytes - off : piece;
      w[0] = src + off;
      w[1] = dst + off;
      w[2] = n;
      w[3] = 0;
      w += kRangeDescWords;
    }
  }
  return (int64_t)need;
}

}  // namespace demodel

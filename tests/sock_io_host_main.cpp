// Stand-alone driver for csrc/sock_io.h (see test_sock_io_host.py): built
// with a plain C++ compiler under ASan+UBSan and under TSan and run as a
// child process.  Every case runs over a loopback TCP pair.

#include <arpa/inet.h>
#include <netinet/in.h>
#include <netinet/tcp.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "sock_io.h"

using demodel::IoResult;

static int g_failed = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,     \
                   #cond);                                             \
      g_failed++;                                                      \
    }                                                                  \
  } while (0)

static uint8_t pat(size_t i) { return (uint8_t)((i * 31 + 7 + (i >> 11)) & 0xff); }

static std::vector<uint8_t> pattern(size_t n, size_t base = 0) {
  std::vector<uint8_t> v(n);
  for (size_t i = 0; i < n; i++) v[i] = pat(base + i);
  return v;
}

static void tcp_pair(int* a, int* b) {
  int ls = socket(AF_INET, SOCK_STREAM, 0);
  struct sockaddr_in sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.sin_family = AF_INET;
  sa.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
  socklen_t len = sizeof(sa);
  if (ls < 0 || bind(ls, (struct sockaddr*)&sa, sizeof(sa)) != 0 ||
      listen(ls, 1) != 0 || getsockname(ls, (struct sockaddr*)&sa, &len) != 0) {
    std::perror("listen");
    std::exit(2);
  }
  *a = socket(AF_INET, SOCK_STREAM, 0);
  if (*a < 0 || connect(*a, (struct sockaddr*)&sa, sizeof(sa)) != 0) {
    std::perror("connect");
    std::exit(2);
  }
  *b = accept(ls, nullptr, nullptr);
  if (*b < 0) {
    std::perror("accept");
    std::exit(2);
  }
  close(ls);
  int one = 1;
  setsockopt(*a, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
  setsockopt(*b, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
}

static void set_nonblock(int fd, bool on) {
  int fl = fcntl(fd, F_GETFL);
  fcntl(fd, F_SETFL, on ? (fl | O_NONBLOCK) : (fl & ~O_NONBLOCK));
}

static void send_all(int fd, const uint8_t* p, size_t n) {
  size_t off = 0;
  while (off < n) {
    ssize_t w = send(fd, p + off, n - off, MSG_NOSIGNAL);
    if (w < 0) {
      if (errno == EINTR) continue;
      return;
    }
    off += (size_t)w;
  }
}

// the fd must leave recv_exact as it entered it
static void check_fd_state(int fd, bool nonblock) {
  CHECK(demodel::fd_nonblocking(fd) == nonblock);
  int lowat = 0;
  socklen_t l = sizeof(lowat);
  CHECK(getsockopt(fd, SOL_SOCKET, SO_RCVLOWAT, &lowat, &l) == 0 &&
        lowat == 1);
  struct timeval tv = {1, 1};
  l = sizeof(tv);
  CHECK(getsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, &l) == 0 &&
        tv.tv_sec == 0 && tv.tv_usec == 0);
}

static void case_small_writes(bool nonblock) {
  int a, b;
  tcp_pair(&a, &b);
  set_nonblock(b, nonblock);
  const size_t n = 300000;
  std::vector<uint8_t> data = pattern(n);
  std::thread w([&] {
    size_t off = 0, k = 0;
    while (off < n) {
      size_t c = 1 + (k * 977) % 1500;
      if (c > n - off) c = n - off;
      send_all(a, data.data() + off, c);
      off += c;
      if (++k % 64 == 0) usleep(200);
    }
  });
  std::vector<uint8_t> got(n + 16, 0xEE);
  uint64_t calls = 0;
  IoResult r = demodel::recv_exact(b, got.data(), n, 2000, &calls);
  w.join();
  CHECK(r.status == 0);
  CHECK(r.bytes == n);
  CHECK(calls >= 1);
  CHECK(std::memcmp(got.data(), data.data(), n) == 0);
  CHECK(got[n] == 0xEE);  // nothing past `want`
  check_fd_state(b, nonblock);
  close(a);
  close(b);
}

static void case_peer_closes(bool nonblock) {
  int a, b;
  tcp_pair(&a, &b);
  set_nonblock(b, nonblock);
  std::vector<uint8_t> data = pattern(1000);
  std::thread w([&] {
    send_all(a, data.data(), 600);
    usleep(20000);
    send_all(a, data.data() + 600, 400);
    close(a);
  });
  std::vector<uint8_t> got(5000, 0xEE);
  uint64_t calls = 0;
  IoResult r = demodel::recv_exact(b, got.data(), 5000, 2000, &calls);
  w.join();
  CHECK(r.status == demodel::kSockEof);
  CHECK(r.bytes == 1000);
  CHECK(std::memcmp(got.data(), data.data(), 1000) == 0);
  CHECK(got[1000] == 0xEE);
  check_fd_state(b, nonblock);
  close(b);
}

static void case_stalled_peer(bool nonblock) {
  int a, b;
  tcp_pair(&a, &b);
  set_nonblock(b, nonblock);
  std::vector<uint8_t> data = pattern(777);
  send_all(a, data.data(), 500);
  std::thread w([&] {
    usleep(50000);  // progress inside the first limit resets the clock
    send_all(a, data.data() + 500, 277);
  });
  std::vector<uint8_t> got(5000, 0xEE);
  uint64_t calls = 0;
  auto t0 = std::chrono::steady_clock::now();
  IoResult r = demodel::recv_exact(b, got.data(), 5000, 200, &calls);
  double s = std::chrono::duration<double>(
                 std::chrono::steady_clock::now() - t0).count();
  w.join();
  CHECK(r.status == ETIMEDOUT);
  CHECK(r.bytes == 777);
  CHECK(std::memcmp(got.data(), data.data(), 777) == 0);
  CHECK(got[777] == 0xEE);
  CHECK(s >= 0.19);
  CHECK(s < 5.0);
  check_fd_state(b, nonblock);
  // the connection is still usable after a timeout
  send_all(a, data.data(), 10);
  r = demodel::recv_exact(b, got.data(), 10, 200, &calls);
  CHECK(r.status == 0 && r.bytes == 10);
  close(a);
  close(b);
}

static void on_usr1(int) {}

static void case_signal(bool nonblock) {
  struct sigaction sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.sa_handler = on_usr1;  // no SA_RESTART: blocked calls see EINTR
  sigemptyset(&sa.sa_mask);
  sigaction(SIGUSR1, &sa, nullptr);
  int a, b;
  tcp_pair(&a, &b);
  set_nonblock(b, nonblock);
  const size_t n = 200000;
  std::vector<uint8_t> data = pattern(n);
  pthread_t self = pthread_self();
  std::thread w([&] {
    usleep(20000);
    pthread_kill(self, SIGUSR1);  // arrives with nothing received yet
    usleep(20000);
    send_all(a, data.data(), n / 2);
    for (int i = 0; i < 3; i++) {
      usleep(10000);
      pthread_kill(self, SIGUSR1);  // arrives mid-body
    }
    send_all(a, data.data() + n / 2, n - n / 2);
  });
  std::vector<uint8_t> got(n, 0xEE);
  uint64_t calls = 0;
  IoResult r = demodel::recv_exact(b, got.data(), n, 2000, &calls);
  w.join();
  CHECK(r.status == 0);
  CHECK(r.bytes == n);
  CHECK(std::memcmp(got.data(), data.data(), n) == 0);
  check_fd_state(b, nonblock);
  close(a);
  close(b);
  signal(SIGUSR1, SIG_DFL);
}

// RecvSession lends a non-blocking fd to the blocking loop and gives it back
static void case_session() {
  int a, b;
  tcp_pair(&a, &b);
  set_nonblock(b, true);
  const size_t n = 100000;
  std::vector<uint8_t> data = pattern(n);
  std::thread w([&] {
    send_all(a, data.data(), n / 2);
    usleep(20000);
    send_all(a, data.data() + n / 2, n - n / 2);
    close(a);
  });
  std::vector<uint8_t> got(n + 100, 0xEE);
  uint64_t calls = 0;
  {
    demodel::RecvSession s(b, 2000);
    CHECK(!demodel::fd_nonblocking(b));
    IoResult r = s.recv(got.data(), n / 4, &calls);
    CHECK(r.status == 0 && r.bytes == n / 4);
    r = s.recv(got.data() + n / 4, n - n / 4 + 100, &calls);
    CHECK(r.status == demodel::kSockEof);
    CHECK(r.bytes == n - n / 4);
  }
  w.join();
  CHECK(std::memcmp(got.data(), data.data(), n) == 0);
  CHECK(got[n] == 0xEE);
  check_fd_state(b, true);
  close(b);
}

static int pattern_file(size_t n) {
  char path[] = "/tmp/sock_io_host_XXXXXX";
  int fd = mkstemp(path);
  if (fd < 0) {
    std::perror("mkstemp");
    std::exit(2);
  }
  unlink(path);
  std::vector<uint8_t> data = pattern(n);
  size_t off = 0;
  while (off < n) {
    ssize_t w = write(fd, data.data() + off, n - off);
    if (w <= 0) {
      std::perror("write");
      std::exit(2);
    }
    off += (size_t)w;
  }
  return fd;
}

static void case_sendfile_slow_reader(bool nonblock) {
  int a, b;
  tcp_pair(&a, &b);
  int small = 4096;
  setsockopt(a, SOL_SOCKET, SO_SNDBUF, &small, sizeof(small));
  set_nonblock(a, nonblock);
  const size_t file_n = 3u << 20, offset = 12345, length = file_n - 20000;
  int f = pattern_file(file_n);
  std::vector<uint8_t> got(length, 0xEE);
  size_t rgot = 0;
  std::thread rd([&] {
    while (rgot < length) {
      size_t c = 64 << 10;
      if (c > length - rgot) c = length - rgot;
      ssize_t n = recv(b, got.data() + rgot, c, 0);
      if (n <= 0) {
        if (n < 0 && errno == EINTR) continue;
        break;
      }
      rgot += (size_t)n;
      usleep(100);
    }
  });
  uint64_t calls = 0;
  IoResult r = demodel::sendfile_exact(a, f, (int64_t)offset, length, 2000,
                                       &calls);
  rd.join();
  CHECK(r.status == 0);
  CHECK(r.bytes == length);
  CHECK(rgot == length);
  std::vector<uint8_t> want = pattern(length, offset);
  CHECK(std::memcmp(got.data(), want.data(), length) == 0);
  CHECK(demodel::fd_nonblocking(a) == nonblock);
  struct timeval tv = {1, 1};
  socklen_t l = sizeof(tv);
  CHECK(getsockopt(a, SOL_SOCKET, SO_SNDTIMEO, &tv, &l) == 0 &&
        tv.tv_sec == 0 && tv.tv_usec == 0);
  // asking past the end of the file: short count, EOF status
  r = demodel::sendfile_exact(a, f, (int64_t)file_n - 10, 100, 2000, &calls);
  CHECK(r.status == demodel::kSockEof && r.bytes == 10);
  close(f);
  close(a);
  close(b);
}

static void case_sendfile_stalled_reader(bool nonblock) {
  int a, b;
  tcp_pair(&a, &b);
  int small = 4096;
  setsockopt(a, SOL_SOCKET, SO_SNDBUF, &small, sizeof(small));
  setsockopt(b, SOL_SOCKET, SO_RCVBUF, &small, sizeof(small));
  set_nonblock(a, nonblock);
  const size_t file_n = 8u << 20;
  int f = pattern_file(file_n);
  uint64_t calls = 0;
  IoResult r = demodel::sendfile_exact(a, f, 0, file_n, 200, &calls);
  CHECK(r.status == ETIMEDOUT);
  CHECK(r.bytes < file_n);
  // what was counted as sent is what the peer can read, in order
  set_nonblock(b, true);
  std::vector<uint8_t> got(file_n);
  size_t rgot = 0;
  for (;;) {
    ssize_t n = recv(b, got.data() + rgot, file_n - rgot, 0);
    if (n > 0) {
      rgot += (size_t)n;
      continue;
    }
    if (n < 0 && errno == EINTR) continue;
    if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK) &&
        rgot < r.bytes) {
      usleep(1000);
      continue;
    }
    break;
  }
  CHECK(rgot == r.bytes);
  std::vector<uint8_t> want = pattern(rgot);
  CHECK(std::memcmp(got.data(), want.data(), rgot) == 0);
  close(f);
  close(a);
  close(b);
}

static void case_sendfile_closed_peer(bool nonblock) {
  int a, b;
  tcp_pair(&a, &b);
  set_nonblock(a, nonblock);
  struct linger lg = {1, 0};  // close -> RST
  setsockopt(b, SOL_SOCKET, SO_LINGER, &lg, sizeof(lg));
  close(b);
  usleep(20000);
  const size_t file_n = 8u << 20;
  int f = pattern_file(file_n);
  uint64_t calls = 0;
  IoResult r = demodel::sendfile_exact(a, f, 0, file_n, 2000, &calls);
  CHECK(r.status == EPIPE || r.status == ECONNRESET);
  CHECK(r.bytes < file_n);
  // again on the now-dead socket: EPIPE as a status, the process survives
  r = demodel::sendfile_exact(a, f, 0, file_n, 2000, &calls);
  CHECK(r.status == EPIPE || r.status == ECONNRESET);
  close(f);
  close(a);
}

static void case_threads() {
  const int kThreads = 8;
  const size_t n = 1u << 20;
  int f = pattern_file(n);
  std::vector<uint8_t> want = pattern(n);
  std::vector<std::thread> ts;
  std::vector<int> bad(kThreads, 0);
  for (int t = 0; t < kThreads; t++) {
    ts.emplace_back([&, t] {
      for (int round = 0; round < 3; round++) {
        int a, b;
        tcp_pair(&a, &b);
        set_nonblock(a, (t + round) & 1);
        set_nonblock(b, t & 1);
        std::thread snd([&] {
          uint64_t c = 0;
          IoResult r = demodel::sendfile_exact(a, f, 0, n, 5000, &c);
          if (r.status != 0 || r.bytes != n) bad[t]++;
        });
        std::vector<uint8_t> got(n);
        uint64_t c = 0;
        IoResult r = demodel::recv_exact(b, got.data(), n, 5000, &c);
        snd.join();
        if (r.status != 0 || r.bytes != n ||
            std::memcmp(got.data(), want.data(), n) != 0)
          bad[t]++;
        close(a);
        close(b);
      }
    });
  }
  for (auto& t : ts) t.join();
  for (int t = 0; t < kThreads; t++) CHECK(bad[t] == 0);
  close(f);
  demodel::SockCounters& c = demodel::sock_counters();
  CHECK(c.recv_exact.load() >= (uint64_t)kThreads * 3);
  CHECK(c.sendfile_exact.load() >= (uint64_t)kThreads * 3);
}

static void case_descs() {
  const uint64_t M = 1u << 20;
  const uint64_t sizes[] = {0, 1, M - 1, M, M + 1, 3 * M + 5};
  const size_t n_t = sizeof(sizes) / sizeof(sizes[0]);
  std::vector<uint64_t> triples;
  uint64_t expect = 0;
  for (size_t i = 0; i < n_t; i++) {
    triples.push_back(1000 + i * 100 * M);     // src_off
    triples.push_back(0x7000000000ull + i * 64 * M);  // dst_ptr
    triples.push_back(sizes[i]);
    expect += (sizes[i] + M - 1) / M;
  }
  CHECK(demodel::scatter_desc_count(triples.data(), n_t, M) == expect);
  const uint64_t guard = 0xABCDABCDABCDABCDull;
  std::vector<uint64_t> out(expect * 4 + 8, guard);
  int64_t n = demodel::expand_scatter_descs(triples.data(), n_t, M,
                                            out.data(), expect);
  CHECK(n == (int64_t)expect);
  // the pieces tile each tensor exactly, in order
  size_t k = 0;
  for (size_t i = 0; i < n_t; i++) {
    uint64_t off = 0;
    while (off < sizes[i]) {
      const uint64_t* d = &out[k * 4];
      uint64_t len = sizes[i] - off < M ? sizes[i] - off : M;
      CHECK(d[0] == triples[3 * i] + off);
      CHECK(d[1] == triples[3 * i + 1] + off);
      CHECK(d[2] == len);
      CHECK(d[3] == 0);
      off += len;
      k++;
    }
  }
  CHECK(k == expect);
  for (size_t i = expect * 4; i < out.size(); i++) CHECK(out[i] == guard);
  // capacity one record short: an error, and nothing is written at all
  std::vector<uint64_t> small((expect - 1) * 4 + 8, guard);
  n = demodel::expand_scatter_descs(triples.data(), n_t, M, small.data(),
                                    expect - 1);
  CHECK(n < 0);
  for (size_t i = 0; i < small.size(); i++) CHECK(small[i] == guard);
  CHECK(demodel::expand_scatter_descs(triples.data(), n_t, 0, small.data(),
                                      expect) < 0);
  CHECK(demodel::expand_scatter_descs(triples.data(), 0, M, small.data(),
                                      0) == 0);
}

int main() {
  signal(SIGPIPE, SIG_IGN);
  for (int nb = 0; nb < 2; nb++) {
    case_small_writes(nb);
    case_peer_closes(nb);
    case_stalled_peer(nb);
    case_signal(nb);
    case_sendfile_slow_reader(nb);
    case_sendfile_stalled_reader(nb);
    case_sendfile_closed_peer(nb);
  }
  case_session();
  case_threads();
  case_descs();
  if (g_failed) {
    std::fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("sock_io OK\n");
  return 0;
}

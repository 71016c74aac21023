// _native bindings of csrc/sock_io.h: the receive loop of host landing and
// the sendfile loop of blob serving, each one GIL-free call.

#include <pybind11/pybind11.h>

#include <optional>
#include <stdexcept>

#include "sock_io.h"

namespace py = pybind11;

void register_sock_io(py::module_& m) {
  m.def(
      "recv_exact",
      [](int fd, py::buffer dst, size_t offset, size_t want,
         int stall_timeout_ms, bool blocking) {
        py::buffer_info info = dst.request(/*writable=*/true);
        size_t cap = (size_t)info.size * (size_t)info.itemsize;
        if (offset > cap || want > cap - offset)
          throw std::out_of_range("recv_exact: range exceeds the buffer");
        char* p = (char*)info.ptr + offset;
        demodel::IoResult r;
        uint64_t calls = 0;
        {
          py::gil_scoped_release nogil;
          if (blocking) {
            demodel::RecvSession s(fd, stall_timeout_ms);
            r = s.recv(p, want, &calls);
          } else {
            r = demodel::recv_exact(fd, p, want, stall_timeout_ms, &calls);
          }
        }
        return py::make_tuple(r.bytes, r.status, calls);
      },
      py::arg("fd"), py::arg("dst"), py::arg("offset"), py::arg("want"),
      py::arg("stall_timeout_ms"), py::arg("blocking") = true,
      "recv() `want` bytes into dst[offset:] without the GIL -> (bytes, "
      "status, recv calls); status 0 ok, -1 EOF, ETIMEDOUT stall, else "
      "errno.  blocking=True lends the fd to a blocking MSG_WAITALL loop "
      "and restores O_NONBLOCK after; False keeps the fd's mode");
  m.def(
      "sendfile_exact",
      [](int out_fd, int in_fd, int64_t offset, size_t length,
         int stall_timeout_ms, bool blocking) {
        demodel::IoResult r;
        uint64_t calls = 0;
        {
          py::gil_scoped_release nogil;
          std::optional<demodel::BlockingScope> scope;
          if (blocking) scope.emplace(out_fd);
          r = demodel::sendfile_exact(out_fd, in_fd, offset, length,
                                      stall_timeout_ms, &calls);
        }
        return py::make_tuple(r.bytes, r.status, calls);
      },
      py::arg("out_fd"), py::arg("in_fd"), py::arg("offset"),
      py::arg("length"), py::arg("stall_timeout_ms"),
      py::arg("blocking") = true,
      "sendfile() [offset, offset+length) of in_fd to a socket without the "
      "GIL -> (bytes, status, sendfile calls); statuses as recv_exact.  "
      "EPIPE is a status, never SIGPIPE");
  m.def("sock_stats", [] {
    demodel::SockCounters& c = demodel::sock_counters();
    py::dict d;
    d["recv_exact"] = c.recv_exact.load();
    d["recv_calls"] = c.recv_calls.load();
    d["sendfile_exact"] = c.sendfile_exact.load();
    d["sendfile_calls"] = c.sendfile_calls.load();
    return d;
  }, "native socket-loop counters of this extension since import");
}

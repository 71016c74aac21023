"""CPU loopback probe: Python vs native socket loops, both ends in one
process (as bench.py runs them).

N streams of S bytes each: a sender thread per stream sendfile()s a
page-cache file, a receiver thread per stream fills a ring of 4 x 32 MiB
buffers.  Variants per side:

  send  py      os.sendfile loop on a non-blocking fd + select (the old
                utils/netio.py loop)
        native  _native.sendfile_exact, fd blocking for the call
  recv  py      recv_into(MSG_WAITALL) on a timeout-mode socket (the
                BlobSource.fill path)
        native  _native.recv_exact, fd blocking for the call
        lowat   _native.recv_exact on the non-blocking fd (poll +
                SO_RCVLOWAT 4 MiB)

    python scripts/sock_loop_probe.py --streams 13 --gib 2 --reps 3

Prints one line per (send, recv) pair: GB/s per repetition and the recv /
sendfile calls per stream."""

import argparse
import os
import select
import socket
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(
    __file__))))

from demodel_amd.build import build_native  # noqa: E402

build_native()
from demodel_amd import _native  # noqa: E402

SLAB = 32 << 20
N_SLABS = 4


def send_py(sock, infd, length, calls):
    sock.setblocking(False)
    fd = sock.fileno()
    off = 0
    while off < length:
        calls[0] += 1
        try:
            n = os.sendfile(fd, infd, off, length - off)
        except BlockingIOError:
            select.select([], [fd], [], 10)
            continue
        if n == 0:
            raise ConnectionResetError
        off += n


def send_native(sock, infd, length, calls):
    sock.setblocking(False)  # asyncio's transports are non-blocking
    sent, status, c = _native.sendfile_exact(sock.fileno(), infd, 0, length,
                                             60_000)
    calls[0] += c
    assert status == 0 and sent == length, (sent, status)


def recv_py(sock, length, ring, calls):
    sock.settimeout(60)
    off = 0
    i = 0
    while off < length:
        want = min(SLAB, length - off)
        view = ring[i % N_SLABS][:want]
        got = 0
        while got < want:
            calls[0] += 1
            n = sock.recv_into(view[got:], want - got, socket.MSG_WAITALL)
            if n <= 0:
                raise ConnectionResetError
            got += n
        off += want
        i += 1


def _recv_native(blocking):
    def run(sock, length, ring, calls):
        sock.settimeout(60)
        fd = sock.fileno()
        off = 0
        i = 0
        while off < length:
            want = min(SLAB, length - off)
            n, status, c = _native.recv_exact(fd, ring[i % N_SLABS], 0, want,
                                              60_000, blocking)
            calls[0] += c
            assert status == 0 and n == want, (n, status)
            off += want
            i += 1
    return run


SENDERS = {"py": send_py, "native": send_native}
RECEIVERS = {"py": recv_py, "native": _recv_native(True),
             "lowat": _recv_native(False)}


def one_run(send, recv, streams, length, infd, rings):
    ls = socket.socket()
    ls.bind(("127.0.0.1", 0))
    ls.listen(streams)
    port = ls.getsockname()[1]
    s_calls = [[0] for _ in range(streams)]
    r_calls = [[0] for _ in range(streams)]
    errs = []

    def guard(fn, *a):
        try:
            fn(*a)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    pairs = []
    for _ in range(streams):
        c = socket.create_connection(("127.0.0.1", port))
        c.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 8 << 20)
        c.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        s, _ = ls.accept()
        pairs.append((s, c))
    ls.close()
    ts = []
    for k, (s, c) in enumerate(pairs):
        ts.append(threading.Thread(target=guard, args=(
            SENDERS[send], s, infd, length, s_calls[k])))
        ts.append(threading.Thread(target=guard, args=(
            RECEIVERS[recv], c, length, rings[k], r_calls[k])))
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    for s, c in pairs:
        s.close()
        c.close()
    if errs:
        raise errs[0]
    return (streams * length / dt / 1e9,
            sum(c[0] for c in r_calls) / streams,
            sum(c[0] for c in s_calls) / streams)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=13)
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", default="py:py,py:native,py:lowat,"
                    "native:py,native:native,native:lowat")
    args = ap.parse_args()
    length = int(args.gib * (1 << 30))
    infd = os.memfd_create("sock-loop-probe")
    block = os.urandom(8 << 20)
    off = 0
    while off < length:
        off += os.pwrite(infd, block[:min(len(block), length - off)], off)
    rings = [[memoryview(bytearray(SLAB)) for _ in range(N_SLABS)]
             for _ in range(args.streams)]
    print(f"{args.streams} streams x {args.gib} GiB, {args.reps} reps, "
          f"{os.cpu_count()} CPUs")
    print("| sender | receiver | GB/s | recv calls/stream | "
          "send calls/stream |")
    print("|---|---|---|---|---|")
    for pair in args.pairs.split(","):
        send, recv = pair.split(":")
        runs = [one_run(send, recv, args.streams, length, infd, rings)
                for _ in range(args.reps)]
        print(f"| {send} | {recv} | "
              + " / ".join(f"{r[0]:.2f}" for r in runs)
              + f" | {runs[-1][1]:.0f} | {runs[-1][2]:.0f} |", flush=True)


if __name__ == "__main__":
    main()

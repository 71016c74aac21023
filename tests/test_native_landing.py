"""The native socket loops on the CPU landing target.

HostLander.land_into hands plain-TCP Content-Length bodies to
_native.recv_exact and the origin serves them through
_native.sendfile_exact; DEMODEL_NATIVE_SOCK=0 restores the Python loops.
Which path ran is shown by the counters the binding exposes
(_native.sock_stats), never by timing."""

import hashlib
import os
import socket
import threading

import pytest

from demodel_amd import _native
from demodel_amd.engine import fetch
from demodel_amd.engine import pull as pull_mod
from demodel_amd.engine.formats import safetensors as st
from demodel_amd.engine.pipeline import HostLander, LandingError
from helpers import Stack, host_landers


@pytest.fixture()
def stack(tmp_path):
    s = Stack(tmp_path)
    yield s
    s.close()


def _stats():
    return dict(_native.sock_stats())


def _two_shard_model(tmp_path):
    files = {}
    raw = {}
    for i, n in enumerate((700_001, 300_017)):
        body = os.urandom(n)
        head, _ = st.build_header({f"w{i}": ("U8", (n,), n)})
        p = tmp_path / f"model-{i:05d}-of-00002.safetensors"
        p.write_bytes(head + body)
        files[p.name] = str(p)
        raw[p.name] = head + body
    return files, raw


def _pull(stack, repo, names):
    """Each file through _pull_blob without a segment executor (what
    bench.py's fan-out step does): the resumable land_into path on every
    machine, where pull_hf would pick range probing on GPU boxes."""
    landers = host_landers(slab_bytes=256 << 10)
    out = {}
    for name in names:
        pf = pull_mod._pull_blob(
            landers, name,
            f"{stack.origin_base}/{repo}/resolve/main/{name}",
            None, "chunked", None, False)
        out[name] = (bytes(pf.blob.buffer), pf.blob.digest_blob,
                     bytes(pf.blob.head))
    return out


def test_switch_on_and_off_land_identical_bytes(stack, tmp_path,
                                                monkeypatch):
    files, raw = _two_shard_model(tmp_path)
    stack.origin.add_hf_repo("org/two", files)

    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "1")
    s0 = _stats()
    on = _pull(stack, "org/two", sorted(files))
    s1 = _stats()
    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "0")
    off = _pull(stack, "org/two", sorted(files))
    s2 = _stats()

    assert on == off
    for name, data in raw.items():
        body, digests, head = on[name]
        assert body == data
        assert head == data[:len(head)] and len(head) == len(data)
        assert digests == b"".join(
            hashlib.sha256(data[o:o + (64 << 10)]).digest()
            for o in range(0, len(data), 64 << 10))
    # both ends ran natively with the switch on, neither with it off
    assert s1["recv_exact"] > s0["recv_exact"]
    assert s1["sendfile_exact"] >= s0["sendfile_exact"] + 2
    assert s2["recv_exact"] == s1["recv_exact"]
    assert s2["sendfile_exact"] == s1["sendfile_exact"]


@pytest.mark.parametrize("side", ["recv", "send"])
def test_switch_selects_one_side(stack, tmp_path, monkeypatch, side):
    files, raw = _two_shard_model(tmp_path)
    stack.origin.add_hf_repo("org/side", files)
    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", side)
    s0 = _stats()
    got = _pull(stack, "org/side", sorted(files))
    s1 = _stats()
    assert {n: v[0] for n, v in got.items()} == raw
    assert (s1["recv_exact"] > s0["recv_exact"]) == (side == "recv")
    assert (s1["sendfile_exact"] > s0["sendfile_exact"]) == (side == "send")


def test_drop_mid_body_resumes_to_identical_bytes(stack, tmp_path,
                                                  monkeypatch):
    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "1")
    data = os.urandom(2 << 20)
    p = tmp_path / "big.bin"
    p.write_bytes(data)
    stack.origin.add_hf_repo("org/drop", {"big.bin": str(p)})
    stack.origin.drop_once["big.bin"] = 300 << 10
    s0 = _stats()
    got = _pull(stack, "org/drop", ["big.bin"])
    s1 = _stats()
    body, digests, head = got["big.bin"]
    assert body == data
    assert head == data[:len(head)] and len(head) == len(data)
    assert not stack.origin.drop_once  # the fault fired
    assert s1["recv_exact"] > s0["recv_exact"]
    blob_gets = [r for r in stack.origin.requests
                 if r.startswith("GET") and "big.bin" in r and "/cdn/" in r]
    assert len(blob_gets) == 2  # original + one Range resume


# ---- hand-made responses over a raw loopback server ---------------------

class _RawServer:
    """Accepts one connection, reads the request head, then runs
    `serve(conn)` on its thread."""

    def __init__(self, serve):
        self._ls = socket.socket()
        self._ls.bind(("127.0.0.1", 0))
        self._ls.listen(1)
        self.port = self._ls.getsockname()[1]
        self._serve = serve
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()

    def _run(self):
        conn, _ = self._ls.accept()
        try:
            buf = b""
            while b"\r\n\r\n" not in buf:
                d = conn.recv(65536)
                if not d:
                    return
                buf += d
            self._serve(conn)
        finally:
            conn.close()
            self._ls.close()

    def join(self):
        self._t.join(10)


def _land(port, nbytes, slab=64 << 10, **kw):
    src = fetch.http_get(f"http://127.0.0.1:{port}/x", timeout=5.0)
    try:
        lander = HostLander(slab_bytes=slab)
        buf = lander.alloc(nbytes)
        head, _ = lander.land_into(buf, 0, src.fill, nbytes, keep_head=True,
                                   **kw)
        return bytes(buf), bytes(head), src
    finally:
        src.close()


def test_leftover_after_the_head_lands_intact(monkeypatch):
    """Body bytes that arrive in the same segment as the response head
    reach the buffer through fill(); the native loop takes over after."""
    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "1")
    data = os.urandom(200_003)
    gate = threading.Event()

    def serve(conn):
        head = (f"HTTP/1.1 200 OK\r\nContent-Length: {len(data)}\r\n"
                "\r\n").encode()
        conn.sendall(head + data[:1000])  # one write: head + 1000 B
        gate.wait(5)
        conn.sendall(data[1000:])

    srv = _RawServer(serve)
    src = fetch.http_get(f"http://127.0.0.1:{srv.port}/x", timeout=5.0)
    try:
        # the head was read before any later byte was sent, so exactly
        # the first write's tail is the leftover
        assert src.leftover_pending()
        assert src.native_body() is None
        gate.set()
        s0 = _stats()
        lander = HostLander(slab_bytes=64 << 10)
        buf = lander.alloc(len(data))
        head, _ = lander.land_into(buf, 0, src.fill, len(data),
                                   keep_head=True)
        s1 = _stats()
    finally:
        src.close()
    srv.join()
    assert bytes(buf) == data
    assert bytes(head) == data
    assert s1["recv_exact"] > s0["recv_exact"]
    assert src.native_body() is None or src.native_body()[1] == 0


def test_chunked_body_takes_the_python_path(monkeypatch):
    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "1")
    data = os.urandom(150_001)

    def serve(conn):
        conn.sendall(b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n"
                     b"\r\n")
        for o in range(0, len(data), 40_000):
            piece = data[o:o + 40_000]
            conn.sendall(f"{len(piece):x}\r\n".encode() + piece + b"\r\n")
        conn.sendall(b"0\r\n\r\n")

    srv = _RawServer(serve)
    s0 = _stats()
    body, head, src = _land(srv.port, len(data))
    s1 = _stats()
    srv.join()
    assert body == data and head == data
    assert not src.native_eligible and src.native_body() is None
    assert s1["recv_exact"] == s0["recv_exact"]
    assert s1["recv_calls"] == s0["recv_calls"]


def test_host_chain_takes_the_python_path(monkeypatch):
    """Exact-digest landings hash slab by slab in Python: no native call
    even on a plain Content-Length body."""
    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "1")
    data = os.urandom(100_000)

    def serve(conn):
        conn.sendall((f"HTTP/1.1 200 OK\r\nContent-Length: {len(data)}"
                      "\r\n\r\n").encode())
        conn.sendall(data)

    srv = _RawServer(serve)
    chain = hashlib.sha256()
    s0 = _stats()
    body, _, _ = _land(srv.port, len(data), chain=chain)
    s1 = _stats()
    srv.join()
    assert body == data
    assert chain.hexdigest() == hashlib.sha256(data).hexdigest()
    assert s1["recv_exact"] == s0["recv_exact"]


def test_native_short_body_raises_landing_error(monkeypatch):
    """A peer that closes early: LandingError counts whole slabs only,
    and they hold the sent prefix."""
    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "1")
    slab = 64 << 10
    data = os.urandom(5 * slab)
    sent = 2 * slab + 100

    def serve(conn):
        conn.sendall((f"HTTP/1.1 200 OK\r\nContent-Length: {len(data)}"
                      "\r\n\r\n").encode())
        conn.sendall(data[:sent])

    srv = _RawServer(serve)
    src = fetch.http_get(f"http://127.0.0.1:{srv.port}/x", timeout=5.0)
    lander = HostLander(slab_bytes=slab)
    buf = lander.alloc(len(data))
    try:
        with pytest.raises(LandingError) as ei:
            lander.land_into(buf, 0, src.fill, len(data))
    finally:
        src.close()
    srv.join()
    assert ei.value.landed == 2 * slab
    assert bytes(buf[:2 * slab]) == data[:2 * slab]

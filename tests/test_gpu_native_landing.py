"""PinnedPool.land_fd and the native scatter descriptors on the GPU.

Bodies come from a loopback socket into tiny rings (64 KiB x 2 slabs), so
5*slab+3 bytes wrap the ring and reuse fenced slots.  Every case reads
HBM back and compares with the sent bytes; the error case is a socket
error on the host (a sender that closes early)."""

import hashlib
import os
import socket
import threading

import pytest

pytestmark = pytest.mark.gpu

SLAB = 64 << 10
HEAD = SLAB + 1000   # the head capture spans more than one slab
VC = 4096            # verify chunk: many chunks even in the small cases
SIZES = [1, SLAB - 1, SLAB, SLAB + 1, 5 * SLAB + 3]


class _RawServer:
    """One connection: read the request head, send a Content-Length
    response whose first write carries `with_head` body bytes, stop after
    `send_bytes` of the body."""

    def __init__(self, data, send_bytes=None, with_head=0):
        self._ls = socket.socket()
        self._ls.bind(("127.0.0.1", 0))
        self._ls.listen(1)
        self.port = self._ls.getsockname()[1]
        self._data = data
        self._send = len(data) if send_bytes is None else send_bytes
        self._with_head = with_head
        self.gate = threading.Event()
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
            head = (f"HTTP/1.1 200 OK\r\nContent-Length: "
                    f"{len(self._data)}\r\n\r\n").encode()
            k = min(self._with_head, self._send)
            conn.sendall(head + self._data[:k])
            if self._with_head:
                self.gate.wait(5)  # the client has parsed the head
            conn.sendall(self._data[k:self._send])
        finally:
            conn.close()
            self._ls.close()

    def join(self):
        self._t.join(10)


def _lander():
    from demodel_amd.engine.pipeline import Lander

    return Lander(slab_bytes=SLAB, n_slabs=2, verify_chunk=VC,
                  head_bytes=HEAD)


def _zeroed(lander, nbytes):
    import torch

    buf = lander._h.DeviceBuffer(nbytes)
    torch.from_dlpack(buf.to_dlpack()).zero_()
    torch.cuda.synchronize()
    return buf


def _readback(buf):
    import torch

    return torch.from_dlpack(buf.to_dlpack()).cpu().numpy().tobytes()


def _chunk_digests(data):
    return b"".join(hashlib.sha256(data[o:o + VC]).digest()
                    for o in range(0, len(data), VC))


@pytest.fixture(autouse=True)
def _native_on(monkeypatch):
    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "1")


@pytest.mark.parametrize("base_off", [0, 13])
@pytest.mark.parametrize("nbytes", SIZES)
def test_land_fd_sizes_and_offsets(nbytes, base_off):
    from demodel_amd.engine import fetch
    from demodel_amd.gpu import hip

    data = os.urandom(nbytes)
    srv = _RawServer(data)
    lander = _lander()
    total = base_off + nbytes
    buf = _zeroed(lander, total + 16)
    src = fetch.http_get(f"http://127.0.0.1:{srv.port}/x", timeout=5.0)
    try:
        n0 = hip().sock_stats()["land_fd"]
        head, _ = lander.land_into(buf, base_off, src.fill, nbytes,
                                   keep_head=True)
        lander.sync()
        assert hip().sock_stats()["land_fd"] == n0 + 1
    finally:
        src.close()
    srv.join()
    want = bytes(base_off) + data + bytes(16)
    assert _readback(buf) == want  # nothing before, nothing after
    assert bytes(head) == data[:HEAD]
    assert lander.finish_verify(buf, total, VC) == _chunk_digests(
        want[:total])


def test_land_fd_leftover_goes_through_the_first_slab():
    from demodel_amd.engine import fetch

    nbytes = 5 * SLAB + 3
    data = os.urandom(nbytes)
    srv = _RawServer(data, with_head=1000)
    lander = _lander()
    buf = _zeroed(lander, nbytes)
    src = fetch.http_get(f"http://127.0.0.1:{srv.port}/x", timeout=5.0)
    try:
        assert src.leftover_pending()
        srv.gate.set()
        head, _ = lander.land_into(buf, 0, src.fill, nbytes, keep_head=True)
        lander.sync()
    finally:
        src.close()
    srv.join()
    assert _readback(buf) == data
    assert bytes(head) == data[:HEAD]
    assert lander.finish_verify(buf, nbytes, VC) == _chunk_digests(data)


def test_switch_off_lands_the_same_bytes(monkeypatch):
    from demodel_amd.engine import fetch
    from demodel_amd.gpu import hip

    monkeypatch.setenv("DEMODEL_NATIVE_SOCK", "0")
    nbytes = 5 * SLAB + 3
    data = os.urandom(nbytes)
    srv = _RawServer(data)
    lander = _lander()
    buf = _zeroed(lander, nbytes)
    src = fetch.http_get(f"http://127.0.0.1:{srv.port}/x", timeout=5.0)
    try:
        n0 = hip().sock_stats()["land_fd"]
        head, _ = lander.land_into(buf, 0, src.fill, nbytes, keep_head=True)
        lander.sync()
        assert hip().sock_stats()["land_fd"] == n0  # the Python loop ran
    finally:
        src.close()
    srv.join()
    assert _readback(buf) == data
    assert bytes(head) == data[:HEAD]


def test_sender_closing_early_then_resume():
    from demodel_amd.engine import fetch
    from demodel_amd.engine.pipeline import LandingError

    nbytes = 5 * SLAB + 3
    sent = 2 * SLAB + 100
    data = os.urandom(nbytes)
    srv = _RawServer(data, send_bytes=sent)
    lander = _lander()
    buf = _zeroed(lander, nbytes)
    src = fetch.http_get(f"http://127.0.0.1:{srv.port}/x", timeout=5.0)
    try:
        with pytest.raises(LandingError) as ei:
            lander.land_into(buf, 0, src.fill, nbytes, keep_head=True)
        lander.sync()
    finally:
        src.close()
    srv.join()
    landed = ei.value.landed
    # whole slabs only: never more than what was submitted to the GPU
    assert 0 < landed <= 2 * SLAB
    assert _readback(buf)[:landed] == data[:landed]

    # a second landing from `landed` (what a Range resume serves)
    srv2 = _RawServer(data[landed:])
    src2 = fetch.http_get(f"http://127.0.0.1:{srv2.port}/x", timeout=5.0)
    try:
        lander.land_into(buf, landed, src2.fill, nbytes - landed)
        lander.sync()
    finally:
        src2.close()
    srv2.join()
    assert _readback(buf) == data
    assert lander.finish_verify(buf, nbytes, VC) == _chunk_digests(data)


def test_load_into_native_descriptors_match_views():
    import torch

    from demodel_amd.engine.formats import safetensors as st
    from demodel_amd.engine.loader import load_into
    from demodel_amd.engine.pipeline import Lander

    m = 1 << 20
    sizes = [0, 1, m - 1, m, m + 1, 3 * m + 5]
    spec = {f"t{i}": ("U8", (n,), n) for i, n in enumerate(sizes)}
    head, _ = st.build_header(spec)
    body = os.urandom(sum(sizes))
    raw = head + body
    lander = Lander(slab_bytes=1 << 20, n_slabs=2)
    pos = [0]

    def fill(view):
        n = min(len(view), len(raw) - pos[0])
        view[:n] = raw[pos[0]:pos[0] + n]
        pos[0] += n
        return n

    blob = lander.land(fill, len(raw), verify=False)
    hdr = st.parse_header(blob.head)
    views = st.torch_views(hdr, blob.torch_u8())
    targets = {f"t{i}": torch.full((n,), 0xEE, dtype=torch.uint8,
                                   device="cuda")
               for i, n in enumerate(sizes)}
    loaded = load_into(blob, hdr, targets)
    assert sorted(loaded) == sorted(targets)
    off = 0
    for i, n in enumerate(sizes):
        got = targets[f"t{i}"].cpu()
        assert torch.equal(got, views[f"t{i}"].cpu())
        assert got.numpy().tobytes() == body[off:off + n]
        off += n

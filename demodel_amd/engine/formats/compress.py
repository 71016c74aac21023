"""GPU decompression front-end: zstd, snappy, raw DEFLATE (gzip) and LZ4.

Drives the wave-per-stream kernels (csrc/zstd_kernel.hip, snappy.hip,
inflate.hip, lz4.hip) over batches of compressed regions already
resident in HBM: cached response bodies in their original
Content-Encoding (reference CONTRIBUTING.md:116), gzip members and zstd
frames of dataset streams, parquet page payloads.  One DecompressJob
runs any mix of the codecs on one stream.
"""

from __future__ import annotations

import ctypes
import struct
from dataclasses import dataclass, field

DESC_WORDS = 8  # u64s per stream descriptor (csrc/lz_window.h)
ZSTD_WS_BYTES = 144 << 10

ERR = {0: "ok", -1: "magic", -2: "format", -3: "overflow",
       -4: "underrun", -5: "dictionary-unsupported"}


def gzip_deflate_offset(head: bytes) -> int:
    """Offset of the raw DEFLATE stream inside a gzip member (RFC 1952)."""
    if len(head) < 10 or head[:2] != b"\x1f\x8b":
        raise ValueError("not gzip (bad magic)")
    if head[2] != 8:
        raise ValueError(f"unsupported gzip method {head[2]}")
    flg = head[3]
    off = 10
    if flg & 0x04:  # FEXTRA
        xlen = struct.unpack_from("<H", head, off)[0]
        off += 2 + xlen
    if flg & 0x08:  # FNAME
        off = head.index(b"\0", off) + 1
    if flg & 0x10:  # FCOMMENT
        off = head.index(b"\0", off) + 1
    if flg & 0x02:  # FHCRC
        off += 2
    return off


@dataclass
class InflateResult:
    written: int
    status: int
    consumed: int

    @property
    def ok(self) -> bool:
        return self.status == 0

    @property
    def error(self) -> str | None:
        return None if self.ok else ERR.get(self.status, str(self.status))


def pack_descs(desc, streams, ws_ptr: int = 0) -> None:
    """Write one 8-u64 descriptor per (src, len, dst, cap) stream into
    the writable buffer desc.  ws_ptr, when non-zero, is the base of a
    workspace of ZSTD_WS_BYTES per stream; each stream's share goes in
    word 7 (zstd), which the other kernels ignore."""
    for i, (src, slen, dst, cap) in enumerate(streams):
        struct.pack_into("<8Q", desc, i * DESC_WORDS * 8,
                         src, slen, dst, cap, 0, 0, 0,
                         ws_ptr + i * ZSTD_WS_BYTES if ws_ptr else 0)


def parse_results(desc, n: int) -> list[InflateResult]:
    """The (written, status, consumed) words the kernel left in each of
    n descriptors; status is a signed int64."""
    out = []
    for i in range(n):
        written, status, consumed = struct.unpack_from(
            "<QqQ", desc, (i * DESC_WORDS + 4) * 8)
        out.append(InflateResult(written=written, status=status,
                                 consumed=consumed))
    return out


def check_results(results, what: str = "GPU page decompress") -> None:
    bad = [(i, r) for i, r in enumerate(results) if not r.ok]
    if bad:
        raise IOError(f"{what} failed: {bad[:3]}")


# codec -> its _hip launch; the order is the order of a job's results
CODECS = {
    "zstd": lambda h, desc, n, stream, window:
        h.zstd_frames(desc, n, stream, window=window),
    "snappy": lambda h, desc, n, stream, window:
        h.snappy_streams(desc, n, stream),
    "deflate": lambda h, desc, n, stream, window:
        h.inflate_streams(desc, n, stream),
    "lz4": lambda h, desc, n, stream, window:
        h.lz4_streams(desc, n, stream),
}


class DecompressJob:
    """An in-flight GPU decompression batch on its own HIP stream: the
    launch returns immediately so several batches (e.g. dataset shards
    landing at different times) decode CONCURRENTLY, which keeps wave
    occupancy high even when each batch alone has fewer frames than the
    chip has wave slots.  streams maps a codec of CODECS to its
    (src_ptr, src_len, dst_ptr, dst_cap) device regions; each non-empty
    codec is one kernel launch.  pre_launch(stream_handle), when given,
    queues extra async work (device copies) on the same stream before
    the kernels; post_launch(stream_handle) mirrors it after them (work
    that consumes the decompressed bytes, e.g. the parquet column
    decode).  window selects the zstd kernel's LDS window."""

    def __init__(self, streams: dict[str, list[tuple[int, int, int, int]]],
                 pre_launch=None, post_launch=None, window: int = 0):
        from ...gpu import hip

        unknown = set(streams) - set(CODECS)
        if unknown:
            raise ValueError(f"unknown codec(s) {sorted(unknown)}")
        h = hip()
        self._s = h.Stream(0)
        self._slabs = {}     # codec -> (pinned slab, n, device buffers)
        self._results = None
        if pre_launch is not None:
            pre_launch(self._s.handle)
        for codec, launch in CODECS.items():
            if streams.get(codec):
                self._launch(h, codec, launch, streams[codec], window)
        if post_launch is not None:
            post_launch(self._s.handle)
        self._ev = h.Event()
        self._ev.record(self._s.handle)

    def _launch(self, h, codec, launch, streams, window) -> None:
        n = len(streams)
        nd = n * DESC_WORDS * 8
        handle = self._s.handle
        ws = h.DeviceBuffer(n * ZSTD_WS_BYTES) if codec == "zstd" else None
        # PINNED staging for the descriptor block: hipMemcpyAsync
        # to/from pageable memory BLOCKS the host thread until every
        # prior op on the stream (the kernel!) completes, which would
        # make this "async" launch synchronous
        pin = h.PinnedPool(nd, 1)
        pack_descs(pin.slab_view(0), streams, ws.ptr if ws else 0)
        dbuf = h.DeviceBuffer(nd)
        addr = pin.slab_ptr(0)
        h.h2d_async(dbuf.ptr, addr, nd, handle)
        launch(h, dbuf.ptr, n, handle, window)
        h.d2h_async(addr, dbuf.ptr, nd, handle)
        self._slabs[codec] = (pin, n, dbuf, ws)

    def done(self) -> bool:
        return self._ev.query()

    def results(self, codec: str) -> list[InflateResult]:
        """One codec's results, in the order its streams were given."""
        if self._results is None:
            self._s.sync()
            self._results = {
                c: parse_results(pin.slab_view(0), n)
                for c, (pin, n, _, _) in self._slabs.items()}
        return self._results.get(codec, [])

    def wait(self) -> list[InflateResult]:
        """Every result, codec by codec in CODECS order."""
        return [r for codec in CODECS for r in self.results(codec)]

    def view(self, ranges: dict[str, tuple[int, int]]) -> "JobView":
        return JobView(self, ranges)


class JobView:
    """Per-codec ranges {codec: (lo, n)} of a (possibly shared)
    DecompressJob — several shards coalesced into ONE launch each hold
    a view of it.  wait() returns this view's results codec by codec in
    CODECS order."""

    def __init__(self, job, ranges: dict[str, tuple[int, int]]):
        self._job, self._ranges = job, ranges

    def done(self) -> bool:
        return self._job.done()

    def wait(self) -> list[InflateResult]:
        res = []
        for codec in CODECS:
            lo, n = self._ranges.get(codec, (0, 0))
            if n:
                res += self._job.results(codec)[lo:lo + n]
        return res


@dataclass
class DecompressPlan:
    """What one DecompressJob is to do for a landed blob: streams per
    codec, (dst, src, n) device copies for what is stored uncompressed,
    the HBM ring everything lands in and the (offset, size) span of each
    unit (page, frame) in it."""
    streams: dict = field(
        default_factory=lambda: {codec: [] for codec in CODECS})
    copies: list = field(default_factory=list)
    ring: object = None
    spans: list = field(default_factory=list)

    def queue_copies(self, stream_handle) -> None:
        """The job's pre_launch hook: the copies, async on its stream."""
        from ...gpu import hip

        h = hip()
        for dst, src, n in self.copies:
            h.d2d_async(dst, src, n, stream_handle)

    def absorb(self, other: "DecompressPlan") -> dict[str, tuple[int, int]]:
        """Append other's streams and copies (ring and spans stay its
        own); returns where they went as {codec: (lo, n)}, which is what
        a view of the merged job takes."""
        ranges = {}
        for codec, mine in self.streams.items():
            theirs = other.streams.get(codec, [])
            ranges[codec] = (len(mine), len(theirs))
            mine += theirs
        self.copies += other.copies
        return ranges


def _decompress(codec: str, streams, window: int = 0):
    if not streams:
        return []
    return DecompressJob({codec: streams}, window=window).wait()


def inflate_gpu(streams: list[tuple[int, int, int, int]]
                ) -> list[InflateResult]:
    """Inflate raw DEFLATE streams on the GPU (csrc/inflate.hip).

    streams: (src_ptr, src_len, dst_ptr, dst_cap) device addresses.
    Returns per-stream InflateResult; callers check .ok."""
    return _decompress("deflate", streams)


def zstd_gpu(frames: list[tuple[int, int, int, int]],
             window: int = 0) -> list[InflateResult]:
    """Decompress zstd frames on the GPU (csrc/zstd_kernel.hip); the
    job allocates the 144 KiB workspace each frame needs."""
    return _decompress("zstd", frames, window)


def lz4_gpu(streams: list[tuple[int, int, int, int]]
            ) -> list[InflateResult]:
    """Decompress raw LZ4 blocks on the GPU (csrc/lz4.hip) — parquet's
    LZ4/LZ4_RAW page codecs."""
    return _decompress("lz4", streams)


def snappy_gpu(streams: list[tuple[int, int, int, int]]
               ) -> list[InflateResult]:
    """Decompress raw snappy streams on the GPU (csrc/snappy.hip)."""
    return _decompress("snappy", streams)


def gunzip_blob_gpu(blob, out_size: int | None = None):
    """Decompress a gzip blob landed in HBM -> new DeviceBuffer.

    Uses the gzip ISIZE trailer for sizing (mod 2^32; capacity doubles on
    overflow).  Single-member fast path; multi-member walks `consumed`.
    """
    from ...gpu import hip

    h = hip()
    off = gzip_deflate_offset(blob.head)
    if out_size is None:
        tail = bytearray(8)
        addr = ctypes.addressof((ctypes.c_char * 8).from_buffer(tail))
        s = h.Stream(0)
        h.d2h_async(addr, blob.buffer.ptr + blob.nbytes - 8, 8, s.handle)
        s.sync()
        out_size = struct.unpack("<I", bytes(tail[4:8]))[0]
        if out_size == 0:
            out_size = 1
    cap = out_size
    for _ in range(3):
        dst = h.DeviceBuffer(cap)
        res = inflate_gpu([(blob.buffer.ptr + off,
                            blob.nbytes - off - 8, dst.ptr, cap)])[0]
        if res.ok:
            return dst, res
        if res.status == -3:  # overflow: ISIZE wrapped (>4 GiB payloads)
            cap *= 4
            continue
        raise IOError(f"GPU inflate failed: {res.error}")
    raise IOError("GPU inflate: capacity growth exhausted")

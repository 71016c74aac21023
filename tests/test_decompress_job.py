"""Host side of the GPU decompression job (engine/formats/compress.py):
descriptor packing and result parsing, merging plans into one launch and
viewing one contributor's results, and the build's rebuild triggers for
the headers the codec kernels share.  No GPU."""

import os
import re
import struct

from demodel_amd import build
from demodel_amd.engine.formats import compress as cz


def test_descriptor_pack_parse_round_trip():
    streams = [(0x1000, 10, 0x9000, 100), (0x2000, 20, 0xA000, 200),
               (0x3000, 30, 0xB000, 300)]
    ws = 0x7F00_0000_0000
    desc = bytearray(len(streams) * cz.DESC_WORDS * 8)
    cz.pack_descs(desc, streams, ws)
    for i, st in enumerate(streams):
        words = struct.unpack_from("<8Q", desc, i * 64)
        assert words[:4] == st
        assert words[4:7] == (0, 0, 0)
        assert words[7] == ws + i * cz.ZSTD_WS_BYTES   # zstd's workspace
    plain = bytearray(len(desc))
    cz.pack_descs(plain, streams)
    assert all(struct.unpack_from("<8Q", plain, i * 64)[7] == 0
               for i in range(3))

    # what the kernel writes back: written, status (int64), consumed
    struct.pack_into("<3Q", desc, 0 * 64 + 32, 100, 0, 10)
    struct.pack_into("<3Q", desc, 1 * 64 + 32, 7, 0xFFFF_FFFF_FFFF_FFFD, 5)
    struct.pack_into("<3Q", desc, 2 * 64 + 32, 300, 0, 30)
    res = cz.parse_results(desc, 3)
    assert [(r.written, r.status, r.consumed) for r in res] == [
        (100, 0, 10), (7, -3, 5), (300, 0, 30)]
    assert [r.ok for r in res] == [True, False, True]
    assert res[1].error == "overflow"
    # the inputs are still what was packed
    assert struct.unpack_from("<4Q", desc, 64) == streams[1]


class _FakeJob:
    def __init__(self, per_codec):
        self._per = per_codec

    def done(self):
        return True

    def results(self, codec):
        return self._per.get(codec, [])


def test_plan_merge_ranges_and_view_order():
    counts = {"zstd": (2, 0, 3), "snappy": (0, 4, 1),
              "deflate": (1, 0, 0), "lz4": (0, 0, 2)}
    plans = []
    for p in range(3):
        plan = cz.DecompressPlan(ring=f"ring{p}", spans=[(p, p)])
        for codec, ns in counts.items():
            plan.streams[codec] += [(codec, p, k, 0) for k in range(ns[p])]
        plan.copies += [(p, p, p)] * p
        plans.append(plan)

    merged = cz.DecompressPlan()
    ranges = [merged.absorb(plan) for plan in plans]
    assert list(merged.streams) == ["zstd", "snappy", "deflate", "lz4"]
    assert {c: len(s) for c, s in merged.streams.items()} == {
        "zstd": 5, "snappy": 5, "deflate": 1, "lz4": 2}
    assert merged.copies == [(1, 1, 1), (2, 2, 2), (2, 2, 2)]
    assert ranges[2] == {"zstd": (2, 3), "snappy": (4, 1),
                         "deflate": (1, 0), "lz4": (0, 2)}
    for plan, rng in zip(plans, ranges):
        for codec, (lo, n) in rng.items():
            assert merged.streams[codec][lo:lo + n] == plan.streams[codec]
        # merging took nothing from the contributor
        assert plan.ring is not None and len(plan.spans) == 1

    # one fabricated result per merged stream, tagged with its stream
    job = _FakeJob({c: [("res",) + s for s in merged.streams[c]]
                    for c in merged.streams})
    for p, rng in enumerate(ranges):
        got = cz.JobView(job, rng).wait()
        want = [("res", codec, p, k, 0)
                for codec in ("zstd", "snappy", "deflate", "lz4")
                for k in range(counts[codec][p])]
        assert got == want
    assert cz.JobView(job, ranges[0]).done()


def test_every_included_header_is_a_rebuild_trigger():
    include = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
    sources = list(build.HIP_SRCS) + list(build.NATIVE_SRCS)
    assert sources
    for src in sources:
        text = open(os.path.join(build.CSRC, src)).read()
        triggers = build._with_hdrs(src)
        assert triggers[0] == os.path.join(build.CSRC, src)
        for hdr in include.findall(text):
            path = os.path.join(build.CSRC, hdr)
            if os.path.exists(path):
                assert path in triggers, f"{src} includes {hdr}"

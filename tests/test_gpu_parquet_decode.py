"""GPU parquet column decode (csrc/parquet_decode.hip) against the scalar
reference of tests/parquet_ref.py and against pyarrow: bare hybrid
streams at every bit width, whole files in every write variant, and
damaged pages that must end in an IOError instead of a stray access."""

import ctypes
import struct

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.parquet as pq  # noqa: E402

import parquet_ref as ref  # noqa: E402
from demodel_amd.engine.formats import parquet as pqf  # noqa: E402

pytestmark = pytest.mark.gpu


def _upload(h, stream, data: bytes):
    buf = h.DeviceBuffer(max(len(data), 1))
    if data:
        host = bytearray(data)
        addr = ctypes.addressof((ctypes.c_char * len(host)).from_buffer(host))
        h.h2d_async(buf.ptr, addr, len(host), stream.handle)
        stream.sync()
    return buf


def _download(h, stream, ptr: int, n: int) -> bytes:
    out = bytearray(max(n, 1))
    addr = ctypes.addressof((ctypes.c_char * len(out)).from_buffer(out))
    if n:
        h.d2h_async(addr, ptr, n, stream.handle)
        stream.sync()
    return bytes(out[:n])


# ---------------------------------------------------------------------------
# kernel level: bare hybrid streams

def _run_hybrid(streams, max_blocks=0):
    """streams: [(bytes, bw, count, limit)] -> [(status, [values])]"""
    from demodel_amd.gpu import have_gpu, hip

    assert have_gpu()
    h = hip()
    s = h.Stream(0)
    src = b"".join(st[0] for st in streams)
    sbuf = _upload(h, s, src)
    n_out = sum(st[2] for st in streams)
    # every value slot starts as a sentinel no stream can produce twice
    obuf = _upload(h, s, b"\xA5" * (4 * n_out))
    desc = bytearray()
    so = oo = 0
    for data, bw, count, limit in streams:
        desc += struct.pack("<8Q", sbuf.ptr + so, len(data),
                            obuf.ptr + 4 * oo, count, bw, limit, 1, 0)
        so += len(data)
        oo += count
    dbuf = _upload(h, s, bytes(desc))
    h.parquet_hybrid(dbuf.ptr, len(streams), s.handle,
                     max_blocks=max_blocks)
    s.sync()
    back = _download(h, s, dbuf.ptr, len(desc))
    vals = np.frombuffer(_download(h, s, obuf.ptr, 4 * n_out), np.uint32)
    out = []
    oo = 0
    for i, (_, _, count, _) in enumerate(streams):
        status = struct.unpack_from("<q", back, i * 64 + 48)[0]
        out.append((status, vals[oo:oo + count].tolist()))
        oo += count
    return out


def test_hybrid_streams_every_bit_width():
    """33 bit widths x 8 shapes = 264 streams in ONE launch on a 48-block
    grid, so most blocks take several turns of the grid stride."""
    rng = np.random.default_rng(42)
    streams, want = [], []
    for bw in range(33):
        for n, mode in ((1, "mixed"), (7, "mixed"), (65, "mixed"),
                        (129, "mixed"), (1000, "mixed"), (1000, "rle"),
                        (7, "bp"), (333, "bp")):
            vals, data = ref.synth_stream(rng, bw, n, mode)
            assert ref.decode_hybrid(data, bw, n) == vals
            streams.append((data, bw, n, 0))
            want.append(vals)
    got = _run_hybrid(streams, max_blocks=48)
    for (data, bw, n, _), (status, vals), w in zip(streams, got, want):
        assert status == 0, (bw, n, status)
        assert vals == w, (bw, n)


def test_hybrid_padded_final_group_and_limit():
    rng = np.random.default_rng(3)
    # 13 values in two groups of 8: the padding is not an overrun ...
    vals = [int(x) for x in rng.integers(0, 32, size=13)]
    data = ref.encode_hybrid(vals, 5, [("bp", 13)])
    # ... and the padding zeros are not checked against the limit, but a
    # real value at the limit is
    hi = max(vals)
    got = _run_hybrid([(data, 5, 13, 0), (data, 5, 13, hi + 1),
                       (data, 5, 13, hi), (data, 33, 13, 0)])
    assert got[0] == (0, vals)
    assert got[1] == (0, vals)
    assert got[2][0] == ref.ERR_DICT_INDEX
    assert got[3][0] == ref.ERR_FORMAT


# ---------------------------------------------------------------------------
# file level

def _land(raw: bytes):
    from demodel_amd.engine.pipeline import Lander

    pos = [0]

    def fill(view):
        n = min(len(view), len(raw) - pos[0])
        view[:n] = raw[pos[0]:pos[0] + n]
        pos[0] += n
        return n

    lander = Lander(slab_bytes=4 << 20, n_slabs=2)
    return lander.land(fill, len(raw))


@pytest.fixture(scope="module")
def table():
    return ref.make_table()


@pytest.mark.parametrize("variant", ref.VARIANTS, ids=ref.variant_id)
def test_gpu_decode_equals_read_table(tmp_path, table, variant):
    from demodel_amd.gpu import have_gpu

    assert have_gpu()
    p = tmp_path / "t.parquet"
    ref.write_variant(table, str(p), variant)
    back = pq.read_table(str(p))
    blob = _land(p.read_bytes())
    cols = pqf.decode_columns_gpu(blob)
    assert list(cols) == list(ref.DECODABLE)
    assert list(cols.skipped) == ["txt"]
    for name in ref.DECODABLE:
        col = cols[name]
        assert col.values.is_cuda
        assert col.values.dtype == pqf.torch_dtype(
            {"int32": pqf.TYPE_INT32, "int64": pqf.TYPE_INT64,
             "float": pqf.TYPE_FLOAT, "double": pqf.TYPE_DOUBLE}[
                 str(getattr(back.schema.field(name).type, "value_type",
                             back.schema.field(name).type))])
        got = ref.column_to_numpy(col)
        ref.assert_same(got, ref.arrow_expected(back, name),
                        f"{ref.variant_id(variant)} {name}")
        if got["valid"] is not None:
            assert (got["values"][~got["valid"]] == 0).all()


def test_gpu_decode_selected_columns_and_errors(tmp_path, table):
    p = tmp_path / "t.parquet"
    ref.write_variant(table, str(p), ("1.0", "dict", "snappy"))
    back = pq.read_table(str(p))
    blob = _land(p.read_bytes())
    cols = pqf.decode_columns_gpu(blob, ("lst", "f64n"))
    assert list(cols) == ["lst", "f64n"] and not cols.skipped
    for name in cols:
        ref.assert_same(ref.column_to_numpy(cols[name]),
                        ref.arrow_expected(back, name), name)
    with pytest.raises(ValueError, match="'txt'.*BYTE_ARRAY"):
        pqf.decode_columns_gpu(blob, ("rand32", "txt"))


# ---------------------------------------------------------------------------
# malformed pages

def _v1_page(def_levels, values, dict_bw=None):
    """A v1 page of an optional INT32 column: length-prefixed definition
    levels, then PLAIN values or (dict_bw given) a dictionary index
    stream.  Returns (bytes, offset of the values region)."""
    runs = [("rle", 40)] if len(set(def_levels[:40])) == 1 else []
    rest = len(def_levels) - sum(n for _, n in runs)
    lv = ref.encode_hybrid(def_levels, 1, runs + [("bp", rest)])
    head = struct.pack("<I", len(lv)) + lv
    if dict_bw is None:
        body = struct.pack(f"<{len(values)}i", *values)
    else:
        body = bytes([dict_bw]) + ref.encode_hybrid(
            values, dict_bw, [("bp", len(values))])
    return head + body, len(head)


def _run_pages(pages, infos, dictionary: bytes, dict_count: int):
    """Decode hand-made pages of one optional INT32 column through the
    package's plan -> ColumnDecode -> DecodeLaunch path.  Returns
    (decode, launch, stream) after the stream finished."""
    from demodel_amd.gpu import have_gpu, hip

    assert have_gpu()
    h = hip()
    s = h.Stream(0)
    blobs = [dictionary] + list(pages)
    spans = []
    off = 0
    for b in blobs:
        spans.append((off, len(b)))
        off += len(b)
    ring = _upload(h, s, b"".join(blobs))
    leaf = pqf.SchemaLeaf("c", pqf.TYPE_INT32, 1, 0, 0, True)
    plans = []
    entry = 0
    for i, info in enumerate(infos):
        plans.append(pqf.PagePlan(i + 1, 0, i + 1, info, entry, 0,
                                  dict_count))
        entry += info.num_values
    plan = pqf.DecodePlan([pqf.ColumnPlan(leaf, plans, entry, entry)], {})
    decode = pqf.ColumnDecode(plan, ring.ptr, spans.__getitem__)
    launch = pqf.DecodeLaunch([decode])
    launch.post(s.handle)
    s.sync()
    return decode, launch, s, ring


def test_malformed_pages_fail_alone():
    """Three damaged pages between good ones, ONE launch.  The bounds
    checks that catch them: hybrid_decode's `run > left` (overrun),
    `need > len - pos` (underrun) and `v >= limit` (dictionary index)."""
    from demodel_amd.gpu import hip

    rng = np.random.default_rng(9)
    n = 100
    dict_vals = [int(x) for x in rng.integers(-1000, 1000, size=8)]
    dictionary = struct.pack("<8i", *dict_vals)

    def levels():
        lv = [1] * 40 + [int(x) for x in rng.integers(0, 2, size=n - 40)]
        return lv, sum(lv)

    def info(page, enc):
        return pqf.PageInfo(pqf.PAGE_DATA, 0, len(page), len(page),
                            num_values=n, encoding=enc,
                            def_encoding=pqf.ENC_RLE,
                            rep_encoding=pqf.ENC_RLE)

    pages, infos, want = [], [], []

    def add(page, enc, expect):
        pages.append(page)
        infos.append(info(page, enc))
        want.append(expect)

    def good(use_dict):
        lv, k = levels()
        if use_dict:
            idx = [int(x) for x in rng.integers(0, 8, size=k)]
            page, _ = _v1_page(lv, idx, dict_bw=3)
            dense = [dict_vals[i] for i in idx]
            enc = pqf.ENC_RLE_DICTIONARY
        else:
            dense = [int(x) for x in rng.integers(-9999, 9999, size=k)]
            page, _ = _v1_page(lv, dense)
            enc = pqf.ENC_PLAIN
        it = iter(dense)
        add(page, enc, (0, [next(it) if d else 0 for d in lv], lv))

    good(False)
    # 1: the first run header (RLE, 40 levels) claims 101 > num_values
    lv, k = levels()
    page, _ = _v1_page(lv, [1] * k)
    assert page[4] == 40 << 1
    page = page[:4] + ref._varint(101 << 1) + page[5:]
    page = struct.pack("<I", struct.unpack_from("<I", page)[0] + 1) \
        + page[4:]
    add(page, pqf.ENC_PLAIN, (ref.ERR_OVERRUN, None, None))
    good(True)
    # 3: dictionary index stream cut in the middle of its bit-packed run
    lv, k = levels()
    idx = [int(x) for x in rng.integers(0, 8, size=k)]
    page, at = _v1_page(lv, idx, dict_bw=3)
    add(page[:at + 1 + 2 + (k * 3 // 8) // 2], pqf.ENC_RLE_DICTIONARY,
        (ref.ERR_UNDERRUN, None, None))
    good(False)
    # 5: one index equal to the dictionary count
    lv, k = levels()
    idx = [int(x) for x in rng.integers(0, 8, size=k)]
    idx[k // 2] = 7
    page, _ = _v1_page(lv, idx, dict_bw=3)
    add(page, pqf.ENC_RLE_DICTIONARY, (ref.ERR_DICT_INDEX, None, None))
    good(True)

    # the reference agrees on every status before the GPU sees the pages
    leaf = pqf.SchemaLeaf("c", pqf.TYPE_INT32, 1, 0, 0, True)
    for i, (page, inf, (status, _, _)) in enumerate(zip(pages, infos, want)):
        dl = [v & 0xFFFFFFFF for v in dict_vals]
        dl = dl[:7] if i == 5 else dl
        try:
            ref.decode_page(page, inf, leaf, dl)
            assert status == 0
        except ref.RefError as e:
            assert e.status == status, i

    # page 5 sees a 7-entry dictionary; the others may use all 8, so run
    # it in a launch of its own plan entry with dict_count 7
    decode, launch, s, ring = _run_pages(pages, infos, dictionary, 8)
    del ring
    res = launch.results(decode)
    assert [r[0] for r in res] == [0, ref.ERR_OVERRUN, 0,
                                   ref.ERR_UNDERRUN, 0, 0, 0]
    with pytest.raises(IOError) as e:
        decode.finish(res)
    msg = str(e.value)
    assert "column 'c' row group 0 page 2: status -3" in msg
    assert "column 'c' row group 0 page 4: status -4" in msg
    assert "page 1:" not in msg and "page 3:" not in msg

    # the good pages of the same launch are intact
    h = hip()
    out = np.frombuffer(_download(h, s, decode.out.ptr,
                                  decode.out.nbytes), np.uint8)
    v_off, d_off, _ = decode._layout[0]
    for i, (status, vals, lv) in enumerate(want):
        if status != 0:
            continue
        got_v = out[v_off + 4 * n * i:v_off + 4 * n * (i + 1)].view(np.int32)
        got_d = out[d_off + n * i:d_off + n * (i + 1)]
        assert got_v.tolist() == vals, i
        assert got_d.tolist() == lv, i

    # the index-at-dictionary-count page, with the 7-entry dictionary
    decode, launch, s, ring = _run_pages([pages[0], pages[5]],
                                         [infos[0], infos[5]],
                                         dictionary[:28], 7)
    res = launch.results(decode)
    assert [r[0] for r in res] == [0, ref.ERR_DICT_INDEX]
    with pytest.raises(IOError, match=r"page 2: status -6 \(dictionary"):
        decode.finish(res)

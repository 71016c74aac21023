"""Parquet page walking (Thrift compact headers) + decompression paths.

CPU: page walker against pyarrow-written files; every ZSTD page payload
must be a valid frame whose decompressed size matches the header (checked
with BOTH pyarrow's zstd and our host decoder).
"""

import os

import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.parquet as pq  # noqa: E402

from demodel_amd.engine.formats import parquet as pqf  # noqa: E402


def _write_parquet(path, n_rows=20_000, codec="zstd",
                   page_version="1.0"):
    import numpy as np

    rng = np.random.default_rng(3)
    words = [f"tok{i}" for i in range(500)]
    text = [" ".join(words[j] for j in rng.integers(0, 500, size=20))
            for _ in range(n_rows)]
    table = pa.table({
        "text": text,
        "idx": np.arange(n_rows),
        "score": rng.random(n_rows),
    })
    pq.write_table(table, path, compression=codec,
                   data_page_version=page_version)
    return table


def test_page_walk_covers_all_chunks(tmp_path):
    p = tmp_path / "t.parquet"
    _write_parquet(str(p))
    raw, pages = pqf.file_pages(str(p))
    assert pages, "no pages found"
    # header parse is validated internally (walk must end exactly at the
    # chunk boundary); check payload sizes are sane
    for codec, info in pages:
        assert codec == pqf.CODEC_ZSTD
        assert 0 < info.comp_size <= len(raw)
        assert info.uncomp_size > 0


def test_zstd_pages_decode_with_both_decoders(tmp_path):
    from demodel_amd import _native

    p = tmp_path / "t.parquet"
    _write_parquet(str(p))
    raw, pages = pqf.file_pages(str(p))
    c = pa.Codec("zstd")
    for codec, info in pages[:20]:
        payload = raw[info.comp_offset:info.comp_offset + info.comp_size]
        want = bytes(c.decompress(payload, info.uncomp_size))
        assert len(want) == info.uncomp_size
        got, status, consumed = _native.zstd_decode(payload,
                                                    info.uncomp_size + 16)
        assert status == 0 and got == want


def test_parse_footer_matches_pyarrow(tmp_path):
    p = tmp_path / "f.parquet"
    _write_parquet(str(p))
    raw = open(str(p), "rb").read()
    flen = pqf.footer_span(raw[-8:])
    chunks = pqf.parse_footer(raw[-8 - flen:-8])
    meta = pq.ParquetFile(str(p)).metadata
    want = []
    for rg in range(meta.num_row_groups):
        for col in range(meta.num_columns):
            cc = meta.row_group(rg).column(col)
            start = cc.dictionary_page_offset or cc.data_page_offset
            want.append((start, cc.total_compressed_size))
    assert [(c.start, c.total_compressed) for c in chunks] == want
    assert all(c.codec == pqf.CODEC_ZSTD for c in chunks)
    # and the self-contained walk agrees with the pyarrow-footer walk
    _, via_pyarrow = pqf.file_pages(str(p))
    pages_self = []
    for cm in chunks:
        for info in pqf.column_chunk_pages(raw, cm.start,
                                           cm.total_compressed):
            pages_self.append((cm.codec, info))
    assert pages_self == via_pyarrow


def test_uncompressed_parquet_pages(tmp_path):
    p = tmp_path / "u.parquet"
    _write_parquet(str(p), codec="none")
    raw, pages = pqf.file_pages(str(p))
    for codec, info in pages:
        assert codec == pqf.CODEC_UNCOMPRESSED
        assert info.comp_size == info.uncomp_size


def _page_plain(raw, codec_name, info):
    """CPU reconstruction of one decompressed page (v1 or v2)."""
    lvl = info.lvl_bytes
    levels = raw[info.comp_offset:info.comp_offset + lvl]
    body = raw[info.comp_offset + lvl:info.comp_offset + info.comp_size]
    if not info.is_compressed or codec_name == "none":
        return levels + body
    # parquet "lz4" pages are raw LZ4 blocks (arrow behavior), while
    # pa.Codec("lz4") is the FRAME codec — use the raw-block one
    c = pa.Codec("lz4_raw" if codec_name == "lz4" else codec_name)
    return levels + bytes(c.decompress(body, info.uncomp_size - lvl))


def test_v2_pages_parse_and_decode_cpu(tmp_path):
    p = tmp_path / "v2.parquet"
    _write_parquet(str(p), codec="zstd", page_version="2.0")
    raw, pages = pqf.file_pages(str(p))
    assert any(info.page_type == 3 for _, info in pages)
    for codec, info in pages:
        if info.page_type == 3:
            assert 0 <= info.lvl_bytes < info.comp_size
        plain = _page_plain(raw, "zstd", info)
        assert len(plain) == info.uncomp_size


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["zstd", "snappy", "gzip", "lz4"])
@pytest.mark.parametrize("page_version", ["1.0", "2.0"])
def test_gpu_page_decompress(tmp_path, codec, page_version):
    import ctypes

    from demodel_amd.engine.pipeline import Lander
    from demodel_amd.gpu import have_gpu, hip

    assert have_gpu()
    p = tmp_path / "g.parquet"
    _write_parquet(str(p), n_rows=50_000, codec=codec,
                   page_version=page_version)
    raw, pages = pqf.file_pages(str(p))

    pos = [0]

    def fill(view):
        n = min(len(view), len(raw) - pos[0])
        view[:n] = raw[pos[0]:pos[0] + n]
        pos[0] += n
        return n

    lander = Lander(slab_bytes=4 << 20, n_slabs=2)
    blob = lander.land(fill, len(raw))
    ring, spans = pqf.decompress_pages_gpu(blob, pages)

    h = hip()
    s = h.Stream(0)
    total = sum(sz for _, sz in spans)
    out = bytearray(total)
    addr = ctypes.addressof((ctypes.c_char * total).from_buffer(out))
    h.d2h_async(addr, ring.ptr, total, s.handle)
    s.sync()
    for (off, sz), (_, info) in zip(spans, pages):
        want = _page_plain(raw, codec, info)
        assert bytes(out[off:off + sz]) == want


def _write_mixed(path, page_version, n_rows=3000):
    """One file whose column chunks use every page codec the GPU path
    has, and an uncompressed one."""
    import numpy as np

    rng = np.random.default_rng(5)
    words = [f"tok{i}" for i in range(500)]
    text = [" ".join(words[j] for j in rng.integers(0, 500, size=20))
            for _ in range(n_rows)]
    table = pa.table({
        "a": text,
        "b": [t[::-1] for t in text],
        "c": np.arange(n_rows, dtype=np.int64),
        "d": rng.random(n_rows),
        "e": np.arange(n_rows, dtype=np.int32),
    })
    pq.write_table(table, path,
                   compression={"a": "zstd", "b": "snappy", "c": "gzip",
                                "d": "lz4", "e": "none"},
                   data_page_size=4096, write_batch_size=64,
                   use_dictionary=False, data_page_version=page_version)


_CODEC_NAMES = {pqf.CODEC_ZSTD: "zstd", pqf.CODEC_SNAPPY: "snappy",
                pqf.CODEC_GZIP: "gzip", pqf.CODEC_LZ4: "lz4",
                pqf.CODEC_LZ4_RAW: "lz4", pqf.CODEC_UNCOMPRESSED: "none"}


def test_mixed_codec_file_has_every_codec(tmp_path):
    from collections import Counter

    p = tmp_path / "m.parquet"
    _write_mixed(str(p), "1.0")
    _, pages = pqf.file_pages(str(p))
    per = Counter(_CODEC_NAMES[codec] for codec, _ in pages)
    assert set(per) == {"zstd", "snappy", "gzip", "lz4", "none"}
    # several streams per kernel, so descriptor indexing matters
    assert min(per[c] for c in ("zstd", "snappy", "gzip", "lz4")) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("page_version", ["1.0", "2.0"])
def test_gpu_page_decompress_all_codecs_one_job(tmp_path, page_version):
    """zstd, snappy, gzip, lz4 and uncompressed pages of ONE file go
    through one decompression job; every page must come back as its own
    chunk's codec decodes it on the CPU."""
    import ctypes

    from demodel_amd.engine.pipeline import Lander
    from demodel_amd.gpu import have_gpu, hip

    assert have_gpu()
    p = tmp_path / "m.parquet"
    _write_mixed(str(p), page_version)
    raw, pages = pqf.file_pages(str(p))

    pos = [0]

    def fill(view):
        n = min(len(view), len(raw) - pos[0])
        view[:n] = raw[pos[0]:pos[0] + n]
        pos[0] += n
        return n

    lander = Lander(slab_bytes=4 << 20, n_slabs=2)
    blob = lander.land(fill, len(raw))
    ring, spans = pqf.decompress_pages_gpu(blob, pages)

    h = hip()
    s = h.Stream(0)
    total = sum(sz for _, sz in spans)
    out = bytearray(total)
    addr = ctypes.addressof((ctypes.c_char * total).from_buffer(out))
    h.d2h_async(addr, ring.ptr, total, s.handle)
    s.sync()
    assert len(spans) == len(pages)
    for i, ((off, sz), (codec, info)) in enumerate(zip(spans, pages)):
        want = _page_plain(raw, _CODEC_NAMES[codec], info)
        assert bytes(out[off:off + sz]) == want, (i, _CODEC_NAMES[codec])

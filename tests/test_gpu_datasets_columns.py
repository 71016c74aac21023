"""stream_dataset(..., columns=...) end to end: shards served by the
test origin, decompressed and decoded on the GPU in one job, compared
with pyarrow's read of the same files."""

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.parquet as pq  # noqa: E402

import parquet_ref as ref  # noqa: E402
from helpers import Stack  # noqa: E402

pytestmark = pytest.mark.gpu


# shard 2 mixes codecs by column, so a coalesced launch of the three
# holds streams of all four codecs, at non-zero offsets in its lists
_SHARD_CODECS = ["snappy", "zstd",
                 {"ids": "gzip", "toks.list.element": "lz4",
                  "text": "zstd"}]


def _write_shards(d, n_shards=3, rows=1500):
    d.mkdir()
    files = {}
    for s in range(n_shards):
        rng = np.random.default_rng(20 + s)
        toks = [[int(x) for x in rng.integers(0, 32000,
                                              size=rng.integers(0, 12))]
                for _ in range(rows)]
        table = pa.table({
            "ids": np.arange(rows, dtype=np.int64) + 10_000 * s,
            "toks": pa.array(toks, pa.list_(pa.int32())),
            "text": [f"doc {s} {i}" for i in range(rows)],
        })
        name = f"train-{s:05d}-of-{n_shards:05d}.parquet"
        path = str(d / name)
        pq.write_table(table, path, compression=_SHARD_CODECS[s],
                       data_page_size=4096)
        files[name] = path
    return files


@pytest.mark.parametrize("eager", [True, False])
def test_stream_dataset_columns(tmp_path, eager):
    from demodel_amd.engine.datasets import stream_dataset

    files = _write_shards(tmp_path / "ds")
    stack = Stack(tmp_path)
    try:
        stack.origin.add_hf_repo("ds/cols", files)
        kw = dict(endpoint=stack.origin_base, patterns=("*.parquet",),
                  workers=2, eager=eager)
        plain = {b.name: b for b in stream_dataset("ds/cols", **kw)}
        typed = {b.name: b for b in stream_dataset(
            "ds/cols", columns=("ids", "toks"), **kw)}
        every = {b.name: b for b in stream_dataset("ds/cols", columns=(),
                                                   **kw)}
        assert set(plain) == set(typed) == set(every) == set(files)
        for name, path in files.items():
            back = pq.read_table(path)
            assert plain[name].columns is None
            b = typed[name]
            # the page bytes are what they were without columns
            assert b.spans == plain[name].spans
            assert (b.data == plain[name].data).all()
            assert list(b.columns) == ["ids", "toks"]
            for col in ("ids", "toks"):
                assert b.columns[col].values.is_cuda
                ref.assert_same(ref.column_to_numpy(b.columns[col]),
                                ref.arrow_expected(back, col),
                                f"{name} {col}")
            assert list(every[name].columns) == ["ids", "toks"]
            assert list(every[name].columns.skipped) == ["text"]
        with pytest.raises(ValueError, match="'text'"):
            list(stream_dataset("ds/cols", columns=("text",), **kw))
    finally:
        stack.close()

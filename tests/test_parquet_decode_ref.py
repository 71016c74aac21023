"""The scalar reference decoder (tests/parquet_ref.py) against pyarrow.

It reproducing pq.read_table for every column and write variant is what
licenses using it as the oracle for synthetic hybrid streams in the GPU
tests; the hybrid encoder has to round-trip through it at every bit
width."""

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.parquet as pq  # noqa: E402

import parquet_ref as ref  # noqa: E402
from demodel_amd.engine.formats import parquet as pqf  # noqa: E402


@pytest.fixture(scope="module")
def table():
    return ref.make_table()


@pytest.mark.parametrize("variant", ref.VARIANTS, ids=ref.variant_id)
def test_reference_reproduces_read_table(tmp_path, table, variant):
    p = tmp_path / "t.parquet"
    ref.write_variant(table, str(p), variant)
    back = pq.read_table(str(p))
    decoded = ref.decode_file(p.read_bytes())
    assert set(decoded) == set(ref.DECODABLE)
    for name in ref.DECODABLE:
        ref.assert_same(ref.assemble(decoded[name]),
                        ref.arrow_expected(back, name),
                        f"{ref.variant_id(variant)} {name}")


def test_null_slots_are_zero_and_payloads_survive(tmp_path, table):
    p = tmp_path / "t.parquet"
    ref.write_variant(table, str(p), ("1.0", "dict", "none"))
    got = ref.assemble(ref.decode_file(p.read_bytes())["f64n"])
    assert (got["values"][~got["valid"]] == 0).all()
    assert 0x7FF8000000000123 in got["values"]          # NaN payload
    assert 0x8000000000000000 in got["values"]          # -0.0


@pytest.mark.parametrize("bw", range(33))
def test_encoder_round_trips_through_reference(bw):
    rng = np.random.default_rng(100 + bw)
    for n, mode in ((1, "mixed"), (7, "bp"), (65, "mixed"), (1000, "mixed"),
                    (1000, "rle"), (333, "bp")):
        vals, stream = ref.synth_stream(rng, bw, n, mode)
        assert len(vals) == n
        assert ref.decode_hybrid(stream, bw, n) == vals


def test_reference_rejects_malformed_streams():
    vals, stream = ref.synth_stream(np.random.default_rng(1), 5, 100, "rle")
    with pytest.raises(ref.RefError) as e:
        ref.decode_hybrid(stream, 5, 99)             # run of 100 for 99
    assert e.value.status == ref.ERR_OVERRUN
    vals, stream = ref.synth_stream(np.random.default_rng(1), 5, 100, "bp")
    with pytest.raises(ref.RefError) as e:
        ref.decode_hybrid(stream[:20], 5, 100)       # cut mid-run
    assert e.value.status == ref.ERR_UNDERRUN
    with pytest.raises(ref.RefError) as e:
        ref.decode_hybrid(stream, 5, 100, limit=3,
                          err_limit=ref.ERR_DICT_INDEX)
    assert e.value.status == ref.ERR_DICT_INDEX
    with pytest.raises(ref.RefError) as e:
        ref.decode_hybrid(stream, 33, 100)
    assert e.value.status == ref.ERR_FORMAT


def test_assemble_column_matches_reference_walk(tmp_path, table):
    """The package's torch list compaction against the scalar walk, on
    the CPU: the same entry-aligned input must give the same column."""
    import torch

    p = tmp_path / "t.parquet"
    ref.write_variant(table, str(p), ("2.0", "dict", "snappy"))
    decoded = ref.decode_file(p.read_bytes())
    for name in ref.DECODABLE:
        e = decoded[name]
        leaf = e["leaf"]
        bits = np.array(e["values"], dtype=ref._bits_dtype(leaf))
        vals = torch.from_numpy(bits.view(
            np.int32 if bits.itemsize == 4 else np.int64).copy()).view(
                pqf.torch_dtype(leaf.physical_type))
        defs = torch.tensor(e["defs"], dtype=torch.uint8)
        reps = torch.tensor(e["reps"], dtype=torch.uint8)
        col = pqf.assemble_column(leaf, vals, defs, reps, e["num_rows"])
        ref.assert_same(ref.column_to_numpy(col), ref.assemble(e), name)

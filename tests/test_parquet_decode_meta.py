"""Footer schema, per-chunk and per-page metadata of the column decode
plan against pyarrow's own view of the same files, and the plan-time
ValueErrors for what the decoder does not cover."""

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
def test_schema_chunks_and_pages_match_pyarrow(tmp_path, table, variant):
    p = tmp_path / "t.parquet"
    ref.write_variant(table, str(p), variant)
    raw = p.read_bytes()
    f = pq.ParquetFile(str(p))
    md, schema = f.metadata, f.schema
    meta, chunk_pages = pqf.raw_meta_pages(raw)

    assert meta.num_rows == md.num_rows == ref.N_ROWS
    assert md.num_row_groups == 2
    assert len(meta.leaves) == md.num_columns
    for i, leaf in enumerate(meta.leaves):
        col = schema.column(i)
        assert leaf.path == col.path
        assert pqf.TYPE_NAMES[leaf.physical_type] == col.physical_type
        assert leaf.max_def == col.max_definition_level
        assert leaf.max_rep == col.max_repetition_level
    by_name = {lf.name: lf for lf in meta.leaves}
    assert set(by_name) == set(table.schema.names)
    for field in table.schema:
        assert by_name[field.name].nullable == field.nullable
    assert by_name["lst"].slot_level == 2
    assert by_name["lst_req"].slot_level == 1
    assert by_name["rand32"].slot_level == 0

    assert len(meta.chunks) == md.num_row_groups * md.num_columns
    n_pages = 0
    k = 0
    for rg in range(md.num_row_groups):
        for ci in range(md.num_columns):
            cc = md.row_group(rg).column(ci)
            cm = meta.chunks[k]
            pages = chunk_pages[k]
            k += 1
            assert (cm.row_group, cm.column) == (rg, ci)
            assert cm.path == cc.path_in_schema
            assert pqf.TYPE_NAMES[cm.physical_type] == cc.physical_type
            assert cm.num_values == cc.num_values
            assert cm.num_rows == md.row_group(rg).num_rows
            data = [pg for pg in pages
                    if pg.page_type != pqf.PAGE_DICTIONARY]
            assert sum(pg.num_values for pg in data) == cm.num_values
            chunk_encs = set(cc.encodings)
            assert {pqf.ENCODING_NAMES[e] for e in cm.encodings} \
                == chunk_encs
            for pg in pages:
                assert pqf.ENCODING_NAMES[pg.encoding] in chunk_encs
                want_type = (pqf.PAGE_DATA_V2 if variant[0] == "2.0"
                             else pqf.PAGE_DATA)
                if pg.page_type == pqf.PAGE_DICTIONARY:
                    assert pg is pages[0] and pg.num_values > 0
                    continue
                assert pg.page_type == want_type
                if pg.page_type == pqf.PAGE_DATA_V2:
                    assert pg.rep_bytes + pg.def_bytes == pg.lvl_bytes
                    assert 0 < pg.num_rows <= pg.num_values
                    assert 0 <= pg.num_nulls <= pg.num_values
                else:
                    assert pg.def_encoding == pqf.ENC_RLE
            n_pages += len(data)
    assert n_pages >= 20, "the fixture is meant to span many pages"

    plan = pqf.plan_columns(meta, chunk_pages)
    assert [c.leaf.name for c in plan.columns] == list(ref.DECODABLE)
    assert list(plan.skipped) == ["txt"]
    assert "BYTE_ARRAY" in plan.skipped["txt"]
    for col in plan.columns:
        assert col.num_rows == ref.N_ROWS
        assert [pg.entry_off for pg in col.pages] == list(np.cumsum(
            [0] + [pg.info.num_values for pg in col.pages])[:-1])
    # () means "all supported", like None
    assert [c.leaf.name for c in pqf.plan_columns(
        meta, chunk_pages, ()).columns] == list(ref.DECODABLE)
    sel = pqf.plan_columns(meta, chunk_pages, ("lst", "few64"))
    assert [c.leaf.name for c in sel.columns] == ["lst", "few64"]
    # the dotted leaf path names the same column
    sel = pqf.plan_columns(meta, chunk_pages, ("lst.list.element",))
    assert [c.leaf.name for c in sel.columns] == ["lst"]


def test_fallback_variant_mixes_dictionary_and_plain_pages(tmp_path, table):
    p = tmp_path / "t.parquet"
    ref.write_variant(table, str(p), ("1.0", "fallback", "none"))
    meta, chunk_pages = pqf.raw_meta_pages(p.read_bytes())
    mixed = 0
    for cm, pages in zip(meta.chunks, chunk_pages):
        encs = {pg.encoding for pg in pages
                if pg.page_type != pqf.PAGE_DICTIONARY}
        if pqf.ENC_PLAIN in encs and len(encs) > 1:
            mixed += 1
    assert mixed, "no chunk fell back from dictionary to PLAIN pages"


def _plan(path, columns=None):
    meta, chunk_pages = pqf.raw_meta_pages(open(path, "rb").read())
    return pqf.plan_columns(meta, chunk_pages, columns)


@pytest.mark.parametrize("name,array,kwargs,needle", [
    ("s", pa.array(["a", "bb", None]), {}, "BYTE_ARRAY"),
    ("b", pa.array([True, False, None]), {}, "BOOLEAN"),
    ("ll", pa.array([[[1, 2], [3]], None, [[]]],
                    pa.list_(pa.list_(pa.int32()))), {}, "nesting"),
    ("c", pa.array(np.arange(100, dtype=np.int32)),
     {"use_dictionary": False,
      "column_encoding": {"c": "DELTA_BINARY_PACKED"}},
     "DELTA_BINARY_PACKED"),
], ids=["string", "boolean", "list-of-list", "delta"])
def test_plan_rejects_unsupported(tmp_path, name, array, kwargs, needle):
    p = str(tmp_path / "u.parquet")
    ok = pa.array(np.arange(len(array), dtype=np.int64))
    pq.write_table(pa.table({name: array, "ok": ok}), p, **kwargs)
    with pytest.raises(ValueError) as e:
        _plan(p, (name,))
    assert repr(name) in str(e.value) and needle in str(e.value)
    # without a selection the column is skipped, with the same reason
    plan = _plan(p)
    assert [c.leaf.name for c in plan.columns] == ["ok"]
    assert needle in plan.skipped[name]


def test_plan_rejects_unknown_column(tmp_path, table):
    p = str(tmp_path / "t.parquet")
    ref.write_variant(table, p, ("1.0", "dict", "none"))
    with pytest.raises(ValueError, match="nope"):
        _plan(p, ("nope",))


def test_new_fields_keep_positional_construction_and_equality():
    a = pqf.PageInfo(0, 10, 20, 30)
    assert a == pqf.PageInfo(0, 10, 20, 30, 0, True, b"")
    assert a.num_values == 0 and a.encoding == -1
    assert pqf.ChunkMeta(6, 4, 100) == pqf.ChunkMeta(6, 4, 100)
    assert pqf.ChunkMeta(6, 4, 100).path == ""


def test_truncated_footer_fails_loudly(tmp_path, table):
    p = tmp_path / "t.parquet"
    ref.write_variant(table, str(p), ("1.0", "dict", "none"))
    raw = p.read_bytes()
    flen = pqf.footer_span(raw[-8:])
    footer = raw[-8 - flen:-8]
    for cut in range(1, len(footer), max(1, len(footer) // 97)):
        try:
            pqf.parse_file_meta(footer[:cut])
        except (ValueError, IndexError):
            pass

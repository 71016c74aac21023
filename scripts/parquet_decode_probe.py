#!/usr/bin/env python3
"""Time the parquet column decode (csrc/parquet_decode.hip) on whole files.

Three files, each landed in HBM once:

* c4     one testing/synth.write_parquet_shards shard (text, url,
         timestamp; only the int64 timestamp column is decodable);
* ints   an int/float/list shard with pyarrow's default dictionary
         encoding (falls back to PLAIN where the dictionary outgrows its
         page);
* plain  the same table with use_dictionary=False.

For each it times, as stream-synchronised wall clock, median over the
rounds after warm-up:

* headers     footer and page-header read-back from HBM plus the host
              plan (part of `full`; no payload moves);
* decode      pages already decompressed in the ring: descriptor upload,
              the decode launch and the status read-back;
* full        launch_columns_gpu + wait + finish: footer and page-header
              read-back, planning, decompression and decode on one
              stream, then the torch wrap (lists compacted);
* read_table  pyarrow on the host reading the same columns from the same
              file (page cache warm) — for scale only, it does not end
              with the data on the device.

GB/s is the typed, entry-aligned output (values plus level bytes) over
the median.  The result is compared with pyarrow's before timing.

Needs a GPU; writes a markdown report (default profiles/parquet_decode.md)
and keeps that file's hand-written tail from "## Notes" on (how to read
the table, the bench.py parent/child comparison).
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEEP_FROM = "\n## Notes"


def int_table(rows: int):
    import numpy as np
    import pyarrow as pa

    rng = np.random.default_rng(5)
    lens = rng.integers(0, 17, size=rows)
    flat = rng.integers(0, 32000, size=int(lens.sum())).astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    f64 = rng.standard_normal(rows)
    return pa.table({
        "ids": np.arange(rows, dtype=np.int64),
        "label": rng.integers(0, 10, size=rows).astype(np.int32),
        "tok": rng.integers(0, 50000, size=rows).astype(np.int32),
        "score": rng.random(rows).astype(np.float32),
        "w": pa.array(f64, mask=rng.random(rows) < 0.3),
        "toks": pa.ListArray.from_arrays(offs, flat),
    })


def land(raw: bytes):
    from demodel_amd.engine.pipeline import Lander

    pos = [0]

    def fill(view):
        n = min(len(view), len(raw) - pos[0])
        view[:n] = raw[pos[0]:pos[0] + n]
        pos[0] += n
        return n

    return Lander(slab_bytes=32 << 20, n_slabs=2).land(fill, len(raw))


def check(cols, table) -> None:
    """values / offsets against pyarrow, before anything is timed."""
    import numpy as np
    import pyarrow as pa

    for name, col in cols.items():
        arr = table.column(name).combine_chunks()
        if pa.types.is_list(arr.type):
            want = arr.flatten().to_numpy(zero_copy_only=False)
            offs = np.asarray(arr.offsets) - arr.offsets[0].as_py()
            if not np.array_equal(col.offsets.cpu().numpy(), offs):
                raise SystemExit(f"{name}: offsets differ from pyarrow")
        else:
            want = arr.fill_null(0).to_numpy(zero_copy_only=False)
        got = col.values.cpu().numpy()
        if got.tobytes() != np.asarray(want, dtype=got.dtype).tobytes():
            raise SystemExit(f"{name}: values differ from pyarrow")


def median_ms(fn, warmup: int, rounds: int) -> tuple[float, float, float]:
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def run_file(label, path, args):
    import pyarrow.parquet as pq

    from demodel_amd.engine.formats import parquet as pqf
    from demodel_amd.gpu import hip

    h = hip()
    raw = open(path, "rb").read()
    blob = land(raw)
    cols = pqf.decode_columns_gpu(blob)
    names = list(cols)
    check(cols, pq.read_table(path, columns=names))
    del cols

    # decode only: decompress once, then time the decode launch alone
    meta, chunk_pages = pqf.blob_meta_pages(blob)
    plan = pqf.plan_columns(meta, chunk_pages)
    flat = [(cm.codec, info)
            for cm, pages in zip(meta.chunks, chunk_pages)
            for info in pages]
    ring, spans = pqf.decompress_pages_gpu(blob, flat)
    decode = pqf.ColumnDecode(plan, ring.ptr, spans.__getitem__)
    s = h.Stream(0)

    def decode_only():
        launch = pqf.DecodeLaunch([decode])
        launch.post(s.handle)
        s.sync()
        if any(r[0] for r in launch.results(decode)):
            raise SystemExit(f"{label}: a page failed to decode")

    def full():
        job, pending = pqf.launch_columns_gpu(blob)
        job.wait()
        pending.finish()

    def headers():
        m, cp = pqf.blob_meta_pages(blob)
        pqf.plan_columns(m, cp)

    def host():
        pq.read_table(path, columns=names)

    out_bytes = sum(
        c.num_entries * (pqf._WIDTH[c.leaf.physical_type]
                         + bool(c.leaf.max_def) + bool(c.leaf.max_rep))
        for c in plan.columns)
    n_pages = len(decode.rows)
    rows = []
    for what, fn, rounds in (("headers", headers, args.rounds),
                             ("decode", decode_only, args.rounds),
                             ("full", full, args.rounds),
                             ("read_table", host, max(3, args.rounds // 5))):
        med, lo, hi = median_ms(fn, args.warmup, rounds)
        rows.append(f"| {label} | {what} | {len(names)} | {n_pages} | "
                    f"{out_bytes / 1e6:.1f} | {med:.3f} | {lo:.3f} | "
                    f"{hi:.3f} | {out_bytes / (med * 1e-3) / 1e9:.2f} |")
    return rows


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "parquet_decode.md"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--small", action="store_true",
                    help="tiny files: checks the script, not the kernel")
    args = ap.parse_args()
    if args.small:
        args.rows, args.rounds, args.warmup = 20_000, 3, 1

    import pyarrow.parquet as pq
    import torch

    from demodel_amd.gpu import have_gpu
    from demodel_amd.testing import synth

    if not have_gpu():
        print("parquet_decode_probe: no GPU; nothing is measured without "
              "one", file=sys.stderr)
        return 2
    tmp = tempfile.mkdtemp(prefix="demodel-pqprobe-")
    c4 = synth.write_parquet_shards(
        os.path.join(tmp, "c4"), n_shards=1,
        rows_per_shard=min(args.rows, 300_000))
    table = int_table(args.rows)
    ints = os.path.join(tmp, "ints.parquet")
    plain = os.path.join(tmp, "plain.parquet")
    pq.write_table(table, ints, compression="snappy")
    pq.write_table(table, plain, compression="snappy", use_dictionary=False)

    body = []
    for label, path in (("c4", next(iter(c4.values()))), ("ints", ints),
                        ("plain", plain)):
        body += run_file(label, path, args)

    props = torch.cuda.get_device_properties(0)
    dev = f"{props.name} ({props.gcnArchName.split(':')[0]})"
    lines = [
        "# Parquet column decode: pages in HBM to typed tensors",
        "",
        f"Measured by `scripts/parquet_decode_probe.py` on {dev}, "
        f"{args.rows} rows in the int files.  Stream-synchronised wall "
        f"clock in ms, {args.warmup} warm-up passes, median / fastest / "
        f"slowest of {args.rounds} rounds (read_table: of "
        f"{max(3, args.rounds // 5)}).  `headers` is the footer and "
        "page-header read-back plus the host plan; `decode` starts from decompressed "
        "pages; `full` is launch_columns_gpu + wait + finish from the "
        "landed file (header read-back, planning, decompression, decode, "
        "list compaction); `read_table` is pyarrow on the host for the "
        "same columns, page cache warm, and does not end on the device.  "
        "MB and GB/s count the typed entry-aligned output (values plus "
        "level bytes).  One wave decodes one page, so the page count "
        "bounds the parallelism.  Nothing here is a gate: the numbers are "
        "recorded, not asserted.",
        "",
        "| file | what | columns | data pages | out MB | median ms | "
        "min ms | max ms | GB/s out |",
        "|---|---|---|---|---|---|---|---|---|",
    ] + body + [""]
    text = "\n".join(lines)
    if os.path.exists(args.out):
        old = open(args.out).read()
        if KEEP_FROM in old:
            text += old[old.index(KEEP_FROM):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

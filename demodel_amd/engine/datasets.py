"""Dataset streaming: pull shards, decompress to device memory, iterate.

BASELINE.json config 5 as a user-facing API: parquet shards (ZSTD pages)
or .zst frame shards stream through the landing pipeline and decompress
wave-parallel into HBM rings; the iterator yields one shard at a time so
a training/ingest loop can consume while later shards still pull.

Overlap is two-level: the pull runs on worker threads (pull_hf_stream)
while this thread LAUNCHES each completed shard's decompression async on
its own HIP stream (DecompressJob), so downloads, several shards'
decodes, and the consumer all run concurrently.  Per-shard frame counts
are far below the chip's wave capacity (256 frames vs 2048 wave slots),
so concurrent per-shard launches are what keep the zstd kernel occupancy
at the level a single whole-dataset launch would get.

On CPU-only machines the same API decompresses with pyarrow, so the data
path is testable anywhere.
"""

from __future__ import annotations

import json
from collections import deque
from dataclasses import dataclass

from ..utils.log import get_logger
from .pull import LanderPool

log = get_logger("datasets")


@dataclass
class ShardBatch:
    name: str
    data: object            # torch.uint8 tensor (device or cpu)
    spans: list             # [(offset, length)] decompressed record spans
    # parquet shards streamed with columns=...: formats.parquet.Columns
    # (name -> Column of device tensors, plus .skipped)
    columns: dict | None = None

    def tensors(self):
        return [self.data[o:o + n] for o, n in self.spans]


def _prep_parquet_gpu(blob, columns=None):
    """(prep_pages_gpu's plan, decode): decode is the ColumnDecode that
    turns the decompressed pages into tensors when columns is not None,
    else None."""
    from .formats import parquet as pqf

    if columns is None:
        return pqf.prep_pages_gpu(blob, pqf.blob_pages(blob)), None
    meta, chunk_pages = pqf.blob_meta_pages(blob)
    plan = pqf.plan_columns(meta, chunk_pages, columns)
    pages = [(cm.codec, info)
             for cm, cp in zip(meta.chunks, chunk_pages) for info in cp]
    prep = pqf.prep_pages_gpu(blob, pages)
    return prep, pqf.ColumnDecode(plan, prep.ring.ptr,
                                  prep.spans.__getitem__)


def _prep_zst_frames_gpu(blob, idx):
    from ..gpu import hip
    from .formats.compress import DecompressPlan

    total = sum(fr["decompressed"] for fr in idx["frames"])
    plan = DecompressPlan(ring=hip().DeviceBuffer(max(total, 1)))
    off = 0
    for fr in idx["frames"]:
        plan.streams["zstd"].append(
            (blob.buffer.ptr + fr["offset"], fr["compressed"],
             plan.ring.ptr + off, fr["decompressed"]))
        plan.spans.append((off, fr["decompressed"]))
        off += fr["decompressed"]
    return plan


def _decompress_cpu(blob, idx):
    import pyarrow as pa
    import torch

    codec = pa.Codec("zstd")
    raw = bytes(blob.buffer)
    out = bytearray()
    spans = []
    for fr in idx["frames"]:
        d = bytes(codec.decompress(
            raw[fr["offset"]:fr["offset"] + fr["compressed"]],
            fr["decompressed"]))
        spans.append((len(out), len(d)))
        out += d
    return torch.frombuffer(bytearray(out), dtype=torch.uint8), spans


def _sidecar_idx(sidecar):
    raw = (bytes(sidecar.blob.buffer) if sidecar.blob.device == "cpu"
           else bytes(sidecar.blob.head[:sidecar.blob.nbytes]))
    return json.loads(raw)


def stream_dataset(repo: str, endpoint: str | None = None,
                   patterns: tuple = ("*.parquet", "*.zst", "*.idx.json"),
                   device_index: int = 0, workers: int = 4,
                   verify: str = "chunked",
                   landers: LanderPool | None = None,
                   digest_map: dict | None = None,
                   on_file=None, inflight: int = 4, eager: bool = True,
                   repo_type: str = "model",
                   columns: tuple | None = None):
    """Yield ShardBatch per data shard of an HF dataset repo.

    columns=None (default) yields the decompressed pages only.  A tuple
    of column names, or () for every column the decoder supports, also
    decodes parquet shards' pages into typed device tensors in the same
    job that decompressed them (formats.parquet.decode_columns_gpu says
    what is supported); they arrive as ShardBatch.columns.  .zst shards
    are unaffected.

    inflight bounds how many decompressed shard rings can be in flight
    (launched but not yet yielded) at once — the HBM high-water mark is
    roughly (inflight + 1) decompressed shards plus the compressed
    blobs.  on_file(pulled_file) fires per landed file (digest capture,
    progress).

    eager=True (default) launches each burst's decode while later
    shards still download — best latency to the first batch.  On
    payloads where decode saturates the chip for long stretches the
    decode waves starve the in-flight pulls' verify kernels, so
    eager=False defers everything into ONE maximal launch after the
    last shard lands — best whole-dataset seconds-to-ready."""
    from ..gpu import have_gpu

    from .formats.compress import check_results
    from .pull import pull_hf_stream

    _, names, gen = pull_hf_stream(
        repo, endpoint=endpoint, workers=workers, verify=verify,
        patterns=list(patterns), device_index=device_index,
        landers=landers, digest_map=digest_map, batched=True,
        repo_type=repo_type)
    expected = set(names)
    gpu = have_gpu()

    def launch_batch(shards):
        """Coalesce every shard that became ready at the same time into
        ONE launch per codec (a shared DecompressJob; each shard holds a
        view of its ranges).  Per-shard frame counts (~hundreds) are far
        below the chip's wave slots, and kernels on the same HW queue
        serialize — batching restores big-launch occupancy while the
        launch itself stays async.  Returns [(shard, jobview_or_None,
        ring_or_data, spans)].  The torch wrap of a GPU ring happens at
        FINISH time: torch.from_dlpack synchronizes with the device,
        which would serialize the launches."""
        from .formats.compress import DecompressJob, DecompressPlan

        out = []
        merged = DecompressPlan()
        decodes = []
        entries = []
        for f in shards:
            if f.name.endswith(".parquet"):
                if not gpu:
                    raise RuntimeError(
                        "parquet streaming needs a GPU (CPU fallback "
                        "covers .zst shards)")
                plan, decode = _prep_parquet_gpu(f.blob, columns)
            else:
                idx = _sidecar_idx(f.sidecar)
                if not gpu:
                    data, spans = _decompress_cpu(f.blob, idx)
                    out.append((f, None, data, spans, None))
                    continue
                plan, decode = _prep_zst_frames_gpu(f.blob, idx), None
            entries.append((f, merged.absorb(plan), plan, decode))
            if decode is not None:
                decodes.append(decode)
        if entries:
            # the shards' column decodes share ONE launch too, queued
            # behind the decompression on the job's stream
            launch = None
            if decodes:
                from .formats.parquet import DecodeLaunch

                launch = DecodeLaunch(decodes)
            job = DecompressJob(
                merged.streams, pre_launch=merged.queue_copies,
                window=16 << 10,
                post_launch=launch.post if launch else None)
            for f, ranges, plan, decode in entries:
                out.append((f, job.view(ranges), plan.ring, plan.spans,
                            (launch, decode) if decode else None))
        return out

    def finish(item):
        shard, job, data, spans, decoding = item
        cols = None
        if job is not None:
            check_results(job.wait(), f"GPU decompress of {shard.name}")
            import torch

            if decoding is not None:
                launch, decode = decoding
                try:
                    cols = decode.finish(launch.results(decode))
                except IOError as e:
                    raise IOError(f"{shard.name}: {e}") from None
            data = torch.from_dlpack(data.to_dlpack())
        log.info("dataset shard %s: %d spans, %d bytes decompressed",
                 shard.name, len(spans), int(data.numel()))
        return ShardBatch(name=shard.name, data=data, spans=spans,
                          columns=cols)

    # pending holds the PulledFile too: its HBM blob must stay alive
    # until the decode kernel reading it has finished
    pending: deque = deque()
    deferred: list = []
    byname: dict = {}
    for burst in gen:
        ready = []
        for f in burst:
            if on_file is not None:
                on_file(f)
            byname[f.name] = f
            if f.name.endswith(".parquet"):
                ready.append(f)
            elif f.name.endswith(".zst"):
                if f.name + ".idx.json" not in expected:
                    raise FileNotFoundError(
                        f"{f.name}: missing .idx.json")
                if f.name + ".idx.json" in byname:
                    f.sidecar = byname[f.name + ".idx.json"]
                    ready.append(f)
            elif f.name.endswith(".zst.idx.json"):
                shard = byname.get(f.name[:-len(".idx.json")])
                if shard is not None:
                    shard.sidecar = f
                    ready.append(shard)
        if not eager:
            deferred.extend(ready)
            continue
        if ready:
            batch = launch_batch(ready)
            log.debug("launched decode of %d shard(s) (%d pending)",
                      len(batch), len(pending) + len(batch))
            pending.extend(batch)
        # yield whatever has finished decoding; block only over the
        # inflight cap (bounds HBM rings held by un-yielded shards)
        while pending and (len(pending) > inflight
                           or pending[0][1] is None
                           or pending[0][1].done()):
            yield finish(pending.popleft())
    if deferred:
        pending.extend(launch_batch(deferred))
    while pending:
        yield finish(pending.popleft())

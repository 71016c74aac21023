"""Model loading: scatter a landed safetensors blob into existing
tensors (SURVEY.md §2.3 K4's real job).

Zero-copy views (safetensors.torch_views) cover the "give me tensors"
case; this module covers loading into a model whose parameters already
live at allocator-chosen addresses — one scatter_ranges launch moves
every matching tensor's bytes HBM->HBM (3.2 TB/s class), with an
f32->bf16 cast path when the checkpoint dtype is wider than the model's
and an FP8 block-scaled dequant path (F8_E4M3 weight + `*_scale_inv` /
`*_scale` tensor -> bf16/f32, csrc/fp8_dequant.hip) when it is narrower.
"""

from __future__ import annotations

from array import array

from ..gpu import hip
from .formats.safetensors import SafetensorsHeader, fp8_scale_map

_PIECE = 1 << 20  # scatter descriptor granularity (see load_into)
_DESC_CLASS = 64 << 10  # descriptor buffers round up to this for reuse

# dtype codes of _hip.fp8_block_dequant
_FP8_SCALE_CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
_FP8_DST_CODE = {"bfloat16": 0, "float32": 1}


def _check_extent(blob, header: SafetensorsHeader, info) -> None:
    """A crafted header must not drive an out-of-bounds read: a tensor a
    kernel is about to read has to lie inside the landed blob and be as
    long as its shape says."""
    n = info.itemsize
    for d in info.shape:
        n *= d
    end = header.data_offset + info.end
    if info.nbytes != n or end > blob.nbytes:
        raise ValueError(
            f"{info.name}: extent [{header.data_offset + info.begin}, "
            f"{end}) of shape {info.shape} does not fit the blob "
            f"({blob.nbytes} bytes)")


def _cpu_view(u8, header: SafetensorsHeader, info):
    """One tensor of a host-landed blob.  Zero-copy unless the tensor
    sits at an offset its dtype cannot be viewed at (safetensors aligns
    nothing), which costs a copy."""
    import torch

    raw = u8[header.data_offset + info.begin:
             header.data_offset + info.end]
    if raw.storage_offset() % info.itemsize or \
            raw.data_ptr() % info.itemsize:
        raw = raw.clone()
    return raw.view(getattr(torch, info.torch_dtype)).view(info.shape)


def _expand_fp8_scale(scale, shape, block):
    """[ceil(R/br), ceil(C/bc)] scales -> one f32 scale per element."""
    R, C = shape
    br, bc = block
    grid = scale.float().reshape(-(-R // br), -(-C // bc))
    return grid.repeat_interleave(br, 0)[:R].repeat_interleave(bc, 1)[:, :C]


def load_into(blob, header: SafetensorsHeader, targets: dict,
              strict: bool = True, stream=None,
              fp8_block_size=None) -> list[str]:
    """Scatter tensors from `blob` into `targets` (name -> torch tensor
    on the same device).  Returns the names loaded.

    Same-dtype tensors batch into one scatter_ranges launch; f32->bf16
    casts launch per tensor, and so do F8_E4M3 weights going to a bf16 or
    f32 target: those are multiplied by their scale tensor (see
    safetensors.fp8_scale_map; `fp8_block_size` is the checkpoint's
    weight_block_size when it states one), and a scale tensor consumed
    that way is not a tensor the model is missing.  Raises on
    shape/dtype mismatches (strict) or missing tensors (strict).
    """
    import torch

    names = {t.name: t for t in header.tensors}
    fp8_scales = None   # resolved on the first FP8 weight that widens
    used_scales = set()

    def fp8_scale_for(name, info, dst):
        """The Fp8Scale to dequantise `name` with, or None when it is not
        an FP8 weight going to a wider target."""
        nonlocal fp8_scales
        if info.st_dtype != "F8_E4M3" or \
                str(dst.dtype).split(".")[-1] not in _FP8_DST_CODE:
            return None
        if fp8_scales is None:
            fp8_scales = fp8_scale_map(header, fp8_block_size)
        sc = fp8_scales.get(name)
        if sc is None:
            raise ValueError(
                f"{name}: cannot load {info.torch_dtype} into {dst.dtype}:"
                f" no scale tensor ({name}_scale_inv or {name}_scale) "
                "found in the checkpoint")
        _check_extent(blob, header, info)
        _check_extent(blob, header, sc.info)
        used_scales.add(sc.info.name)
        return sc

    def check_missing():
        missing = set(names) - set(targets) - used_scales
        if missing:
            raise KeyError(f"model is missing tensors: {sorted(missing)[:5]}"
                           f"{'...' if len(missing) > 5 else ''}")

    if blob.device == "cpu":
        # CPU landing target: plain torch copies from zero-copy views
        u8 = blob.torch_u8()
        loaded = []
        for name, dst in targets.items():
            info = names.get(name)
            if info is None:
                if strict:
                    raise KeyError(f"tensor {name!r} not in checkpoint")
                continue
            if tuple(dst.shape) != tuple(info.shape):
                raise ValueError(f"{name}: shape mismatch")
            sc = fp8_scale_for(name, info, dst)
            if sc is not None:
                v = (_cpu_view(u8, header, info).float()
                     * _expand_fp8_scale(_cpu_view(u8, header, sc.info),
                                         info.shape, sc.block))
            else:
                v = _cpu_view(u8, header, info)
            with torch.no_grad():
                dst.copy_(v.to(dst.dtype))
            loaded.append(name)
        if strict:
            check_missing()
        return loaded

    h = hip()
    own = stream is None
    s = h.Stream(0) if own else stream
    handle = s.handle

    triples = array("Q")  # (src_off, dst_ptr, nbytes) per tensor
    n_desc = 0
    casts = []
    dequants = []
    loaded = []
    for name, dst in targets.items():
        info = names.get(name)
        if info is None:
            if strict:
                raise KeyError(f"tensor {name!r} not in checkpoint")
            continue
        if tuple(dst.shape) != info.shape:
            raise ValueError(
                f"{name}: shape {tuple(dst.shape)} != {info.shape}")
        if not dst.is_contiguous():
            raise ValueError(f"{name}: target must be contiguous")
        src_off = header.data_offset + info.begin
        sc = fp8_scale_for(name, info, dst)
        if sc is not None:
            dequants.append((
                src_off, header.data_offset + sc.info.begin,
                _FP8_SCALE_CODE[sc.info.torch_dtype], dst.data_ptr(),
                _FP8_DST_CODE[str(dst.dtype).split(".")[-1]],
                info.shape[0], info.shape[1], sc.block[0], sc.block[1]))
        elif dst.dtype == getattr(torch, info.torch_dtype):
            # one descriptor per <=1 MiB piece: the kernel maps one
            # workgroup per descriptor, so an unsplit 1 GB tensor would
            # crawl on a single WG (~4 GB/s; measured 256 ms for the
            # 16 GB model).  1 MiB pieces give 16k WGs across 256 CUs.
            # The split itself is native (write_scatter_descs below): the
            # Python loop over ~15k pieces cost 7 ms of the timed step.
            triples.extend((src_off, dst.data_ptr(), info.nbytes))
            n_desc += -(-info.nbytes // _PIECE)
        elif info.torch_dtype == "float32" and dst.dtype == torch.bfloat16:
            casts.append((src_off, dst.data_ptr(), info.nbytes // 4))
        else:
            raise ValueError(
                f"{name}: cannot load {info.torch_dtype} into {dst.dtype}")
        loaded.append(name)
    if strict:
        check_missing()

    dbuf = pin = None
    pool = getattr(blob, "pool", None)
    dlen = n_desc * 32
    dcap = -(-dlen // _DESC_CLASS) * _DESC_CLASS
    if n_desc:
        # descriptor block: device side recycled through the landing
        # BufferPool (no hipMalloc/hipFree per file per pull), host side
        # staged in a cached pinned slab (a pageable source makes the
        # "async" copy block on the stream's earlier work)
        dbuf = pool.take(dcap) if pool is not None else None
        if dbuf is None:
            dbuf = h.DeviceBuffer(dcap)
        pin = h.PinnedPool(dcap, 1)
        pin.acquire(0)
        wrote = pin.write_scatter_descs(0, triples, _PIECE)
        assert wrote == n_desc, (wrote, n_desc)
        pin.submit(0, dbuf.ptr, dlen, handle)
        h.scatter_ranges(blob.buffer.ptr, dbuf.ptr, n_desc, handle)
    for src_off, dst_ptr, n in casts:
        h.cast_f32_to_bf16(blob.buffer.ptr + src_off, dst_ptr, n, handle)
    for (src_off, sc_off, sc_code, dst_ptr, dst_code, rows, cols,
         brows, bcols) in dequants:
        h.fp8_block_dequant(blob.buffer.ptr + src_off,
                            blob.buffer.ptr + sc_off, sc_code, dst_ptr,
                            dst_code, rows, cols, brows, bcols, handle)
    # synchronous by contract: desc buffer and host staging must outlive
    # the launches
    s.sync()
    if dbuf is not None and pool is not None:
        pool.put(dbuf, dcap)
    return loaded


def _pull_config(result) -> dict | None:
    """The pull's config.json as a dict, or None when it has none."""
    import json

    cfg_file = next((f for f in result.files if f.name == "config.json"),
                    None)
    if cfg_file is None:
        return None
    cfg_bytes = (bytes(cfg_file.blob.head[:cfg_file.nbytes])
                 if cfg_file.blob.device != "cpu"
                 else bytes(cfg_file.blob.buffer))
    return json.loads(cfg_bytes)


def pull_pretrained(repo: str, endpoint: str | None = None,
                    device: str | None = None, model_builder=None,
                    dequantize: bool = False, **pull_kw):
    """Pull an HF repo and materialize a transformers model with weights
    scattered straight from the landed HBM blobs (no host round-trip on
    GPU machines).

    model_builder(config) -> nn.Module; defaults to
    transformers.AutoModelForCausalLM.from_config.

    dequantize=True loads an FP8 block-scaled checkpoint into plain
    modules: `quantization_config` is dropped from the config before the
    model is built, the model is built in the config's torch_dtype
    (default bfloat16), and the FP8 weights are widened on the way in
    (load_into).
    Returns (model, PullResult)."""
    import torch

    from ..gpu import have_gpu
    from .pull import pull_hf

    res = pull_hf(repo, endpoint=endpoint, **pull_kw)
    cfg_dict = _pull_config(res)
    if cfg_dict is None:
        raise FileNotFoundError("repo has no config.json")

    import transformers

    build_dtype = None
    if dequantize:
        cfg_dict = {k: v for k, v in cfg_dict.items()
                    if k != "quantization_config"}
        dt = cfg_dict.get("torch_dtype") or cfg_dict.get("dtype") \
            or "bfloat16"
        build_dtype = getattr(torch, str(dt).split(".")[-1])
    config = transformers.AutoConfig.for_model(
        cfg_dict.get("model_type"), **{
            k: v for k, v in cfg_dict.items() if k != "model_type"})
    if device is None:
        device = "cuda" if have_gpu() else "cpu"
    if model_builder is None:
        def model_builder(c):
            return transformers.AutoModelForCausalLM.from_config(c)
    prev_dtype = torch.get_default_dtype()
    try:
        if build_dtype is not None:
            torch.set_default_dtype(build_dtype)
        with torch.device(device):
            model = model_builder(config)
    finally:
        torch.set_default_dtype(prev_dtype)
    model = model.to(device)
    model.eval()  # match from_pretrained semantics
    n = load_model_from_pull(res, model)
    if n == 0:
        raise RuntimeError("no tensors loaded from pull")
    return model, res


def load_model_from_pull(result, model, strict: bool = False) -> int:
    """Load a pull result's safetensors shards into a torch module's
    named parameters/buffers.  FP8 weights widen with the block size the
    pull's config.json states (quantization_config.weight_block_size),
    when it has one.  Returns tensors loaded."""
    from .formats import safetensors as st

    try:
        cfg = _pull_config(result)
    except ValueError:  # not this function's file to complain about
        cfg = None
    qcfg = cfg.get("quantization_config") if isinstance(cfg, dict) else None
    fp8_block_size = (qcfg.get("weight_block_size")
                      if isinstance(qcfg, dict) else None)
    targets = dict(model.named_parameters())
    targets.update(dict(model.named_buffers()))
    n = 0
    for f in result.files:
        if not f.name.endswith(".safetensors"):
            continue
        hdr = st.parse_header(f.blob.head)
        present = {t.name for t in hdr.tensors}
        n += len(load_into(f.blob, hdr,
                           {k: v for k, v in targets.items()
                            if k in present},
                           strict=strict, fp8_block_size=fp8_block_size))
    return n

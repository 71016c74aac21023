"""safetensors container parsing — header only, zero-copy by design.

Format: u64-LE header length, then a JSON header mapping tensor name ->
{"dtype", "shape", "data_offsets": [begin, end)} relative to the data
section, then the raw data section.  A blob landed contiguously in HBM
therefore becomes tensors by *viewing* byte ranges — no per-tensor copy at
all (the MI355X replacement for a host-side parse+upload loop).
"""

from __future__ import annotations

import json
import struct
from dataclasses import dataclass

_DTYPES = {
    "BOOL": ("bool", 1), "U8": ("uint8", 1), "I8": ("int8", 1),
    "F8_E4M3": ("float8_e4m3fn", 1), "F8_E5M2": ("float8_e5m2", 1),
    "I16": ("int16", 2), "U16": ("uint16", 2), "F16": ("float16", 2),
    "BF16": ("bfloat16", 2), "I32": ("int32", 4), "U32": ("uint32", 4),
    "F32": ("float32", 4), "F64": ("float64", 8), "I64": ("int64", 8),
    "U64": ("uint64", 8),
}


@dataclass
class TensorInfo:
    name: str
    st_dtype: str          # safetensors dtype tag, e.g. "BF16"
    torch_dtype: str       # torch name, e.g. "bfloat16"
    itemsize: int
    shape: tuple[int, ...]
    begin: int             # byte offset into the DATA section
    end: int

    @property
    def nbytes(self) -> int:
        return self.end - self.begin


@dataclass
class SafetensorsHeader:
    header_bytes: int      # 8 + json length
    data_offset: int       # where the data section starts in the file
    tensors: list[TensorInfo]
    metadata: dict

    @property
    def data_bytes(self) -> int:
        return max((t.end for t in self.tensors), default=0)


@dataclass
class Fp8Scale:
    """The scale tensor that goes with one F8_E4M3 weight: element
    [r, c] of the weight multiplies scale[r // block[0], c // block[1]]."""
    info: TensorInfo
    block: tuple[int, int]     # (block_rows, block_cols)


_FP8_SCALE_DTYPES = ("F32", "BF16", "F16")
_FP8_DEFAULT_BLOCK = (128, 128)


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n *= d
    return n


def _resolve_fp8_block(name, shape, sshape, block_size):
    R, C = shape
    if _numel(sshape) == 1 and len(sshape) <= 1:
        return (max(R, 1), max(C, 1))                    # per tensor
    if sshape in ((R,), (R, 1)):
        return (1, max(C, 1))                            # per output row
    if len(sshape) == 2:
        sr, sc = sshape
        for cand in (block_size, _FP8_DEFAULT_BLOCK):
            if cand is None:
                continue
            br, bc = (int(x) for x in cand)
            if br > 0 and bc > 0 and \
                    (-(-R // br), -(-C // bc)) == (sr, sc):
                return (br, bc)
        if sr > 0 and sc > 0 and R and C and R % sr == 0 and C % sc == 0:
            return (R // sr, C // sc)
    raise ValueError(
        f"{name}: scale shape {sshape} fits no block of weight shape "
        f"{shape}")


def fp8_scale_map(header: SafetensorsHeader,
                  block_size=None) -> dict[str, Fp8Scale]:
    """Find the scale tensor of every F8_E4M3 tensor X in the header:
    X + "_scale_inv" (one scale per 128x128 block in published
    checkpoints) or else X + "_scale" (compressed-tensors: per tensor or
    per output row).  Both multiply.  `block_size` is the checkpoint's
    quantization_config.weight_block_size when it has one.

    Returns weight name -> Fp8Scale; FP8 tensors without a scale tensor
    are absent.  Raises ValueError for a scale of the wrong dtype, a
    scaled weight that is not 2-D, or a scale shape that fits no block.
    """
    if block_size is not None:
        if len(block_size) != 2:
            raise ValueError(f"block_size must be (rows, cols), got "
                             f"{block_size!r}")
        block_size = tuple(int(x) for x in block_size)
    by_name = {t.name: t for t in header.tensors}
    out = {}
    for t in header.tensors:
        if t.st_dtype != "F8_E4M3":
            continue
        sinfo = by_name.get(t.name + "_scale_inv") or \
            by_name.get(t.name + "_scale")
        if sinfo is None:
            continue
        if sinfo.st_dtype not in _FP8_SCALE_DTYPES:
            raise ValueError(
                f"{sinfo.name}: scale dtype {sinfo.st_dtype} is not one of "
                f"{_FP8_SCALE_DTYPES}")
        if len(t.shape) != 2:
            raise ValueError(
                f"{t.name}: FP8 tensor with a scale must be 2-D, got shape "
                f"{t.shape}")
        out[t.name] = Fp8Scale(
            info=sinfo,
            block=_resolve_fp8_block(t.name, t.shape, sinfo.shape,
                                     block_size))
    return out


def parse_header(prefix: bytes) -> SafetensorsHeader:
    """Parse from the first bytes of a safetensors file.

    Raises ValueError if `prefix` is too short (caller feeds more bytes) —
    len required is 8 + header_len, available via header_len_needed().
    """
    if len(prefix) < 8:
        raise ValueError("need at least 8 bytes")
    (hlen,) = struct.unpack("<Q", prefix[:8])
    if hlen > 100 << 20:
        raise ValueError(f"implausible safetensors header length {hlen}")
    if len(prefix) < 8 + hlen:
        raise ValueError(f"need {8 + hlen} header bytes, have {len(prefix)}")
    obj = json.loads(prefix[8:8 + hlen])
    meta = obj.pop("__metadata__", {})
    tensors = []
    for name, spec in obj.items():
        tag = spec["dtype"]
        if tag not in _DTYPES:
            raise ValueError(f"unsupported safetensors dtype {tag!r}")
        tname, isz = _DTYPES[tag]
        b, e = spec["data_offsets"]
        # untrusted input: negative offsets would make the python-slice
        # views silently read from the blob's END
        if not (isinstance(b, int) and isinstance(e, int)
                and 0 <= b <= e):
            raise ValueError(f"bad data_offsets for {name!r}: {b}, {e}")
        tensors.append(TensorInfo(
            name=name, st_dtype=tag, torch_dtype=tname, itemsize=isz,
            shape=tuple(spec["shape"]), begin=b, end=e))
    tensors.sort(key=lambda t: t.begin)
    return SafetensorsHeader(header_bytes=8 + hlen, data_offset=8 + hlen,
                             tensors=tensors, metadata=meta)


def header_len_needed(first8: bytes) -> int:
    (hlen,) = struct.unpack("<Q", first8[:8])
    return 8 + hlen


def build_header(tensors: dict[str, tuple[str, tuple[int, ...], int]],
                 ) -> tuple[bytes, int]:
    """Serialize a header for synthetic blob generation.

    tensors: name -> (st_dtype, shape, nbytes); offsets assigned in order.
    Returns (header_bytes_blob, data_section_bytes).
    """
    obj = {}
    off = 0
    for name, (tag, shape, nbytes) in tensors.items():
        obj[name] = {"dtype": tag, "shape": list(shape),
                     "data_offsets": [off, off + nbytes]}
        off += nbytes
    js = json.dumps(obj).encode()
    pad = (8 - (len(js) % 8)) % 8  # spec: header often padded with spaces
    js += b" " * pad
    return struct.pack("<Q", len(js)) + js, off


def torch_views(header: SafetensorsHeader, blob_u8):
    """Zero-copy tensor views over a landed blob (torch uint8 1-D tensor
    covering the WHOLE file, header included)."""
    import torch

    out = {}
    data0 = header.data_offset
    for t in header.tensors:
        raw = blob_u8[data0 + t.begin: data0 + t.end]
        dt = getattr(torch, t.torch_dtype)
        out[t.name] = raw.view(dt).view(t.shape)
    return out

"""FP8 block-scaled dequant kernel (csrc/fp8_dequant.hip) through _hip,
bit for bit against a torch CPU reference (fp8_fixtures.reference).

Every case runs with the destination inside a larger buffer filled with
a sentinel, and checks that the bytes on both sides of it are untouched.
"""

import ctypes

import numpy as np
import pytest
import torch

import fp8_fixtures as fx

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel bytes on each side of the destination
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def hipmod():
    from demodel_amd.gpu import have_gpu, hip

    assert have_gpu(), "gpu marker requires a GPU"
    return hip()


def _upload(h, data: bytes, stream):
    buf = h.DeviceBuffer(max(len(data), 1))
    if data:
        src = (ctypes.c_char * len(data)).from_buffer_copy(data)
        h.h2d_async(buf.ptr, ctypes.addressof(src), len(data),
                    stream.handle)
        stream.sync()
    return buf


def _download(h, buf, n, stream) -> bytearray:
    out = bytearray(n)
    addr = ctypes.addressof((ctypes.c_char * n).from_buffer(out))
    h.d2h_async(addr, buf.ptr, n, stream.handle)
    stream.sync()
    return out


def _bytes(t: torch.Tensor) -> bytes:
    return t.contiguous().view(torch.uint8).numpy().tobytes()


def _dequant(h, codes, scale, scale_tag, block, dst_dtype,
             src_off=0, scale_off=0, dst_off_elems=0) -> torch.Tensor:
    """Run the kernel on `codes` [R, C] with the source, the scale and
    the destination each placed at the given offset from a 256 B-aligned
    allocation; returns the destination as a CPU tensor."""
    s = h.Stream(0)
    R, C = codes.shape
    esz = 2 if dst_dtype == torch.bfloat16 else 4
    src = _upload(h, bytes(src_off) + _bytes(codes), s)
    sc = _upload(h, bytes(scale_off) + _bytes(scale), s)
    lo = GUARD + dst_off_elems * esz
    hi = lo + R * C * esz
    total = hi + GUARD
    dst = _upload(h, bytes([SENTINEL]) * total, s)
    assert src.ptr % 256 == 0 and sc.ptr % 256 == 0 and dst.ptr % 256 == 0
    h.fp8_block_dequant(src.ptr + src_off, sc.ptr + scale_off,
                        fx.SCALE_CODE[scale_tag], dst.ptr + lo,
                        fx.DST_CODE[dst_dtype], R, C, block[0], block[1],
                        s.handle)
    raw = _download(h, dst, total, s)
    assert raw[:lo] == bytes([SENTINEL]) * lo, "wrote before dst"
    assert raw[hi:] == bytes([SENTINEL]) * GUARD, "wrote past dst"
    if R * C == 0:
        return torch.empty((R, C), dtype=dst_dtype)
    return torch.frombuffer(bytearray(raw[lo:hi]),
                            dtype=dst_dtype).view(R, C)


def _check(h, shape, block, scale_tag="F32", dst_dtype=torch.bfloat16,
           seed=0, **offs):
    rng = np.random.default_rng(seed)
    codes = fx.draw_codes(rng, shape)
    grid = (-(-shape[0] // block[0]), -(-shape[1] // block[1]))
    scale = fx.draw_scales(rng, grid, scale_tag)
    got = _dequant(h, codes, scale, scale_tag, block, dst_dtype, **offs)
    fx.assert_dequant_equal(got, codes,
                            fx.reference(codes, scale, block, dst_dtype))


def test_decode_table_all_256_codes(hipmod):
    """Every code once, scale 1.0, f32 out: the e4m3fn decode itself."""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(1, 256)
    scale = torch.ones(1, dtype=torch.float32)
    got = _dequant(hipmod, codes, scale, "F32", (1, 256), torch.float32)
    want = fx.reference(codes, scale, (1, 256), torch.float32)
    fx.assert_dequant_equal(got, codes, want)
    g = got.view(-1)
    assert torch.isnan(g).nonzero().view(-1).tolist() == [0x7F, 0xFF]
    assert g[0x7E].item() == 448.0 and g[0xFE].item() == -448.0
    assert g.view(torch.int32)[0x80].item() == -2 ** 31        # -0.0
    assert g.view(torch.int32)[0x00].item() == 0
    # subnormals k * 2**-9, then the first normal 2**-6
    assert g[1:8].tolist() == [k * 2.0 ** -9 for k in range(1, 8)]
    assert g[8].item() == 2.0 ** -6
    assert g[0x38].item() == 1.0


def test_single_element(hipmod):
    _check(hipmod, (1, 1), (128, 128))


def test_edge_blocks_one_and_two_wide(hipmod):
    _check(hipmod, (129, 130), (128, 128))


@pytest.mark.parametrize("dst_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("scale_tag", ["F32", "BF16", "F16"])
def test_block_scaled_200x300(hipmod, scale_tag, dst_dtype):
    _check(hipmod, (200, 300), (128, 128), scale_tag, dst_dtype)


@pytest.mark.parametrize("dst_dtype", [torch.bfloat16, torch.float32])
def test_per_row_scales_odd_cols(hipmod, dst_dtype):
    """Odd cols: every row starts at another alignment on both sides."""
    _check(hipmod, (5, 37), (1, 37), "F32", dst_dtype)


def test_per_tensor_scale(hipmod):
    _check(hipmod, (33, 65), (33, 65), "BF16")


@pytest.mark.parametrize("dst_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("scale_off", [1, 2])
@pytest.mark.parametrize("src_off", [1, 3, 8])
@pytest.mark.parametrize("shape", [(3, 16), (3, 48)])
def test_any_alignment(hipmod, shape, src_off, scale_off, dst_dtype):
    """Source, scale and destination off their natural alignment; whole
    16-element runs, so the vector paths are the ones that must cope."""
    _check(hipmod, shape, (1, 32), "F32", dst_dtype, src_off=src_off,
           scale_off=scale_off, dst_off_elems=1)


@pytest.mark.parametrize("shape,block", [
    ((7, 100), (3, 24)),     # a run straddles two block columns
    ((7, 100), (2, 5)),      # blocks narrower than a run
    ((4, 64), (1, 1)),       # one scale per element
])
def test_blocks_not_a_multiple_of_the_run(hipmod, shape, block):
    _check(hipmod, shape, block, "F16", src_off=5, dst_off_elems=3)


def test_grid_stride_more_runs_than_one_pass(hipmod):
    """More runs than the largest grid covers in one pass: the stride
    loop over rows turns."""
    pass_elems, _ = hipmod.fp8_block_dequant_pass_limits()
    cols = 16 * 1024 + 1                   # 1025 runs a row, last 1 wide
    rows = pass_elems // 16 // 1025 + 5
    assert rows * 1025 * 16 > pass_elems
    assert rows * cols < 64 << 20          # a few tens of MB
    _check(hipmod, (rows, cols), (128, 128))


def test_grid_stride_row_wider_than_one_pass(hipmod):
    """A row with more runs than the grid's x extent covers: the stride
    loop along the row turns, and its last run is ragged."""
    _, pass_cols = hipmod.fp8_block_dequant_pass_limits()
    _check(hipmod, (5, pass_cols + 16 * 70 + 3), (128, 128), "BF16")


def test_empty_tensor_launches_nothing(hipmod):
    for shape in [(0, 16), (16, 0)]:
        got = _dequant(hipmod, torch.empty(shape, dtype=torch.uint8),
                       torch.ones(1), "F32", (128, 128), torch.bfloat16)
        assert got.numel() == 0


@pytest.mark.parametrize("kw", [
    {"block_rows": 0}, {"block_cols": 0}, {"block_rows": -1},
    {"scale_dtype": 3}, {"scale_dtype": -1}, {"dst_dtype": 2},
    {"rows": -1},
])
def test_bad_arguments_raise(hipmod, kw):
    h = hipmod
    s = h.Stream(0)
    src = _upload(h, bytes(256), s)
    sc = _upload(h, _bytes(torch.ones(4)), s)
    dst = _upload(h, bytes([SENTINEL]) * 1024, s)
    args = dict(src=src.ptr, scale=sc.ptr, scale_dtype=0, dst=dst.ptr,
                dst_dtype=0, rows=4, cols=16, block_rows=128,
                block_cols=128, stream=s.handle)
    args.update(kw)
    with pytest.raises(ValueError):
        h.fp8_block_dequant(**args)
    s.sync()
    assert _download(h, dst, 1024, s) == bytes([SENTINEL]) * 1024

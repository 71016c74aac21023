"""GGUF dequant kernels (csrc/gguf_dequant.hip) and cast_f32_to_bf16
(csrc/scatter.hip) through _hip, against the per-field oracle of
gguf_blocks: bit for bit wherever the f32 arithmetic is exact, under a
derived bound (gguf_blocks.assert_bound) where two terms are added.

Every case runs with the destination inside a larger buffer filled with
a sentinel and checks the 64 bytes on both sides of it; GGUF sources sit
32 bytes into a 256 B-aligned allocation, the alignment a GGUF file
promises its tensor data.
"""

import numpy as np
import pytest
import torch

import gguf_blocks as gb

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel bytes on each side of the destination
SENTINEL = 0xA5
SRC_OFF = 32


@pytest.fixture(scope="module")
def hipmod():
    from demodel_amd.gpu import have_gpu, hip

    assert have_gpu(), "gpu marker requires a GPU"
    return hip()


@pytest.fixture(scope="module")
def stream(hipmod):
    return hipmod.Stream(0)


def _src_at(data, off) -> torch.Tensor:
    """`data` (bytes or a uint8 device tensor) `off` bytes into a fresh
    256 B-aligned device allocation; returns the view that holds it."""
    if not isinstance(data, torch.Tensor):
        data = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    buf = torch.empty(off + data.numel(), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[off:].copy_(data)
    return buf[off:]


def _guarded(nbytes) -> torch.Tensor:
    buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8,
                     device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf


def _assert_guards(buf) -> None:
    assert bool((buf[:GUARD] == SENTINEL).all()), "wrote before dst"
    assert bool((buf[-GUARD:] == SENTINEL).all()), "wrote past dst"


def _launch(h, s, t, src, n_blocks) -> torch.Tensor:
    """Run the kernel of type `t` over a device source; returns the
    guarded destination's payload as an int16 device tensor."""
    sp = gb.SPECS[t]
    assert src.numel() == n_blocks * sp.nbytes
    buf = _guarded(n_blocks * sp.elems * 2)
    torch.cuda.synchronize()
    h.gguf_dequant(sp.qtype, src.data_ptr(), buf.data_ptr() + GUARD,
                   n_blocks, s.handle)
    s.sync()
    _assert_guards(buf)
    return buf[GUARD:-GUARD].view(torch.int16)


def _dequant(h, s, f) -> np.ndarray:
    """bf16 bits the kernel gives for the blocks of `f`."""
    out = _launch(h, s, f["t"], _src_at(gb.pack(f), SRC_OFF),
                  gb.n_blocks(f))
    return out.cpu().numpy().view(np.uint16)


# ---- (a) position map --------------------------------------------------

@pytest.mark.parametrize("t", gb.ALL)
def test_position_map(hipmod, stream, t):
    f = gb.onehot(t)
    got = _dequant(hipmod, stream, f)
    gb.check_bf16(f, got, exact=True)
    n = gb.SPECS[t].elems
    assert np.array_equal(got.reshape(n, n),
                          np.eye(n, dtype=np.uint16) * 0x3F80)


# ---- (b) scale-slot map ------------------------------------------------

@pytest.mark.parametrize("t", gb.ALL)
def test_scale_slot_map(hipmod, stream, t):
    f = gb.slot_map(t)
    gb.check_bf16(f, _dequant(hipmod, stream, f), exact=True)


# ---- (c) field extremes ------------------------------------------------

@pytest.mark.parametrize("t", gb.ALL)
def test_field_extremes(hipmod, stream, t):
    f = gb.extremes(t)
    gb.check_bf16(f, _dequant(hipmod, stream, f), exact=True)


# ---- (d) f16 fields ----------------------------------------------------

@pytest.mark.parametrize("t", gb.ALL)
def test_f16_fields(hipmod, stream, t):
    """q8_0: all 65536 patterns of d.  Subnormals, +-0, +-inf (inf * 0 is
    NaN) and NaNs in every f16 field of every type."""
    for label, f, exact in gb.f16_cases(t):
        try:
            gb.check_bf16(f, _dequant(hipmod, stream, f), exact)
        except AssertionError as e:
            raise AssertionError(f"{t} {label}: {e}") from None


# ---- (e) random finite blocks ------------------------------------------

@pytest.fixture(scope="module")
def random400():
    return {t: gb.random_blocks(t, 400) for t in gb.ALL}


@pytest.mark.parametrize("t", gb.ALL)
def test_random_finite_blocks(hipmod, stream, random400, t):
    f = random400[t]
    gb.check_bf16(f, _dequant(hipmod, stream, f), exact=t in gb.ONE_TERM)


# ---- (f) launch geometry -----------------------------------------------

@pytest.mark.parametrize("t,n", [(t, n) for t in gb.KTYPES
                                 for n in (1, 2, 3, 4, 5, 7)] +
                                [(t, n) for t in gb.LEGACY
                                 for n in (1, 2, 255, 256, 257)])
def test_partial_workgroups(hipmod, stream, random400, t, n):
    f = gb.take(random400[t], n)
    gb.check_bf16(f, _dequant(hipmod, stream, f), exact=t in gb.ONE_TERM)


def test_zero_blocks_launches_nothing(hipmod, stream):
    buf = _guarded(0)
    src = _src_at(bytes(256), SRC_OFF)
    torch.cuda.synchronize()
    for t in gb.ALL:
        hipmod.gguf_dequant(gb.SPECS[t].qtype, src.data_ptr(),
                            buf.data_ptr() + GUARD, 0, stream.handle)
    stream.sync()
    assert bool((buf == SENTINEL).all())


# ---- (g) grid-stride loop ----------------------------------------------

TILE = 4099     # blocks; prime, so every wave meets every tile position


@pytest.mark.parametrize("t", gb.ALL)
def test_grid_stride_loop(hipmod, stream, t):
    """The smallest sizes at which the 8192-workgroup grid goes round
    more than once.  The tile is checked against the oracle; the large
    run must then repeat the tile's output bit for bit, every block
    being computed on its own."""
    sp = gb.SPECS[t]
    n = 2 * 32768 + 5 if t in gb.KTYPES else 2097152 + 257
    assert -(-n // (4 if t in gb.KTYPES else 256)) > 8192
    f = gb.random_blocks(t, TILE, seed=1)
    tile_src = _src_at(gb.pack(f), SRC_OFF)
    tile_out = _launch(hipmod, stream, t, tile_src, TILE)
    gb.check_bf16(f, tile_out.cpu().numpy().view(np.uint16),
                  exact=t in gb.ONE_TERM)
    reps = -(-n // TILE)
    src = _src_at(tile_src.repeat(reps)[:n * sp.nbytes], SRC_OFF)
    got = _launch(hipmod, stream, t, src, n)
    want = tile_out.repeat(reps)[:n * sp.elems]
    assert torch.equal(got, want)


# ---- cast_f32_to_bf16 --------------------------------------------------

def _cast(h, s, x_bits: np.ndarray, src_off) -> np.ndarray:
    n = x_bits.size
    src = _src_at(x_bits.astype(np.uint32).tobytes(), src_off)
    buf = _guarded(n * 2)
    torch.cuda.synchronize()
    h.cast_f32_to_bf16(src.data_ptr(), buf.data_ptr() + GUARD, n, s.handle)
    s.sync()
    _assert_guards(buf)
    return buf[GUARD:-GUARD].view(torch.int16).cpu().numpy().view(np.uint16)


def _cast_inputs(n) -> np.ndarray:
    """n f32 bit patterns: the special values first, cycled, so that a
    short array still starts with a NaN, and every fourth one a random
    pattern."""
    rng = np.random.default_rng(n)
    x = np.resize(gb.CAST_SPECIALS, n).copy()
    x[3::4] = rng.integers(0, 2 ** 32, size=x[3::4].size, dtype=np.uint32)
    return x


@pytest.mark.parametrize("src_off", [0, 8])
def test_cast_special_values(hipmod, stream, src_off):
    got = _cast(hipmod, stream, gb.CAST_SPECIALS, src_off)
    gb.assert_same_bf16(got, gb.bf16_bits(gb.CAST_SPECIALS.view(np.float32)))
    # the ties, and the two finite values that round to inf
    by = dict(zip(gb.CAST_SPECIALS.tolist(), got.tolist()))
    assert by[0x3F808000] == 0x3F80 and by[0x3F818000] == 0x3F82
    assert by[0x7F7FFFFF] == 0x7F80 and by[0x7F7F8000] == 0x7F80
    assert by[0x00000001] == 0x0000 and by[0x80000001] == 0x8000
    assert by[0x007FFFFF] == 0x0080


@pytest.mark.parametrize("src_off", [0, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1025])
def test_cast_tail_sizes(hipmod, stream, n, src_off):
    x = _cast_inputs(n)
    got = _cast(hipmod, stream, x, src_off)
    gb.assert_same_bf16(got, gb.bf16_bits(x.view(np.float32)))


def test_cast_stride_loop(hipmod, stream):
    """One more than the 8192-workgroup grid covers in a pass, with a
    ragged tail; on the device against torch's own cast."""
    n = 8192 * 1024 + 3
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    x[-3:] = torch.tensor([1.00390625, -65280.0, 1.01171875], device="cuda")
    buf = _guarded(n * 2)
    torch.cuda.synchronize()
    hipmod.cast_f32_to_bf16(x.data_ptr(), buf.data_ptr() + GUARD, n,
                            stream.handle)
    stream.sync()
    _assert_guards(buf)
    want = x.to(torch.bfloat16).view(torch.int16)
    assert torch.equal(buf[GUARD:-GUARD].view(torch.int16), want)

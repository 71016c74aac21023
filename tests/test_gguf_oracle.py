"""gguf.dequant_cpu, the numpy reference the GGUF pipeline tests lean on,
against the per-field oracle of gguf_blocks: the same case families the
GPU kernels get in test_gpu_gguf_dequant.py, plus checks of the fixture
module itself.  No GPU needed.
"""

import numpy as np
import pytest
import torch

import gguf_blocks as gb
from demodel_amd.engine.formats import gguf


def _cpu(f) -> np.ndarray:
    sp = gb.SPECS[f["t"]]
    raw = gb.pack(f)
    return gguf.dequant_cpu(sp.qtype, raw, gb.n_blocks(f) * sp.elems)


@pytest.mark.parametrize("t", gb.ALL)
def test_packer_returns_block_bytes(t):
    sp = gb.SPECS[t]
    assert gguf.GGML_TYPES[sp.qtype] == (t, sp.elems, sp.nbytes)
    assert len(gb.pack(gb.uniform(t, 1))) == gguf.GGML_TYPES[sp.qtype][2]
    assert len(gb.pack(gb.random_blocks(t, 7))) == 7 * sp.nbytes


@pytest.mark.parametrize("t", gb.ALL)
def test_packer_fields_fill_disjoint_bits(t):
    """All fields at their all-ones value give an all-ones block: every
    bit of the block belongs to some field, and (bytes being ORed in) no
    two fields can then share one."""
    sp = gb.SPECS[t]
    top = {"q8_0": -1}.get(t, sp.qhi)
    f = gb.uniform(t, 1, d=0xFFFF, other=0xFFFF, q=top,
                   sc=-1 if t == "q6_K" else sp.schi, mn=sp.mnhi)
    assert gb.pack(f) == b"\xff" * sp.nbytes


def test_f16_value_all_patterns():
    bits = np.arange(65536, dtype=np.uint16)
    want = bits.view(np.float16).astype(np.float64)
    got = gb.f16_value(bits)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint64),
                          want[~nan].view(np.uint64))


def _torch_bf16_bits(x) -> np.ndarray:
    return (torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy()
            .view(np.uint16))


def test_bf16_bits_matches_torch_on_specials():
    """Bit for bit, but for the payload of a NaN: torch's own cast gives
    0x7FC0 or 0xFFFF depending on whether an element falls in a vector
    lane or in the scalar tail, so there a NaN has to meet a NaN."""
    x = gb.CAST_SPECIALS.view(np.float32)
    gb.assert_same_bf16(gb.bf16_bits(x), _torch_bf16_bits(x))
    assert np.isnan(x[:8]).all() and not np.isnan(x[8:]).any()
    assert np.array_equal(gb.bf16_bits(x)[8:], _torch_bf16_bits(x)[8:])


def test_bf16_bits_matches_torch_on_random_bits():
    u = np.random.default_rng(0).integers(0, 2 ** 32, size=200000,
                                          dtype=np.uint32)
    x = u.view(np.float32)
    gb.assert_same_bf16(gb.bf16_bits(x), _torch_bf16_bits(x))


@pytest.mark.parametrize("t", gb.ALL)
def test_position_map(t):
    f = gb.onehot(t)
    got = _cpu(f)
    gb.check_f32(f, got, exact=True)
    n = gb.SPECS[t].elems
    assert np.array_equal(got.reshape(n, n), np.eye(n, dtype=np.float32))


@pytest.mark.parametrize("t", gb.ALL)
def test_scale_slot_map(t):
    f = gb.slot_map(t)
    gb.check_f32(f, _cpu(f), exact=True)


@pytest.mark.parametrize("t", gb.ALL)
def test_field_extremes(t):
    f = gb.extremes(t)
    gb.check_f32(f, _cpu(f), exact=True)


@pytest.mark.parametrize("t", gb.ALL)
def test_f16_fields(t):
    for label, f, exact in gb.f16_cases(t):
        try:
            gb.check_f32(f, _cpu(f), exact)
        except AssertionError as e:
            raise AssertionError(f"{t} {label}: {e}") from None


@pytest.mark.parametrize("t", gb.ALL)
def test_random_finite_blocks(t):
    f = gb.random_blocks(t, 400)
    e = gb.expected(f)
    assert not (np.isnan(e.v) | np.isinf(e.v)).any()
    gb.check_f32(f, _cpu(f), exact=t in gb.ONE_TERM)


@pytest.mark.parametrize("t", gb.TWO_TERM)
def test_random_blocks_do_cancel(t):
    """The cancellation patterns are there: some elements are exactly 0
    with both terms live, some are far smaller than their terms."""
    e = gb.expected(gb.random_blocks(t, 400))
    live = (e.a > 0) & (e.b > 0)
    assert ((e.v == 0) & live).sum() > 100
    assert ((e.v != 0) & live & (np.abs(e.v) < 2.0 ** -9 * e.a)).sum() > 100


def test_comparisons_reject_two_bf16_ulps():
    """The comparison itself: a value two bf16 ulps off is refused, the
    correctly rounded one accepted."""
    f = gb.take(gb.random_blocks("q4_K", 4), 1)   # independent fields
    e = gb.expected(f)
    good = gb.bf16_bits(e.v.astype(np.float32))
    gb.assert_bound(gb.bf16_value(good), e)
    i = int(np.argmax(np.abs(e.v) > 4 * (e.a + e.b) * 2.0 ** -14))
    bad = good.copy().reshape(-1)
    bad[i] += 2
    with pytest.raises(AssertionError):
        gb.assert_bound(gb.bf16_value(bad), e)
    with pytest.raises(AssertionError):
        gb.assert_bits(bad, e.v.astype(np.float32).astype(np.float64))

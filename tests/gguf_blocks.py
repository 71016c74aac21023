"""Shared pieces of the GGUF dequant tests: block packers, a per-field
oracle and the case families both test files run.

Nothing here reads a packed block back.  A case is a dict of *fields*
(f16 bit patterns, integer sub-block scales and mins, one integer quant
code per element); `pack` scatters the fields into ggml block bytes and
`expected` computes the values in float64 straight from the same fields,
so the two never share a reading of the byte layout.  The code under
test (the HIP kernels, gguf.dequant_cpu) is the only thing that decodes.

Field conventions, every array with a leading block dimension:
  d, dmin, m   uint16 f16 bit patterns                       [nb]
  q            stored quant code, one per element            [nb, elems]
               (q8_0: the int8 value itself)
  sc, mn       stored sub-block scale / min                  [nb, slots]
               (q6_K: the int8 scale itself)
The value of an element is given per type in `expected`.
"""

from collections import namedtuple

import numpy as np

Spec = namedtuple("Spec", "qtype elems nbytes qlo qhi qzero f16 slots "
                          "sclo schi sczero mnhi")

# qzero: the code that decodes to 0; sczero: the stored scale that means 0
SPECS = {
    "q4_0": Spec(2, 32, 18, 0, 15, 8, ("d",), 0, 0, 0, 0, 0),
    "q4_1": Spec(3, 32, 20, 0, 15, 0, ("d", "m"), 0, 0, 0, 0, 0),
    "q5_0": Spec(6, 32, 22, 0, 31, 16, ("d",), 0, 0, 0, 0, 0),
    "q5_1": Spec(7, 32, 24, 0, 31, 0, ("d", "m"), 0, 0, 0, 0, 0),
    "q8_0": Spec(8, 32, 34, -128, 127, 0, ("d",), 0, 0, 0, 0, 0),
    "q2_K": Spec(10, 256, 84, 0, 3, 0, ("d", "dmin"), 16, 0, 15, 0, 15),
    "q3_K": Spec(11, 256, 110, 0, 7, 4, ("d",), 16, 0, 63, 32, 0),
    "q4_K": Spec(12, 256, 144, 0, 15, 0, ("d", "dmin"), 8, 0, 63, 0, 63),
    "q5_K": Spec(13, 256, 176, 0, 31, 0, ("d", "dmin"), 8, 0, 63, 0, 63),
    "q6_K": Spec(14, 256, 210, 0, 63, 32, ("d",), 16, -128, 127, 0, 0),
}
ALL = list(SPECS)
LEGACY = [t for t in ALL if SPECS[t].elems == 32]
KTYPES = [t for t in ALL if SPECS[t].elems == 256]
# one term, and the f32 product of its factors is exact: d carries at
# most 11 significant bits, a sub-block scale at most 7 (|int8| <= 127,
# 128 is a power of two), a quant at most 7 (q8_0) or 5
ONE_TERM = ["q4_0", "q5_0", "q8_0", "q3_K", "q6_K"]
TWO_TERM = [t for t in ALL if t not in ONE_TERM]

F16_ONE = 0x3C00
F16_ZERO = 0x0000


# ------------------------------------------------------------------ #
# number formats

def f16_value(bits) -> np.ndarray:
    """f16 bit patterns -> float64, by arithmetic on the three fields."""
    bits = np.asarray(bits, np.int64)
    sign = np.where(bits & 0x8000, -1.0, 1.0)
    e = (bits >> 10) & 31
    man = (bits & 0x3FF).astype(np.float64)
    mag = np.where(e == 0, np.ldexp(man, -24),
                   np.ldexp(1024.0 + man, e - 25))
    mag = np.where(e == 31, np.where(man == 0, np.inf, np.nan), mag)
    return sign * mag


def f16_bits(x) -> np.ndarray:
    """Values exactly representable in f16 -> their bit patterns."""
    h = np.asarray(x, np.float64).astype(np.float16)
    assert np.array_equal(h.astype(np.float64), np.asarray(x, np.float64))
    return h.view(np.uint16)


def bf16_bits(x) -> np.ndarray:
    """float32 -> bf16 bits, round to nearest, ties to even; every NaN
    becomes the canonical quiet NaN 0x7FC0."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    upper, lower = u >> 16, u & 0xFFFF
    up = (lower > 0x8000) | ((lower == 0x8000) & ((upper & 1) == 1))
    r = upper + up
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def bf16_value(bits) -> np.ndarray:
    u = np.asarray(bits, np.uint16).astype(np.uint32) << 16
    return u.view(np.float32).astype(np.float64)


# f32 bit patterns the cast tests use: NaNs quiet and signalling with
# several payloads, +-inf, +-0, the smallest and largest subnormals, ties
# on both sides of even, and two finite values that round up to inf
CAST_SPECIALS = np.array([
    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FC12345, 0x7FBFFFFF,
    0x7F80FFFF, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x3F808000, 0x3F818000,
    0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0x7F7F8000,
    0xFF7FFFFF, 0xFF7F8000, 0x7F7F7FFF, 0x3F800000, 0x00008000, 0x00018000,
], dtype=np.uint32)


# ------------------------------------------------------------------ #
# packers

def _nb(f) -> int:
    return int(np.asarray(f["d"]).reshape(-1).shape[0])


def _ints(f, key, n, lo, hi) -> np.ndarray:
    a = np.asarray(f[key], np.int64).reshape(_nb(f), n)
    assert a.min() >= lo and a.max() <= hi, (f["t"], key)
    return a


def _put_f16(blk, off, f, key) -> None:
    bits = np.asarray(f[key], np.int64).reshape(-1)
    assert bits.min() >= 0 and bits.max() <= 0xFFFF
    blk[:, off] = bits & 0xFF
    blk[:, off + 1] = bits >> 8


def _or(blk, col, val) -> None:
    blk[:, col] |= val.astype(np.uint8)


def _put_legacy_nibbles(blk, off, q4) -> None:
    for i in range(32):
        _or(blk, off + i % 16, q4[:, i] << (0 if i < 16 else 4))


def _put_legacy_qh(blk, off, q) -> None:
    qh = np.zeros(q.shape[0], np.int64)
    for i in range(32):
        qh |= ((q[:, i] >> 4) & 1) << i
    for k in range(4):
        blk[:, off + k] = (qh >> (8 * k)) & 0xFF


def _put_k4_scales(blk, off, sc, mn) -> None:
    """The 12-byte 6-bit scale/min packing of q4_K and q5_K."""
    for j in range(8):
        if j < 4:
            _or(blk, off + j, sc[:, j])
            _or(blk, off + j + 4, mn[:, j])
        else:
            _or(blk, off + j + 4, (sc[:, j] & 15) | ((mn[:, j] & 15) << 4))
            _or(blk, off + j - 4, (sc[:, j] >> 4) << 6)
            _or(blk, off + j, (mn[:, j] >> 4) << 6)


def _pack_q4_0(f, blk):
    _put_f16(blk, 0, f, "d")
    _put_legacy_nibbles(blk, 2, _ints(f, "q", 32, 0, 15))


def _pack_q4_1(f, blk):
    _put_f16(blk, 0, f, "d")
    _put_f16(blk, 2, f, "m")
    _put_legacy_nibbles(blk, 4, _ints(f, "q", 32, 0, 15))


def _pack_q5_0(f, blk):
    q = _ints(f, "q", 32, 0, 31)
    _put_f16(blk, 0, f, "d")
    _put_legacy_qh(blk, 2, q)
    _put_legacy_nibbles(blk, 6, q & 15)


def _pack_q5_1(f, blk):
    q = _ints(f, "q", 32, 0, 31)
    _put_f16(blk, 0, f, "d")
    _put_f16(blk, 2, f, "m")
    _put_legacy_qh(blk, 4, q)
    _put_legacy_nibbles(blk, 8, q & 15)


def _pack_q8_0(f, blk):
    _put_f16(blk, 0, f, "d")
    blk[:, 2:34] = _ints(f, "q", 32, -128, 127) & 0xFF


def _pack_q2_K(f, blk):
    q = _ints(f, "q", 256, 0, 3)
    sc = _ints(f, "sc", 16, 0, 15)
    mn = _ints(f, "mn", 16, 0, 15)
    blk[:, 0:16] = sc | (mn << 4)
    for i in range(256):
        n, r = divmod(i, 128)
        g, l = divmod(r, 32)
        _or(blk, 16 + 32 * n + l, q[:, i] << (2 * g))
    _put_f16(blk, 80, f, "d")
    _put_f16(blk, 82, f, "dmin")


def _pack_q3_K(f, blk):
    q = _ints(f, "q", 256, 0, 7)       # value q - 4: low two bits + hmask
    sc = _ints(f, "sc", 16, 0, 63)     # value sc - 32
    for i in range(256):
        n, r = divmod(i, 128)
        g, l = divmod(r, 32)
        _or(blk, 32 + 32 * n + l, (q[:, i] & 3) << (2 * g))
        _or(blk, l, (q[:, i] >> 2) << (4 * n + g))
    for k in range(16):
        low, high = sc[:, k] & 15, sc[:, k] >> 4
        if k < 8:
            _or(blk, 96 + k, low)
        else:
            _or(blk, 96 + k - 8, low << 4)
        _or(blk, 96 + 8 + k % 4, high << (2 * (k // 4)))
    _put_f16(blk, 108, f, "d")


def _pack_q4_K(f, blk):
    q = _ints(f, "q", 256, 0, 15)
    _put_f16(blk, 0, f, "d")
    _put_f16(blk, 2, f, "dmin")
    _put_k4_scales(blk, 4, _ints(f, "sc", 8, 0, 63), _ints(f, "mn", 8, 0, 63))
    for i in range(256):
        j = i // 32
        _or(blk, 16 + 32 * (i // 64) + i % 32, q[:, i] << (4 * (j % 2)))


def _pack_q5_K(f, blk):
    q = _ints(f, "q", 256, 0, 31)
    _put_f16(blk, 0, f, "d")
    _put_f16(blk, 2, f, "dmin")
    _put_k4_scales(blk, 4, _ints(f, "sc", 8, 0, 63), _ints(f, "mn", 8, 0, 63))
    for i in range(256):
        j = i // 32
        _or(blk, 16 + i % 32, (q[:, i] >> 4) << j)
        _or(blk, 48 + 32 * (i // 64) + i % 32, (q[:, i] & 15) << (4 * (j % 2)))


def _pack_q6_K(f, blk):
    q = _ints(f, "q", 256, 0, 63)      # value q - 32
    for i in range(256):
        n, r = divmod(i, 128)
        g, l = divmod(r, 32)
        low, high = q[:, i] & 15, q[:, i] >> 4
        if g < 2:
            _or(blk, 64 * n + 32 * g + l, low)
        else:
            _or(blk, 64 * n + 32 * (g - 2) + l, low << 4)
        _or(blk, 128 + 32 * n + l, high << (2 * g))
    blk[:, 192:208] = _ints(f, "sc", 16, -128, 127) & 0xFF
    _put_f16(blk, 208, f, "d")


_PACKERS = {"q4_0": _pack_q4_0, "q4_1": _pack_q4_1, "q5_0": _pack_q5_0,
            "q5_1": _pack_q5_1, "q8_0": _pack_q8_0, "q2_K": _pack_q2_K,
            "q3_K": _pack_q3_K, "q4_K": _pack_q4_K, "q5_K": _pack_q5_K,
            "q6_K": _pack_q6_K}


def pack(f) -> bytes:
    """The blocks of `f`, back to back: nb * block_bytes bytes."""
    blk = np.zeros((_nb(f), SPECS[f["t"]].nbytes), np.uint8)
    _PACKERS[f["t"]](f, blk)
    return blk.tobytes()


# ------------------------------------------------------------------ #
# oracle

Expected = namedtuple("Expected", "v a b")   # a, b: |terms|, two-term only


def expected(f) -> Expected:
    """Element values in float64 with IEEE semantics (inf * 0 = NaN).
    Every product here is exact in float64, and so is the difference of
    the two terms: together they span fewer than 53 bits."""
    t = f["t"]
    sp = SPECS[t]
    nb = _nb(f)
    q = np.asarray(f["q"], np.float64).reshape(nb, sp.elems)
    d = f16_value(f["d"]).reshape(nb, 1)
    per = sp.elems // sp.slots if sp.slots else 0

    def slots(key):
        a = np.asarray(f[key], np.float64).reshape(nb, sp.slots)
        return np.repeat(a, per, axis=1)

    with np.errstate(invalid="ignore"):
        if t in ("q4_0", "q5_0", "q8_0"):
            return Expected(d * (q - sp.qzero), None, None)
        if t in ("q3_K", "q6_K"):
            return Expected(d * (slots("sc") - sp.sczero) * (q - sp.qzero),
                            None, None)
        if t in ("q4_1", "q5_1"):
            a = d * q
            b = f16_value(f["m"]).reshape(nb, 1) * np.ones_like(q)
            return Expected(a + b, np.abs(a), np.abs(b))
        a = d * slots("sc") * q
        b = f16_value(f["dmin"]).reshape(nb, 1) * slots("mn")
        return Expected(a - b, np.abs(a), np.abs(b))


# ------------------------------------------------------------------ #
# comparison

def assert_same_bf16(got_bits, want_bits) -> None:
    """Equal bits, except that any NaN matches any NaN."""
    got = np.asarray(got_bits, np.uint16).reshape(-1)
    want = np.asarray(want_bits, np.uint16).reshape(-1)
    assert got.shape == want.shape
    nan = (want & 0x7FFF) > 0x7F80
    got_nan = (got & 0x7FFF) > 0x7F80
    assert np.array_equal(got_nan, nan), \
        f"NaN at {np.flatnonzero(got_nan != nan)[:8]}"
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, (
        f"{bad.size} wrong, first at {bad[:8]}: got "
        f"{[hex(x) for x in got[bad[:8]]]} want "
        f"{[hex(x) for x in want[bad[:8]]]}")


def assert_bits(got_bits, v) -> None:
    """`v` is exactly representable in f32 (asserted): the result must be
    its one correctly rounded bf16, sign of zero included; a NaN must be
    a NaN, whatever its payload."""
    v = np.asarray(v, np.float64).reshape(-1)
    got_bits = np.asarray(got_bits, np.uint16).reshape(-1)
    assert got_bits.shape == v.shape
    with np.errstate(over="raise"):
        v32 = v.astype(np.float32)
    nan = np.isnan(v)
    assert np.array_equal(v32.astype(np.float64)[~nan], v[~nan])
    assert_same_bf16(got_bits, bf16_bits(v32))


def assert_bound(got, e: Expected) -> None:
    """Two-term types: |got - exact| <= 2**-8 |exact| + 2**-22 (|a|+|b|).

    At most three f32 roundings of magnitude <= |a|+|b| (fewer when the
    compiler fuses), then one bf16 rounding with unit roundoff 2**-8.
    Where the exact value is NaN or infinite the result must be NaN, or
    the same infinity."""
    got = np.asarray(got, np.float64).reshape(-1)
    v, a, b = (np.asarray(x, np.float64).reshape(-1) for x in e)
    assert got.shape == v.shape
    nan, inf = np.isnan(v), np.isinf(v)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[inf], v[inf])
    num = ~(nan | inf)
    err = np.abs(got[num] - v[num])
    bound = 2.0 ** -8 * np.abs(v[num]) + 2.0 ** -22 * (a[num] + b[num])
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (
        f"{bad.size} outside the bound, first at {np.flatnonzero(num)[bad[:8]]}"
        f": err {err[bad[:8]]} bound {bound[bad[:8]]}")


def check_bf16(f, got_bits, exact: bool) -> None:
    """A kernel's bf16 output for the blocks of `f`."""
    e = expected(f)
    if exact:
        assert_bits(got_bits, e.v)
    else:
        assert_bound(bf16_value(got_bits), e)


def check_f32(f, got, exact: bool) -> None:
    """A float32 reference's output for the blocks of `f`: the same
    checks, and where the value is exact in f32, that very f32."""
    got = np.asarray(got, np.float32).reshape(-1)
    e = expected(f)
    if exact:
        assert_bits(bf16_bits(got), e.v)
        v = e.v.reshape(-1)
        nan = np.isnan(v)
        assert np.array_equal(got[~nan].view(np.uint32),
                              v[~nan].astype(np.float32).view(np.uint32))
    else:
        assert_bound(got, e)


# ------------------------------------------------------------------ #
# case families

def uniform(t, nb, d=F16_ONE, other=F16_ONE, q=None, sc=None, mn=0):
    """nb equal blocks: quants `q` (default: the code that decodes to 0),
    sub-block scales `sc` (default: the stored value that means 1)."""
    sp = SPECS[t]
    f = {"t": t, "d": np.full(nb, d, np.int64),
         "q": np.full((nb, sp.elems), sp.qzero if q is None else q,
                      np.int64)}
    if len(sp.f16) == 2:
        f[sp.f16[1]] = np.full(nb, other, np.int64)
    if sp.slots:
        f["sc"] = np.full((nb, sp.slots),
                          sp.sczero + 1 if sc is None else sc, np.int64)
        if sp.mnhi:
            f["mn"] = np.full((nb, sp.slots), mn, np.int64)
    return f


def take(f, n):
    return {k: (v if k == "t" else v[:n]) for k, v in f.items()}


def concat(fs):
    return {k: (fs[0]["t"] if k == "t" else
                np.concatenate([f[k] for f in fs])) for k in fs[0]}


def n_blocks(f) -> int:
    return _nb(f)


def onehot(t):
    """(a) block k: every quant decodes to 0 except element k, which
    decodes to 1; d = 1, sub-scales 1, mins 0 (legacy m = 0)."""
    sp = SPECS[t]
    other = F16_ZERO if t in LEGACY else F16_ONE
    f = uniform(t, sp.elems, other=other)
    k = np.arange(sp.elems)
    f["q"][k, k] = sp.qzero + 1
    return f


def slot_map(t):
    """(b) every quant decodes to 1, d = dmin = 1, slot j holds scale
    j + 1 and min 2j + 1.  q2_K's fields are 4 bits wide and cannot hold
    16 or 31: its 16 slots get two different permutations of 0..15.
    Legacy types have one scale a block: block k gets d = k + 1 and
    m = 2k + 1."""
    sp = SPECS[t]
    if not sp.slots:
        k = np.arange(5)
        f = uniform(t, 5, q=sp.qzero + 1)
        f["d"] = f16_bits(k + 1.0).astype(np.int64)
        if "m" in f:
            f["m"] = f16_bits(2.0 * k + 1).astype(np.int64)
        return f
    f = uniform(t, 1, q=sp.qzero + 1)
    j = np.arange(sp.slots)
    if t == "q2_K":
        f["sc"][0] = (j + 1) % 16
        f["mn"][0] = (7 * j + 3) % 16
    else:
        f["sc"][0] = sp.sczero + j + 1
        if sp.mnhi:
            f["mn"][0] = 2 * j + 1
    return f


def _each_slot_value(t, key, values, bg):
    """One block per (slot, value): that slot of `key` holds the value,
    the other slots `bg`."""
    sp = SPECS[t]
    nv = len(values)
    f = uniform(t, sp.slots * nv, q=sp.qzero + 1)
    f[key][:] = bg
    f[key][np.arange(sp.slots * nv),
           np.repeat(np.arange(sp.slots), nv)] = np.tile(values, sp.slots)
    return f


def extremes(t):
    """(c) field extremes, d = dmin = 1 (legacy m = 1): results are
    integers below 2**24, exact in f32."""
    sp = SPECS[t]
    fs = []
    if sp.slots:
        # every stored scale value in every slot, the others all-zero
        # bits and all-one bits (q6_K: the int8 range)
        vals = np.arange(sp.sclo, sp.schi + 1)
        for bg in sorted({sp.sclo, sp.schi, 0}):
            fs.append(_each_slot_value(t, "sc", vals, bg))
        if sp.mnhi:
            for bg in (0, sp.mnhi):
                fs.append(_each_slot_value(
                    t, "mn", np.arange(sp.mnhi + 1), bg))
    # every quant at its minimum and maximum: alone, interleaved at every
    # power-of-two period (so that two elements any layout could confuse
    # differ), and drawn at random
    i = np.arange(sp.elems)
    pats = [np.full(sp.elems, sp.qlo), np.full(sp.elems, sp.qhi)]
    period = 1
    while period < sp.elems:
        pats.append(np.where((i // period) % 2 == 0, sp.qlo, sp.qhi))
        pats.append(np.where((i // period) % 2 == 0, sp.qhi, sp.qlo))
        period *= 2
    rng = np.random.default_rng(sp.qtype)
    pats.append(rng.choice([sp.qlo, sp.qhi], size=sp.elems))
    pats.append(rng.integers(sp.qlo, sp.qhi + 1, size=sp.elems))
    scs = (sp.sclo, sp.schi, sp.sczero + 1) if sp.slots else (None,)
    for sc in scs:
        for mn in ((0, sp.mnhi) if sp.mnhi else (0,)):
            for p in pats:
                f = uniform(t, 1, sc=sc, mn=mn)
                f["q"][0] = p
                fs.append(f)
    # each bit of each element's code set alone (q5_0, q5_1, q5_K: bit 4
    # lives in qh; q3_K: bit 2 in hmask; q6_K: bits 4 and 5 in qh), and
    # cleared alone
    k = np.arange(sp.elems)
    nbits = (sp.qhi - sp.qlo).bit_length()
    for b in range(nbits):
        for bg in (0, (1 << nbits) - 1):
            f = uniform(t, sp.elems, q=bg)
            f["q"][k, k] = bg ^ (1 << b)
            if t == "q8_0":
                f["q"] = (f["q"] ^ 0x80) - 0x80      # as int8
            fs.append(f)
    return concat(fs)


def f16_patterns() -> np.ndarray:
    """(d) every exponent with mantissas 0x000, 0x001 and 0x3FF in both
    signs (that holds +-0, +-inf, subnormals 0x0001 and 0x03FF and NaN
    0x7C01), subnormal 0x0200, NaNs 0x7E00 and 0xFE00."""
    p = [s | (e << 10) | m for s in (0, 0x8000) for e in range(32)
         for m in (0x000, 0x001, 0x3FF)]
    p += [0x0200, 0x7E00, 0xFE00]
    for must in (0x0001, 0x0200, 0x03FF, 0x0000, 0x8000, 0x7C00, 0xFC00,
                 0x7E00, 0x7C01, 0xFE00):
        assert must in p
    return np.array(p, np.int64)


def _varied(t, nb):
    """Random quants, scales and mins; in every block the quant that
    decodes to 0 and the scale and min that mean 0 are there (so that
    they meet every d: inf * 0), and the extremes of each."""
    sp = SPECS[t]
    rng = np.random.default_rng([7, sp.qtype])
    f = uniform(t, nb)
    f["q"] = rng.integers(sp.qlo, sp.qhi + 1, size=(nb, sp.elems))
    f["q"][:, 0], f["q"][:, 1], f["q"][:, 2] = sp.qzero, sp.qlo, sp.qhi
    if sp.slots:
        f["sc"] = rng.integers(sp.sclo, sp.schi + 1, size=(nb, sp.slots))
        f["sc"][:, 1], f["sc"][:, 2] = sp.sczero, sp.schi
        if sp.mnhi:
            f["mn"] = rng.integers(0, sp.mnhi + 1, size=(nb, sp.slots))
            f["mn"][:, 0], f["mn"][:, 3] = 0, sp.mnhi
    return f


def f16_cases(t):
    """(d) [(label, fields, exact)]: one block per f16 pattern, for each
    f16 field of the type.  Two-term types run each field twice: with
    the other term exactly +0, where the result is one exact f32 product
    and compares in bits, and with the other term live, under the bound."""
    sp = SPECS[t]
    pats = f16_patterns()
    if t == "q8_0":
        pats = np.arange(65536, dtype=np.int64)
    nb = len(pats)
    out = []
    if t in ONE_TERM:
        f = _varied(t, nb)
        f["d"] = pats
        return [("d", f, True)]
    first, second = sp.f16
    # first term alone: the second is +0 (m = 0, or mins 0 with dmin = 1)
    f = _varied(t, nb)
    f[first] = pats
    if t in LEGACY:
        f[second][:] = F16_ZERO
    else:
        f["mn"][:] = 0
    out.append((first + "-alone", f, True))
    # second term alone: d = 1 and every quant 0
    f = _varied(t, nb)
    f[second] = pats
    f["q"][:] = 0
    out.append((second + "-alone", f, True))
    # both live, the other f16 field 1.0
    for key in (first, second):
        f = _varied(t, nb)
        f[key] = pats
        out.append((key + "-live", f, False))
    return out


def random_blocks(t, n, seed=0):
    """(e) n blocks of independent finite fields; in two-term types three
    blocks in four carry a cancellation pattern: dmin == d, then also
    min == scale with half the quants 1 (the terms cancel exactly), then
    d and dmin one f16 ulp apart.  Legacy: m = -d, and one ulp off it."""
    sp = SPECS[t]
    rng = np.random.default_rng([seed, sp.qtype])
    f = uniform(t, n)

    def finite_f16(size):
        bits = rng.integers(0, 0x7C00, size=size)
        bits[::13] &= 0x03FF                      # subnormals and zero
        return bits | (rng.integers(0, 2, size=size) << 15)

    def ulp_off(bits):
        mag = bits & 0x7FFF
        return (bits & 0x8000) | np.where(mag >= 0x7BFF, mag - 1, mag + 1)

    f["d"] = finite_f16(n)
    f["q"] = rng.integers(sp.qlo, sp.qhi + 1, size=(n, sp.elems))
    if sp.slots:
        f["sc"] = rng.integers(sp.sclo, sp.schi + 1, size=(n, sp.slots))
        if sp.mnhi:
            f["mn"] = rng.integers(0, sp.mnhi + 1, size=(n, sp.slots))
    if t in ONE_TERM:
        return f
    second = sp.f16[1]
    f[second] = finite_f16(n)
    k = np.arange(n) % 4
    if t in LEGACY:
        f[second] = np.where(k >= 1, f["d"] ^ 0x8000, f[second])
        f[second] = np.where(k == 3, ulp_off(f[second]), f[second])
    else:
        f[second] = np.where(k >= 1, f["d"], f[second])
        f[second] = np.where(k == 3, ulp_off(f[second]), f[second])
        same = k >= 2
        f["mn"][same] = np.minimum(f["sc"][same], sp.mnhi)
        f["sc"][same] = f["mn"][same]
    ones = (np.arange(n)[:, None] % 4 >= 2) & (
        np.arange(sp.elems)[None, :] % 2 == 0)
    f["q"] = np.where(ones, 1, f["q"])
    return f

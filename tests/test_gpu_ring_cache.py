"""The native landing ring and the pinned-slab / stream / event caches
under it, on a real GPU: ring wrap, reuse after destruction, the
DEMODEL_PINNED_CACHE_MB=0 switch, steady state over repeated pulls, and
concurrent lander churn."""

import ctypes
import gc
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VC = 64 << 10
SLAB = 64 << 10
CLASS = 2 << 20            # pinned size class of a 64 KiB slab
WRAP_BYTES = (1 << 20) + 13  # 17 laps of a 2-slab ring, ragged last slab


def _fill_from(data):
    pos = [0]

    def fill(view):
        n = min(len(view), len(data) - pos[0])
        view[:n] = data[pos[0]:pos[0] + n]
        pos[0] += n
        return n

    return fill


def _slab_addrs(lander):
    """Slab addresses read off the views: slab_ptr() would mark the ring
    as raw-used and change what its destructor does."""
    return sorted(
        ctypes.addressof(ctypes.c_char.from_buffer(lander.pool.slab_view(i)))
        for i in range(lander.pool.n_slabs))


def _land_and_check(lander, data):
    blob = lander.land(_fill_from(data), len(data))
    assert blob.torch_u8().cpu().numpy().tobytes() == data
    assert blob.chunk_digests == [
        hashlib.sha256(data[o:o + VC]).hexdigest()
        for o in range(0, len(data), VC)]


def _wrap_then_reuse():
    """Ring-wrap landing, then destroy + rebuild with the same geometry
    and land different data.  Returns the stats and slab addresses around
    the rebuild."""
    from demodel_amd.engine.pipeline import Lander
    from demodel_amd.gpu import hip

    h = hip()
    a = Lander(slab_bytes=SLAB, n_slabs=2, verify_chunk=VC)
    addrs_a = _slab_addrs(a)
    _land_and_check(a, os.urandom(WRAP_BYTES))
    del a
    gc.collect()
    s1 = h.cache_stats()
    b = Lander(slab_bytes=SLAB, n_slabs=2, verify_chunk=VC)
    s2 = h.cache_stats()
    addrs_b = _slab_addrs(b)
    _land_and_check(b, os.urandom(WRAP_BYTES))
    del b
    gc.collect()
    return s1, s2, addrs_a, addrs_b, h.cache_stats()


def test_ring_wrap_and_reuse():
    s1, s2, addrs_a, addrs_b, _ = _wrap_then_reuse()
    for kind, n in (("pinned", 2), ("streams", 2), ("events", 2)):
        assert s2[kind]["misses"] == s1[kind]["misses"], (kind, s1, s2)
        assert s2[kind]["hits"] == s1[kind]["hits"] + n, (kind, s1, s2)
    assert s2["pinned"]["bytes_live"] == s1["pinned"]["bytes_live"] \
        + 2 * CLASS
    assert s2["pinned"]["bytes_cached"] == s1["pinned"]["bytes_cached"] \
        - 2 * CLASS
    assert addrs_b == addrs_a


def test_cap_zero_disables_caching():
    env = dict(os.environ, DEMODEL_PINNED_CACHE_MB="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)],
                       env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    s = json.loads(r.stdout.strip().splitlines()[-1])
    for kind in ("pinned", "streams", "events"):
        assert s[kind]["hits"] == 0, s
        assert s[kind]["bytes_cached"] == 0, s
        assert s[kind]["bytes_live"] == 0, s
        assert s[kind]["cap_bytes"] == 0, s
    assert s["pinned"]["misses"] == 4 and s["pinned"]["freed"] == 4, s


def test_steady_state_pulls(tmp_path, monkeypatch):
    import torch

    from helpers import Stack

    from demodel_amd.engine import pull as pull_mod
    from demodel_amd.engine.formats import safetensors as st
    from demodel_amd.gpu import hip

    h = hip()
    rng = np.random.default_rng(7)
    src = {}
    files = {}
    for k in range(2):
        arrs = {f"f{k}.t{j}": rng.standard_normal(
            (768, 512 + 8 * j)).astype(np.float32) for j in range(4)}
        head, _ = st.build_header(
            {n: ("F32", a.shape, a.nbytes) for n, a in arrs.items()})
        p = tmp_path / f"m{k}.safetensors"
        p.write_bytes(head + b"".join(a.tobytes() for a in arrs.values()))
        assert p.stat().st_size > 6 << 20
        files[p.name] = str(p)
        src.update(arrs)

    monkeypatch.setattr(pull_mod, "SEGMENT_MIN", 1 << 20)
    stack = Stack(tmp_path)
    try:
        stack.origin.add_hf_repo("org/ring", files)
        landers = pull_mod.LanderPool(0, slab_bytes=256 << 10)
        stats = []
        for _ in range(3):
            res = pull_mod.pull_hf("org/ring", endpoint=stack.origin_base,
                                   workers=4, verify="chunked",
                                   landers=landers, slab_bytes=256 << 10)
            got = res.tensors()
            assert set(got) == set(src)
            for n, a in src.items():
                assert torch.equal(got[n].cpu(), torch.from_numpy(a)), n
            del got
            landers.recycle(res)
            del res
            gc.collect()
            stats.append(h.cache_stats())
    finally:
        stack.close()
    s2, s3 = stats[1], stats[2]
    for kind in ("pinned", "streams", "events"):
        assert s3[kind]["misses"] == s2[kind]["misses"], (kind, stats)
        assert s3[kind]["bytes_live"] <= s2[kind]["bytes_live"], \
            (kind, stats)
    assert s3["pinned"]["hits"] > s2["pinned"]["hits"]


def test_concurrent_lander_churn():
    from demodel_amd.engine.pipeline import Lander
    from demodel_amd.gpu import hip

    h = hip()
    gc.collect()
    s0 = h.cache_stats()
    errors = []
    start = threading.Barrier(8)

    def work(t):
        try:
            start.wait()
            for r in range(3):
                data = hashlib.sha256(b"%d.%d" % (t, r)).digest() \
                    * ((512 << 10) // 32)
                lander = Lander(slab_bytes=SLAB, n_slabs=2,
                                verify_chunk=VC)
                _land_and_check(lander, data)
                del lander
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    gc.collect()
    s1 = h.cache_stats()
    p0, p1 = s0["pinned"], s1["pinned"]
    assert p1["bytes_live"] == p0["bytes_live"]
    takes = (p1["hits"] - p0["hits"]) + (p1["misses"] - p0["misses"])
    assert takes == 8 * 3 * 2
    # every slab allocated for this test is either idle in the cache or
    # was freed over the cap: none lost, none counted twice
    kept = (p1["misses"] - p0["misses"]) - (p1["freed"] - p0["freed"])
    assert p1["bytes_cached"] - p0["bytes_cached"] == kept * CLASS
    assert p1["bytes_cached"] <= p1["cap_bytes"]
    for kind in ("streams", "events"):
        assert s1[kind]["bytes_live"] == s0[kind]["bytes_live"], kind


if __name__ == "__main__":
    # child of test_cap_zero_disables_caching: same sequence, stats out
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    import demodel_amd.gpu  # noqa: F401  (torch first, then _hip)

    _, _, _, _, final = _wrap_then_reuse()
    print(json.dumps(final))

"""Range-resume tests: the engine survives mid-stream connection drops
(Range continuation), and the proxy serves Range slices from cache."""

import hashlib
import os
import urllib.request

import pytest

from demodel_amd.engine import pull as pull_mod
from helpers import Stack, host_landers


@pytest.fixture()
def stack(tmp_path):
    s = Stack(tmp_path)
    yield s
    s.close()


def test_pull_resumes_after_drop(stack, tmp_path):
    data = os.urandom(2 << 20)
    p = tmp_path / "big.bin"
    p.write_bytes(data)
    stack.origin.add_hf_repo("org/r", {"big.bin": str(p)})
    # the first GET of the blob dies after 300 KiB
    stack.origin.drop_once["big.bin"] = 300 << 10

    # small slabs so the drop at 300 KiB leaves a completed-slab prefix
    # and the resume continues WITH a Range request
    res = pull_mod.pull_hf("org/r", endpoint=stack.origin_base,
                           verify="digest", workers=1,
                           landers=host_landers(slab_bytes=256 << 10))
    f = res.files[0]
    assert f.nbytes == len(data)
    assert f.blob.sha256 == hashlib.sha256(data).hexdigest()
    assert f.digest_ok is True
    assert bytes(f.blob.buffer) == data
    # blob.head must survive the resume (it is rebuilt from the landed
    # buffer — the in-flight capture restarts at the resume offset)
    assert f.blob.head == data[:len(f.blob.head)]
    assert len(f.blob.head) == len(data)  # head_bytes default > 2 MiB
    assert not stack.origin.drop_once  # fault fired
    # origin saw the blob requested twice (original + resume)
    blob_gets = [r for r in stack.origin.requests
                 if r.startswith("GET") and "big.bin" in r
                 and "/cdn/" in r]
    assert len(blob_gets) == 2


def test_resume_past_head_keeps_head(stack, tmp_path):
    """Drop AFTER head_bytes: the resumed stream never sees byte 0, yet
    blob.head must still be the true file prefix (ADVICE round-1
    medium: head was lost / captured from the resume offset)."""
    from demodel_amd.engine.pull import LanderPool

    data = os.urandom(2 << 20)
    p = tmp_path / "late.bin"
    p.write_bytes(data)
    stack.origin.add_hf_repo("org/late", {"late.bin": str(p)})
    stack.origin.drop_once["late.bin"] = 1 << 20  # drop at 1 MiB
    landers = LanderPool(0, slab_bytes=128 << 10, head_bytes=64 << 10)
    res = pull_mod.pull_hf("org/late", endpoint=stack.origin_base,
                           verify="digest", workers=1, landers=landers)
    f = res.files[0]
    assert f.blob.sha256 == hashlib.sha256(data).hexdigest()
    assert f.blob.head == data[:64 << 10]
    assert not stack.origin.drop_once


def test_pull_fails_when_retries_exhausted(stack, tmp_path, monkeypatch):
    data = os.urandom(1 << 20)
    p = tmp_path / "cursed.bin"
    p.write_bytes(data)
    stack.origin.add_hf_repo("org/c", {"cursed.bin": str(p)})
    stack.origin.drop_once["cursed.bin"] = 100
    import demodel_amd.engine.pull as pm

    monkeypatch.setattr(pm, "RESUME_RETRIES", 0)
    with pytest.raises(IOError):
        pull_mod.pull_hf("org/c", endpoint=stack.origin_base,
                         verify="chunked", workers=1)


def test_proxy_serves_range_from_cache(stack, tmp_path):
    data = os.urandom(500_000)
    p = tmp_path / "r.bin"
    p.write_bytes(data)
    stack.origin.add_hf_repo("org/rr", {"r.bin": str(p)})
    url = f"{stack.endpoint}/org/rr/resolve/main/r.bin"
    # prime the cache
    with urllib.request.urlopen(url, timeout=20) as r:
        assert r.read() == data

    req = urllib.request.Request(url, headers={"Range": "bytes=1000-4999"})
    with urllib.request.urlopen(req, timeout=20) as r:
        assert r.status == 206
        assert r.headers["X-Demodel-Cache"] == "HIT"
        assert r.headers["Content-Range"] == \
            f"bytes 1000-4999/{len(data)}"
        assert r.read() == data[1000:5000]

    # suffix range
    req = urllib.request.Request(url, headers={"Range": "bytes=-100"})
    with urllib.request.urlopen(req, timeout=20) as r:
        assert r.status == 206
        assert r.read() == data[-100:]


@pytest.mark.gpu
class TestSegmentedResume:
    """Range-parallel pulls survive drops in any segment."""

    def _pull(self, stack, tmp_path, monkeypatch, drop_key, drop_at):
        import demodel_amd.engine.pull as pm

        monkeypatch.setattr(pm, "SEGMENT_MIN", 1 << 20)
        data = os.urandom(5 << 20)
        p = tmp_path / "seg.bin"
        p.write_bytes(data)
        stack.origin.add_hf_repo("org/seg", {"seg.bin": str(p)})
        stack.origin.drop_once[drop_key] = drop_at
        res = pull_mod.pull_hf("org/seg", endpoint=stack.origin_base,
                               verify="chunked", workers=2)
        f = [x for x in res.files if x.name == "seg.bin"][0]
        assert f.nbytes == len(data)
        assert not stack.origin.drop_once  # fault fired
        got = bytes(f.blob.torch_u8().cpu().numpy().tobytes())
        assert got == data
        # seg-0 fallback must not lose the head (rebuilt via D2H)
        assert f.blob.head == data[:len(f.blob.head)]
        assert len(f.blob.head) == len(data)  # < head_bytes default
        del res, f

    def test_drop_in_segment0(self, stack, tmp_path, monkeypatch):
        # the probe stream (segment 0) dies after 300 KiB
        self._pull(stack, tmp_path, monkeypatch, "seg.bin", 300 << 10)

    def test_drop_in_later_segment(self, stack, tmp_path, monkeypatch):
        # the range GET for the segment starting at 2 MiB dies early
        self._pull(stack, tmp_path, monkeypatch,
                   f"seg.bin@{2 << 20}", 100 << 10)

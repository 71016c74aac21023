"""FP8 block-scaled safetensors through load_into on the GPU: landed
blob -> bf16/f32 params, bit for bit against a torch CPU reference
(fp8_fixtures.reference, never the loader's own CPU branch)."""

import pytest
import torch

import fp8_fixtures as fx
from helpers import Stack

from demodel_amd.engine.formats import safetensors as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_pull(tmp_path_factory):
    from demodel_amd.engine import pull as pull_mod
    from demodel_amd.gpu import have_gpu

    assert have_gpu()
    tmp = tmp_path_factory.mktemp("fp8gpu")
    stack = Stack(tmp)
    try:
        p = tmp / "m.safetensors"
        t = fx.build_fp8_checkpoint(str(p))
        stack.origin.add_hf_repo("o/fp8", {"m.safetensors": str(p)})
        res = pull_mod.pull_hf("o/fp8", endpoint=stack.origin_base,
                               workers=1)
        blob = res.files[0].blob
        assert blob.device != "cpu"
        yield blob, st.parse_header(blob.head), t
    finally:
        stack.close()


def test_load_into_fp8_block_scaled(gpu_pull):
    from demodel_amd.engine.loader import load_into

    blob, hdr, t = gpu_pull
    targets = {k: torch.zeros(tuple(t[k].shape), dtype=torch.bfloat16,
                              device="cuda")
               for k in ("a.weight", "b.weight", "n.weight", "e.weight")}
    targets["pad"] = torch.zeros(3, dtype=torch.uint8, device="cuda")
    # strict: the two scale tensors must not count as missing from the model
    loaded = load_into(blob, hdr, targets, strict=True)
    assert sorted(loaded) == sorted(targets)
    want = fx.expected_bf16(t)
    fx.assert_dequant_equal(targets["a.weight"].cpu(), t["a.weight"],
                            want["a.weight"])
    fx.assert_dequant_equal(targets["b.weight"].cpu(), t["b.weight"],
                            want["b.weight"])
    assert torch.equal(targets["n.weight"].cpu(), want["n.weight"])
    assert torch.equal(targets["e.weight"].cpu(), want["e.weight"])
    assert targets["pad"].cpu().tolist() == [1, 2, 3]


def test_load_into_fp8_f32_target_and_fp8_target(gpu_pull):
    from demodel_amd.engine.loader import load_into

    blob, hdr, t = gpu_pull
    a32 = torch.zeros(200, 300, dtype=torch.float32, device="cuda")
    b8 = torch.zeros(64, 48, dtype=torch.float8_e4m3fn, device="cuda")
    load_into(blob, hdr, {"a.weight": a32, "b.weight": b8}, strict=False)
    fx.assert_dequant_equal(
        a32.cpu(), t["a.weight"],
        fx.reference(t["a.weight"], t["a.weight_scale_inv"], (128, 128),
                     torch.float32))
    # FP8 into an FP8 target stays a plain scatter of the codes
    assert torch.equal(b8.view(torch.uint8).cpu(), t["b.weight"])


def test_load_into_fp8_explicit_block_size(gpu_pull):
    """weight_block_size as a config.json states it, passed down."""
    from demodel_amd.engine.loader import load_into

    blob, hdr, t = gpu_pull
    a = torch.zeros(200, 300, dtype=torch.bfloat16, device="cuda")
    load_into(blob, hdr, {"a.weight": a}, strict=False,
              fp8_block_size=[128, 128])
    fx.assert_dequant_equal(a.cpu(), t["a.weight"],
                            fx.expected_bf16(t)["a.weight"])


def _gpu_blob(tmp_path, spec, payload):
    from demodel_amd.engine import pull as pull_mod

    head, _ = st.build_header(spec)
    stack = Stack(tmp_path)
    try:
        p = tmp_path / "m.safetensors"
        p.write_bytes(head + payload)
        stack.origin.add_hf_repo("o/x", {"m.safetensors": str(p)})
        res = pull_mod.pull_hf("o/x", endpoint=stack.origin_base,
                               workers=1)
    finally:
        stack.close()
    blob = res.files[0].blob
    return blob, st.parse_header(blob.head)


def _untouched(dst):
    torch.cuda.synchronize()
    return bool((dst.view(torch.int16) == 0x1234).all().item())


def test_fp8_errors_raise_before_any_launch(tmp_path):
    from demodel_amd.engine.loader import load_into

    w = ("F8_E4M3", (4, 8), 32)
    dst = torch.full((4, 8), 0x1234, dtype=torch.int16,
                     device="cuda").view(torch.bfloat16)
    other = torch.full((4,), 0x1234, dtype=torch.int16,
                       device="cuda").view(torch.bfloat16)
    plain = ("BF16", (4,), 8)

    # an FP8 weight with no scale tensor, going to a wider target
    blob, hdr = _gpu_blob(tmp_path / "a", {"p": plain, "w": w}, bytes(40))
    with pytest.raises(ValueError, match="no scale tensor"):
        load_into(blob, hdr, {"p": other, "w": dst}, strict=False)
    assert _untouched(dst) and _untouched(other)

    # a scale shape that fits no block
    blob, hdr = _gpu_blob(
        tmp_path / "b",
        {"p": plain, "w": w, "w_scale_inv": ("F32", (3, 3), 36)},
        bytes(8 + 32 + 36))
    with pytest.raises(ValueError, match="fits no block"):
        load_into(blob, hdr, {"p": other, "w": dst}, strict=False)
    assert _untouched(dst) and _untouched(other)

    # a crafted header: the scale's extent runs past the landed blob
    blob, hdr = _gpu_blob(
        tmp_path / "c",
        {"p": plain, "w": w, "w_scale_inv": ("F32", (4, 1), 16)},
        bytes(8 + 32 + 4))
    assert hdr.data_offset + hdr.tensors[-1].end > blob.nbytes
    with pytest.raises(ValueError, match="does not fit the blob"):
        load_into(blob, hdr, {"p": other, "w": dst}, strict=False)
    assert _untouched(dst) and _untouched(other)

    # ... and a scale whose byte count disagrees with its shape
    blob, hdr = _gpu_blob(
        tmp_path / "d",
        {"p": plain, "w": w, "w_scale_inv": ("F32", (4, 1), 4)},
        bytes(8 + 32 + 4))
    with pytest.raises(ValueError, match="does not fit the blob"):
        load_into(blob, hdr, {"p": other, "w": dst}, strict=False)
    assert _untouched(dst) and _untouched(other)

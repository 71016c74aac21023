"""pull_pretrained(dequantize=True) on the GPU: an FP8 block-scaled
checkpoint pulled into HBM and widened there into a plain bf16
transformers model (tests/test_fp8_safetensors.py has the same on a host
landing)."""

import gc

import pytest
import torch

import fp8_fixtures as fx
from helpers import Stack

transformers = pytest.importorskip("transformers")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _collect_when_done():
    """Tests that expect an exception (here and in the modules before)
    leave tracebacks behind that keep landers, pinned rings and streams
    alive until a cycle collection.  Later modules count what the native
    resource caches hold, so give those resources back before handing
    over rather than in the middle of their measurements."""
    yield
    gc.collect()


def test_pull_pretrained_dequantize_gpu(tmp_path):
    from demodel_amd.engine.loader import pull_pretrained
    from demodel_amd.gpu import have_gpu

    assert have_gpu()
    files, quantised, plain = fx.build_tiny_llama_fp8_repo(tmp_path / "repo")
    stack = Stack(tmp_path)
    try:
        stack.origin.add_hf_repo("tiny/llama-fp8", files)
        model, res = pull_pretrained(
            "tiny/llama-fp8", endpoint=stack.origin_base, workers=2,
            dequantize=True)
    finally:
        stack.close()
    assert all(f.blob.device != "cpu" for f in res.files)
    assert type(model) is transformers.LlamaForCausalLM
    assert all(p.is_cuda for p in model.parameters())
    fx.assert_tiny_llama_loaded(model, quantised, plain)
    x = torch.randint(0, 256, (1, 8), device="cuda")
    with torch.no_grad():
        logits = model(x).logits
    assert logits.shape == (1, 8, 256)
    assert torch.isfinite(logits.float()).all()


def test_library_written_file_fp8_target_and_shape_error(tmp_path):
    """On a file the safetensors library wrote: an FP8 parameter takes
    the codes as they are, and a wider parameter of the wrong shape is
    a shape error before anything else."""
    from demodel_amd.engine.loader import load_into
    from demodel_amd.engine import pull as pull_mod
    from demodel_amd.engine.formats import safetensors as st

    files, quantised, _ = fx.build_tiny_llama_fp8_repo(tmp_path / "repo")
    stack = Stack(tmp_path)
    try:
        stack.origin.add_hf_repo("tiny/llama-fp8", files)
        res = pull_mod.pull_hf("tiny/llama-fp8",
                               endpoint=stack.origin_base, workers=2)
    finally:
        stack.close()
    f = next(f for f in res.files if f.name == "model.safetensors")
    hdr = st.parse_header(f.blob.head)
    name = next(iter(quantised))
    codes, _ = quantised[name]
    # the codes alone, into an FP8 parameter: a plain scatter
    raw = torch.zeros(codes.shape, dtype=torch.float8_e4m3fn, device="cuda")
    load_into(f.blob, hdr, {name: raw}, strict=False)
    assert torch.equal(raw.view(torch.uint8).cpu(), codes)
    # a bf16 parameter of the wrong shape is still a shape error
    with pytest.raises(ValueError, match="shape"):
        load_into(f.blob, hdr,
                  {name: torch.zeros(3, 3, dtype=torch.bfloat16,
                                     device="cuda")}, strict=False)

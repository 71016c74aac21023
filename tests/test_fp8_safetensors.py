"""FP8 block-scaled safetensors without a GPU: scale discovery
(fp8_scale_map), load_into on a host-landed blob, and pull_pretrained
with dequantize=True end to end.  The reference is computed here with
torch on the CPU (fp8_fixtures.reference), never through the loader."""

import pytest
import torch

import fp8_fixtures as fx
from helpers import Stack, host_landers

from demodel_amd.engine.formats import safetensors as st


def _header(spec):
    head, _ = st.build_header(spec)
    return st.parse_header(head)


def _w(shape):
    n = 1
    for d in shape:
        n *= d
    return ("F8_E4M3", shape, n)


def _s(shape, tag="F32"):
    n = {"F32": 4, "BF16": 2, "F16": 2, "I32": 4, "F64": 8}[tag]
    for d in shape:
        n *= d
    return (tag, shape, n)


# ---------------------------------------------------------------- names

def test_scale_map_name_rules():
    hdr = _header({
        "x.weight": _w((256, 256)),
        "x.weight_scale_inv": _s((2, 2)),
        "x.weight_scale": _s((1,)),            # _scale_inv wins
        "y.weight": _w((4, 8)),
        "y.weight_scale": _s((4, 1), "BF16"),
        "z.weight": _w((4, 8)),                # FP8 without a scale
        "p.weight": ("BF16", (4, 8), 64),      # not FP8: its scale is
        "p.weight_scale": _s((1,)),            # nobody's business
        "q.weight": ("F8_E5M2", (4, 8), 32),   # E5M2 is out of scope
        "q.weight_scale": _s((1,)),
    })
    m = st.fp8_scale_map(hdr)
    assert sorted(m) == ["x.weight", "y.weight"]
    assert m["x.weight"].info.name == "x.weight_scale_inv"
    assert m["x.weight"].block == (128, 128)
    assert m["y.weight"].info.name == "y.weight_scale"
    assert m["y.weight"].info.st_dtype == "BF16"
    assert m["y.weight"].block == (1, 8)
    assert isinstance(m["y.weight"], st.Fp8Scale)


def test_scale_map_empty_without_fp8():
    hdr = _header({"w": ("BF16", (4, 4), 32), "w_scale": _s((1,))})
    assert st.fp8_scale_map(hdr) == {}


# --------------------------------------------------- block resolution

@pytest.mark.parametrize("wshape,sshape,block_size,want", [
    ((200, 300), (), None, (200, 300)),           # per tensor, 0-d
    ((200, 300), (1,), None, (200, 300)),         # per tensor, (1,)
    ((200, 300), (200,), None, (1, 300)),         # per row, 1-d
    ((200, 300), (200, 1), None, (1, 300)),       # per row, column vector
    ((200, 300), (2, 3), None, (128, 128)),       # default 128x128, ceil
    ((129, 130), (2, 2), None, (128, 128)),
    ((200, 300), (4, 5), (64, 64), (64, 64)),     # explicit block, ceil
    ((200, 300), (4, 5), [64, 64], (64, 64)),     # ... as config.json has it
    ((200, 300), (2, 3), (64, 64), (128, 128)),   # explicit misses, 128 fits
    ((200, 300), (4, 3), None, (50, 100)),        # exact division
    ((200, 300), (1, 300), None, (200, 1)),       # exact: per column
    ((200, 300), (1, 1), None, (200, 300)),       # exact: one block
])
def test_scale_map_block_resolution(wshape, sshape, block_size, want):
    hdr = _header({"w": _w(wshape), "w_scale_inv": _s(sshape)})
    m = st.fp8_scale_map(hdr, block_size=block_size)
    assert m["w"].block == want
    assert m["w"].info.shape == sshape


@pytest.mark.parametrize("wshape,sshape,block_size", [
    ((200, 300), (3, 7), None),          # neither ceil nor exact division
    ((200, 300), (3, 7), (64, 64)),
    ((200, 300), (7,), None),            # 1-d but not one per row
    ((200, 300), (2, 3, 1), None),       # 3-d scale
    ((200, 300), (0, 3), None),
])
def test_scale_map_unresolvable_names_the_tensor(wshape, sshape,
                                                 block_size):
    hdr = _header({"blk.w": _w(wshape), "blk.w_scale_inv": _s(sshape)})
    with pytest.raises(ValueError, match="blk.w"):
        st.fp8_scale_map(hdr, block_size=block_size)


@pytest.mark.parametrize("wshape", [(300,), (2, 10, 30), ()])
def test_scale_map_rank_error(wshape):
    hdr = _header({"w": _w(wshape), "w_scale": _s((1,))})
    with pytest.raises(ValueError, match="2-D"):
        st.fp8_scale_map(hdr)


@pytest.mark.parametrize("tag", ["I32", "F64", "F8_E4M3"])
def test_scale_map_dtype_error(tag):
    sc = _w((1,)) if tag == "F8_E4M3" else _s((1,), tag)
    hdr = _header({"w": _w((4, 4)), "w_scale": sc})
    with pytest.raises(ValueError, match="dtype"):
        st.fp8_scale_map(hdr)


def test_scale_map_bad_block_size():
    hdr = _header({"w": _w((4, 4)), "w_scale": _s((1,))})
    with pytest.raises(ValueError):
        st.fp8_scale_map(hdr, block_size=(128,))


# ------------------------------------------------ quantize_fp8_blocks

def test_quantize_fp8_blocks_roundtrip():
    from demodel_amd.testing.synth import quantize_fp8_blocks

    torch.manual_seed(1)
    w = torch.randn(200, 300)
    w[:128, :128] = 0                      # an all-zero block: scale floor
    codes, scales = quantize_fp8_blocks(w, (128, 128))
    assert codes.dtype == torch.uint8 and codes.shape == (200, 300)
    assert scales.dtype == torch.float32 and scales.shape == (2, 3)
    assert (scales > 0).all()
    assert not ((codes & 0x7F) == 0x7F).any()          # no NaN codes
    back = fx.reference(codes, scales, (128, 128), torch.float32)
    assert torch.equal(back[:128, :128], torch.zeros(128, 128))
    # e4m3 keeps 3 mantissa bits: relative error <= 2**-4 per element,
    # plus half a subnormal step (2**-10) of the block's scale
    full = fx.expand(scales, (200, 300), (128, 128))
    assert ((back - w).abs() <= w.abs() * 2.0 ** -4 + full * 2.0 ** -10
            ).all()
    # the block maximum maps to +-448 exactly
    assert int(((codes & 0x7F) == 0x7E).sum()) >= 5


# --------------------------------------------- load_into, host landing

@pytest.fixture(scope="module")
def cpu_pull(tmp_path_factory):
    from demodel_amd.engine import pull as pull_mod

    tmp = tmp_path_factory.mktemp("fp8cpu")
    stack = Stack(tmp)
    try:
        p = tmp / "m.safetensors"
        t = fx.build_fp8_checkpoint(str(p))
        stack.origin.add_hf_repo("o/fp8", {"m.safetensors": str(p)})
        res = pull_mod.pull_hf("o/fp8", endpoint=stack.origin_base,
                               workers=1, landers=host_landers())
        blob = res.files[0].blob
        assert blob.device == "cpu"
        yield blob, st.parse_header(blob.head), t
    finally:
        stack.close()


def test_load_into_cpu_landed_blob(cpu_pull):
    from demodel_amd.engine.loader import load_into

    blob, hdr, t = cpu_pull
    targets = {k: torch.zeros(tuple(t[k].shape), dtype=torch.bfloat16)
               for k in ("a.weight", "b.weight", "n.weight", "e.weight")}
    targets["pad"] = torch.zeros(3, dtype=torch.uint8)
    loaded = load_into(blob, hdr, targets, strict=True)
    assert sorted(loaded) == sorted(targets)
    want = fx.expected_bf16(t)
    fx.assert_dequant_equal(targets["a.weight"], t["a.weight"],
                            want["a.weight"])
    fx.assert_dequant_equal(targets["b.weight"], t["b.weight"],
                            want["b.weight"])
    assert torch.equal(targets["n.weight"], want["n.weight"])
    assert torch.equal(targets["e.weight"], want["e.weight"])
    assert targets["pad"].tolist() == [1, 2, 3]


def test_load_into_cpu_f32_target_and_fp8_target(cpu_pull):
    from demodel_amd.engine.loader import load_into

    blob, hdr, t = cpu_pull
    a32 = torch.zeros(200, 300, dtype=torch.float32)
    b8 = torch.zeros(64, 48, dtype=torch.float8_e4m3fn)
    load_into(blob, hdr, {"a.weight": a32, "b.weight": b8}, strict=False)
    fx.assert_dequant_equal(
        a32, t["a.weight"],
        fx.reference(t["a.weight"], t["a.weight_scale_inv"], (128, 128),
                     torch.float32))
    # FP8 into FP8 stays a plain copy of the codes
    assert torch.equal(b8.view(torch.uint8), t["b.weight"])


def test_load_into_cpu_strict_still_reports_unconsumed(cpu_pull):
    from demodel_amd.engine.loader import load_into

    blob, hdr, t = cpu_pull
    # b.weight not loaded, so its scale is a tensor the model lacks
    with pytest.raises(KeyError, match="b.weight"):
        load_into(blob, hdr,
                  {"a.weight": torch.zeros(200, 300,
                                           dtype=torch.bfloat16)},
                  strict=True)


def _cpu_blob(tmp_path, spec, payload):
    """A host-landed blob of a hand-built file, pulled like any other."""
    from demodel_amd.engine import pull as pull_mod

    head, _ = st.build_header(spec)
    stack = Stack(tmp_path)
    try:
        p = tmp_path / "m.safetensors"
        p.write_bytes(head + payload)
        stack.origin.add_hf_repo("o/x", {"m.safetensors": str(p)})
        res = pull_mod.pull_hf("o/x", endpoint=stack.origin_base,
                               workers=1, landers=host_landers())
    finally:
        stack.close()
    blob = res.files[0].blob
    return blob, st.parse_header(blob.head)


def test_load_into_cpu_errors(tmp_path):
    from demodel_amd.engine.loader import load_into

    dst = torch.zeros(4, 8, dtype=torch.bfloat16)
    # no scale tensor at all
    blob, hdr = _cpu_blob(tmp_path / "a", {"w": _w((4, 8))}, bytes(32))
    with pytest.raises(ValueError, match="no scale tensor"):
        load_into(blob, hdr, {"w": dst}, strict=False)
    # a scale shape that fits no block
    blob, hdr = _cpu_blob(
        tmp_path / "b", {"w": _w((4, 8)), "w_scale_inv": _s((3, 3))},
        bytes(32 + 36))
    with pytest.raises(ValueError, match="fits no block"):
        load_into(blob, hdr, {"w": dst}, strict=False)
    # a scale whose extent runs past the blob
    blob, hdr = _cpu_blob(
        tmp_path / "c", {"w": _w((4, 8)), "w_scale_inv": _s((4, 1))},
        bytes(32 + 4))
    with pytest.raises(ValueError, match="does not fit the blob"):
        load_into(blob, hdr, {"w": dst}, strict=False)


# ------------------------------------------------------- end to end

def test_pull_pretrained_dequantize_cpu(tmp_path):
    transformers = pytest.importorskip("transformers")

    from demodel_amd.engine.loader import pull_pretrained

    files, quantised, plain = fx.build_tiny_llama_fp8_repo(tmp_path / "repo")
    assert len(quantised) == 14
    hdr = st.parse_header(open(files["model.safetensors"], "rb").read())
    assert {i.st_dtype for i in hdr.tensors} == {"F8_E4M3", "F32", "BF16"}

    stack = Stack(tmp_path)
    try:
        stack.origin.add_hf_repo("tiny/llama-fp8", files)
        model, res = pull_pretrained(
            "tiny/llama-fp8", endpoint=stack.origin_base, workers=2,
            device="cpu", landers=host_landers(), dequantize=True)
    finally:
        stack.close()
    assert type(model) is transformers.LlamaForCausalLM
    fx.assert_tiny_llama_loaded(model, quantised, plain)
    x = torch.randint(0, 256, (1, 8))
    with torch.no_grad():
        logits = model(x).logits
    assert logits.shape == (1, 8, 256)
    assert torch.isfinite(logits.float()).all()

"""Shared pieces of the FP8 block-scaled safetensors tests: the CPU
reference, the bit-exact comparison and the test checkpoint.

The reference is one f32 multiply and one round-to-nearest-even, the same
two operations the kernel does, so results compare bit for bit.  Scales
are drawn from [2**-10, 16): the smallest nonzero e4m3fn magnitude is
2**-9, so no product is an f32 subnormal and flush modes cannot enter;
the largest product, 448 * 16, is far from any overflow.  The only NaNs
are then the two NaN codes, 0x7F and 0xFF.
"""

import json

import numpy as np
import torch

SCALE_DTYPES = {"F32": torch.float32, "BF16": torch.bfloat16,
                "F16": torch.float16}
SCALE_CODE = {"F32": 0, "BF16": 1, "F16": 2}
DST_CODE = {torch.bfloat16: 0, torch.float32: 1}


def draw_codes(rng, shape) -> torch.Tensor:
    return torch.from_numpy(
        rng.integers(0, 256, size=shape, dtype=np.uint8))


def draw_scales(rng, shape, tag="F32") -> torch.Tensor:
    s = rng.uniform(2.0 ** -10, 16.0, size=shape).astype(np.float32)
    return torch.from_numpy(s).to(SCALE_DTYPES[tag])


def expand(scale: torch.Tensor, shape, block) -> torch.Tensor:
    R, C = shape
    br, bc = block
    grid = scale.reshape(-(-R // br), -(-C // bc))
    return grid.repeat_interleave(br, 0)[:R].repeat_interleave(bc, 1)[:, :C]


def reference(codes: torch.Tensor, scale: torch.Tensor, block,
              dst_dtype) -> torch.Tensor:
    expanded_scale = expand(scale, tuple(codes.shape), block)
    return (codes.view(torch.float8_e4m3fn).float()
            * expanded_scale.float()).to(dst_dtype)


def assert_dequant_equal(got: torch.Tensor, codes: torch.Tensor,
                         want: torch.Tensor) -> None:
    """Raw bits equal wherever the input code is a number, NaN wherever
    it is one of the two NaN codes.  The mask comes from the input."""
    assert got.dtype == want.dtype and got.shape == want.shape
    nan_in = (codes & 0x7F) == 0x7F
    bits = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    assert not torch.isnan(want[~nan_in]).any()
    assert torch.equal(got.view(bits)[~nan_in], want.view(bits)[~nan_in])
    assert torch.isnan(got[nan_in]).all()


def build_fp8_checkpoint(path, seed=0) -> dict:
    """Write the test checkpoint and return its tensors.  `pad` makes the
    FP8 payload and the f32 scale both start at odd offsets."""
    from demodel_amd.engine.formats import safetensors as st

    rng = np.random.default_rng(seed)
    t = {
        "pad": torch.tensor([1, 2, 3], dtype=torch.uint8),
        "a.weight": draw_codes(rng, (200, 300)),
        "a.weight_scale_inv": draw_scales(rng, (2, 3), "F32"),
        "b.weight": draw_codes(rng, (64, 48)),
        "b.weight_scale": draw_scales(rng, (64, 1), "BF16"),
        "n.weight": torch.from_numpy(
            rng.standard_normal(32).astype(np.float32)).to(torch.bfloat16),
        "e.weight": torch.from_numpy(
            rng.standard_normal((8, 8)).astype(np.float32)),
    }
    tags = {"pad": "U8", "a.weight": "F8_E4M3",
            "a.weight_scale_inv": "F32", "b.weight": "F8_E4M3",
            "b.weight_scale": "BF16", "n.weight": "BF16",
            "e.weight": "F32"}
    raw = {k: v.contiguous().view(torch.uint8).numpy().tobytes()
           for k, v in t.items()}
    spec = {k: (tags[k], tuple(t[k].shape), len(raw[k])) for k in t}
    head, _ = st.build_header(spec)
    hdr = st.parse_header(head)
    by = {i.name: i for i in hdr.tensors}
    assert (hdr.data_offset + by["a.weight"].begin) % 2 == 1
    assert (hdr.data_offset + by["a.weight_scale_inv"].begin) % 2 == 1
    with open(path, "wb") as f:
        f.write(head + b"".join(raw[k] for k in t))
    t["_spec"] = spec
    t["_raw"] = raw
    return t


def expected_bf16(t: dict) -> dict:
    """What load_into must leave in bf16 targets for the four weights."""
    return {
        "a.weight": reference(t["a.weight"], t["a.weight_scale_inv"],
                              (128, 128), torch.bfloat16),
        "b.weight": reference(t["b.weight"], t["b.weight_scale"],
                              (1, 48), torch.bfloat16),
        "n.weight": t["n.weight"],
        "e.weight": t["e.weight"].to(torch.bfloat16),
    }


def build_tiny_llama_fp8_repo(d):
    """A tiny random Llama as an FP8 block-scaled checkpoint in directory
    `d`: every *_proj.weight quantised per 128x128 block (F8_E4M3 +
    `_scale_inv` F32), the rest bf16, written with the safetensors
    library, plus a config.json that carries the quantization_config.
    Returns ({rfilename: path}, {name: (codes, scales)}, {name: bf16})."""
    import transformers
    from safetensors.torch import save_file

    from demodel_amd.testing.synth import quantize_fp8_blocks

    cfg = transformers.LlamaConfig(
        hidden_size=160, intermediate_size=288, num_hidden_layers=2,
        num_attention_heads=4, num_key_value_heads=2, vocab_size=256,
        max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    src = transformers.LlamaForCausalLM(cfg)
    out, quantised, plain = {}, {}, {}
    for name, p in src.state_dict().items():
        if name.endswith("_proj.weight"):
            codes, scales = quantize_fp8_blocks(p.float(), (128, 128))
            out[name] = codes.view(torch.float8_e4m3fn)
            out[name + "_scale_inv"] = scales
            quantised[name] = (codes, scales)
        else:
            out[name] = p.detach().to(torch.bfloat16).contiguous()
            plain[name] = out[name]
    d.mkdir()
    save_file(out, str(d / "model.safetensors"))
    cfg_dict = cfg.to_dict()
    cfg_dict["torch_dtype"] = "bfloat16"
    cfg_dict.pop("dtype", None)
    cfg_dict["quantization_config"] = {"quant_method": "fp8",
                                       "weight_block_size": [128, 128]}
    (d / "config.json").write_text(json.dumps(cfg_dict))
    files = {"model.safetensors": str(d / "model.safetensors"),
             "config.json": str(d / "config.json")}
    return files, quantised, plain


def assert_tiny_llama_loaded(model, quantised, plain) -> None:
    """Quantised parameters equal the reference dequant bit for bit, the
    others the checkpoint's bf16 values."""
    params = dict(model.named_parameters())
    for name, (codes, scales) in quantised.items():
        assert params[name].dtype == torch.bfloat16
        assert_dequant_equal(
            params[name].detach().cpu(), codes,
            reference(codes, scales, (128, 128), torch.bfloat16))
    for name, want in plain.items():
        assert torch.equal(params[name].detach().cpu(), want)

#!/usr/bin/env python3
"""Time the FP8 block-scaled dequant kernel against its two yardsticks.

For one 8192x8192 tensor and for a set of 64 tensors of 4096x4096
(block 128x128, f32 scales, bf16 out) it times

* kernel     _hip.fp8_block_dequant, one launch per tensor;
* cast       _hip.cast_f32_to_bf16 on the same element count;
* composite  what a user writes today with torch on the GPU:
             w.view(float8_e4m3fn).float() * scale.repeat_interleave(..)
             then .to(bfloat16).

Device events around `inner` back-to-back passes per sample, warm-up
first, the three variants alternating within each round, median over
the rounds.  Bytes are the ones the algorithm needs (kernel: 1 B in,
2 B out, plus the scales; cast: 4 B in, 2 B out) and the rate is those
bytes over the median time.  The kernel's output is compared bit for
bit with the composite's at the sizes timed before anything is timed.

Needs a GPU; writes a markdown report (default profiles/fp8_dequant.md).
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOCK = 128


def composite(torch, codes, scale):
    R, C = codes.shape
    w = codes.view(torch.float8_e4m3fn).float() * \
        scale.repeat_interleave(BLOCK, 0)[:R].repeat_interleave(
            BLOCK, 1)[:, :C]
    return w.to(torch.bfloat16)


def time_variants(torch, variants: dict, warmup: int, rounds: int,
                  inner: int) -> dict:
    """variants: name -> callable doing one pass.  Returns name ->
    list of per-pass milliseconds, one per round."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / inner)
    return out


def run_shape(torch, h, label, shape, n_tensors, args):
    from demodel_amd.testing.synth import quantize_fp8_blocks

    R, C = shape
    n = R * C
    torch.manual_seed(0)
    codes_cpu, scale_cpu = quantize_fp8_blocks(torch.randn(R, C),
                                               (BLOCK, BLOCK))
    # every tensor of the set has storage of its own, so the set's
    # working set is n_tensors times one tensor's
    codes = [codes_cpu.cuda() for _ in range(n_tensors)]
    scales = [scale_cpu.cuda() for _ in range(n_tensors)]
    outs = [torch.empty(R, C, dtype=torch.bfloat16, device="cuda")
            for _ in range(n_tensors)]
    f32s = [torch.randn(R, C, device="cuda") for _ in range(n_tensors)]
    casts = [torch.empty(R, C, dtype=torch.bfloat16, device="cuda")
             for _ in range(n_tensors)]
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        for c, s, o in zip(codes, scales, outs):
            h.fp8_block_dequant(c.data_ptr(), s.data_ptr(), 0,
                                o.data_ptr(), 0, R, C, BLOCK, BLOCK,
                                stream)

    def cast():
        for f, o in zip(f32s, casts):
            h.cast_f32_to_bf16(f.data_ptr(), o.data_ptr(), n, stream)

    keep = [None]

    def comp():
        for c, s in zip(codes, scales):
            keep[0] = composite(torch, c, s)

    # same results first (bit for bit), at the size that is timed
    kernel()
    torch.cuda.synchronize()
    want = composite(torch, codes[-1], scales[-1])
    if not torch.equal(outs[-1].view(torch.int16), want.view(torch.int16)):
        raise SystemExit(f"{label}: kernel and composite disagree")
    del want

    ms = time_variants(torch, {"kernel": kernel, "cast": cast,
                               "composite": comp},
                       args.warmup, args.rounds, args.inner)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lo = {k: min(v) for k, v in ms.items()}
    hi = {k: max(v) for k, v in ms.items()}
    total = n * n_tensors
    bytes_needed = {
        "kernel": total * 3 + scale_cpu.numel() * 4 * n_tensors,
        "cast": total * 6,
    }
    rows = []
    for k in ("kernel", "cast", "composite"):
        rate = (f"{bytes_needed[k] / (med[k] * 1e-3) / 1e9:.0f}"
                if k in bytes_needed else "-")
        rows.append(f"| {label} | {k} | {med[k]:.4f} | {lo[k]:.4f} | "
                    f"{hi[k]:.4f} | {rate} |")
    ratio = med["composite"] / med["kernel"]
    return rows, (label, ratio, med)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "fp8_dequant.md"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=25,
                    help="timed samples per variant (median reported)")
    ap.add_argument("--inner", type=int, default=8,
                    help="back-to-back passes per timed sample")
    ap.add_argument("--small", action="store_true",
                    help="tiny shapes: checks the script, not the kernel")
    args = ap.parse_args()
    if args.rounds < 20 and not args.small:
        ap.error("--rounds must be at least 20")

    import torch

    from demodel_amd.gpu import have_gpu, hip

    if not have_gpu():
        print("fp8_dequant_probe: no GPU; nothing is measured without one",
              file=sys.stderr)
        return 2
    h = hip()
    shapes = ([("1 x 256x384", (256, 384), 1), ("4 x 128x256", (128, 256), 4)]
              if args.small else
              [("1 x 8192x8192", (8192, 8192), 1),
               ("64 x 4096x4096", (4096, 4096), 64)])
    table, ratios = [], []
    for label, shape, n_tensors in shapes:
        rows, r = run_shape(torch, h, label, shape, n_tensors, args)
        table += rows
        ratios.append(r)
        torch.cuda.empty_cache()

    props = torch.cuda.get_device_properties(0)
    dev = f"{props.name} ({props.gcnArchName.split(':')[0]})"
    lines = [
        "# FP8 block-scaled dequant: kernel vs cast vs torch composite",
        "",
        f"Measured by `scripts/fp8_dequant_probe.py` on {dev}: F8_E4M3 "
        f"codes with f32 scales per {BLOCK}x{BLOCK} block to bf16.  "
        f"Device events around {args.inner} back-to-back passes per "
        f"sample, {args.warmup} warm-up passes, the three variants "
        f"alternating within each of {args.rounds} rounds; median, "
        "fastest and slowest sample in ms per pass (a pass is every "
        "tensor of the set once).  GB/s is the bytes the algorithm needs "
        "(kernel: 1 B in + 2 B out per element plus the scales; cast: "
        "4 B in + 2 B out) over the median.  The kernel's output equals "
        "the composite's bit for bit at both sizes.",
        "",
        "| set | variant | median ms | min ms | max ms | GB/s in+out |",
        "|---|---|---|---|---|---|",
    ] + table + [""]
    for label, ratio, med in ratios:
        lines.append(
            f"- {label}: composite / kernel = {ratio:.1f}x in time "
            f"(cast / kernel = {med['cast'] / med['kernel']:.2f}x).")
    lines += [
        "",
        "The composite moves at least 5x the kernel's bytes (f32 "
        "temporaries of the codes, of the expanded scales and of the "
        "product, each written and read again), so a ratio under 5x "
        "would mean a badly shaped kernel.",
    ]
    lines += [] if args.small else [
        "",
        "The single 8192x8192 tensor (64 MiB in, 128 MiB out) is re-read "
        "from buffers that were just touched, so the last-level cache "
        "helps every variant there; the 64-tensor set (1 GiB in, 2 GiB "
        "out) does not fit in it and is the figure to hold against HBM "
        "bandwidth.",
        "",
    ]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

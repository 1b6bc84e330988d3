"""A/B of the three forms of the uint8 stem at the benchmark's shapes: float32 matrix cores (`hip_stem_conv_pool`), half matrix
cores (`hip_stem_conv_pool_h`, bfloat16) and bf16 matrix cores with exactly split float32 weights (`hip_stem_conv_pool_split`).

    python scripts/perf_stem.py [--n 4096] [--reps 20] [--form f32|bf16|split|all] [--once]

Prints the median / minimum launch time per form and patch size (hip events around single launches, the forms interleaved), the
effective bandwidth, and the error of the float32 and split forms against a float64 convolution on the inputs of the stem tests
(2 x 256^2 and 3 x 224^2).  `--once` launches the chosen form once at 1024 x 256^2: with a timing build of the library
(TIA_LIB_PATH, built with build.build(defines=("TIA_STEM_TIMING=1",), out=...)) the kernel prints its per-phase cycles."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import torch.nn.functional as F  # noqa: N812

from tiatoolbox_amd.models.architecture.fused import (hip_stem_conv_pool, hip_stem_conv_pool_h, hip_stem_conv_pool_split,
                                                      pack_stem_weights, pack_stem_weights_h, pack_stem_weights_split)


def forms(w, b, which):
    out = {}
    if which in ("f32", "all"):
        wp = pack_stem_weights(w)
        out["f32"] = lambda x: hip_stem_conv_pool(x, wp, b)
    if which in ("bf16", "all"):
        wh = pack_stem_weights_h(w, torch.bfloat16)
        out["bf16"] = lambda x: hip_stem_conv_pool_h(x, wh, b, dtype=torch.bfloat16)
    if which in ("split", "all"):
        ws = pack_stem_weights_split(w)
        out["split"] = lambda x: hip_stem_conv_pool_split(x, ws, b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--form", default="all", choices=["f32", "bf16", "split", "all"])
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(64, 3, 7, 7, generator=g) * 0.05).cuda()
    b = (torch.randn(64, generator=g) * 0.1).cuda()
    fs = forms(w, b, args.form)
    if args.once:
        x = torch.randint(0, 256, (1024, 256, 256, 3), dtype=torch.uint8, device="cuda")
        for name, f in fs.items():
            print(f"--- {name}", flush=True)
            f(x)
            torch.cuda.synchronize()
        return
    for side in (256, 224):
        x = torch.randint(0, 256, (args.n, side, side, 3), dtype=torch.uint8, device="cuda")
        times = {name: [] for name in fs}
        for name, f in fs.items():  # warm-up: attributes, clocks
            for _ in range(3):
                f(x)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, f in fs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                y = f(x)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        for name, t in times.items():
            med = statistics.median(t)
            nbytes = x.numel() + (args.n * 64 * (side // 4) ** 2) * (2 if name == "bf16" else 4)
            print(f"stem {name:5s} {args.n} x {side}^2: median {med:7.3f} ms  min {min(t):7.3f}  max {max(t):7.3f}  "
                  f"({nbytes / med / 1e6:6.0f} GB/s)", flush=True)
        del x, y
    # error against float64 (same inputs as tests/test_stem_gpu.py, tier (a) of tests/test_stem_split_gpu.py)
    for n, side in ((2, 256), (3, 224)):
        gw = torch.Generator().manual_seed(side * 1000 + side)
        wt = torch.randn((64, 3, 7, 7), generator=gw) * 0.05
        bt = torch.randn(64, generator=gw) * 0.1
        gx = torch.Generator().manual_seed(n + side + side)
        x = torch.randint(0, 256, (n, side, side, 3), generator=gx, dtype=torch.uint8)
        ref = F.max_pool2d(F.relu(F.conv2d(x.double().div(255).permute(0, 3, 1, 2), wt.double(), bt.double(), 2, 3)), 3, 2, 1)
        for name, f in forms(wt.cuda(), bt.cuda(), "all").items():
            if name == "bf16":
                continue
            err = (f(x.cuda()).double().cpu() - ref).abs()
            print(f"error vs float64, {n} x {side}^2, {name:5s}: max {err.max().item():.3e}  rms {err.pow(2).mean().sqrt().item():.3e}")


if __name__ == "__main__":
    main()

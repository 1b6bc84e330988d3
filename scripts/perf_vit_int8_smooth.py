"""``FusedViT`` with ``linear_dtype="int8", smoothing=scales`` beside the unsmoothed INT8 graph and the bfloat16 graph, in
ONE session, alternating:

1. whole forward of a seeded ``--model`` on ``--batch`` x ``--side``^2 patches: one HIP event pair per call, ``--warmup`` calls of each
   graph first, then ``--reps`` rounds with the three graphs in turn inside every round; the figure is the median, the spread the
   inter-quartile range of the rounds (minimum and maximum are kept as well).  The comparison is smoothed against unsmoothed INT8 of the
   same session: the change is one more float32 load and multiplication per ``fc2`` input element, so parity is expected; a
   difference counts when the medians differ by more than the wider of the two inter-quartile ranges;
2. ``fc2``'s producer alone at block 0's shape and this batch's rows, smoothed against unsmoothed, timed the same way: where a
   difference of the forwards would have to come from.

The scales are calibrated on ``--calibration`` seeded patches (``calibrate_int8_smoothing``, alpha ``--alpha``); its one-off time is
printed.  Seeded random weights: no pretrained checkpoint is read, and what smoothing does to the accuracy of a real checkpoint is
not measured here.

``--trace-only smoothed|int8``: calibrate, warm up, run that graph ``--reps`` times and exit -- the program to put behind
``rocprofv3 --kernel-trace --stats -- python scripts/perf_vit_int8_smooth.py --trace-only smoothed`` (a run of its own, no counters):
where a difference between the two forwards sits, kernel by kernel.

usage: perf_vit_int8_smooth.py [--model UNI] [--batch 256] [--side 224] [--depth N] [--warmup 3] [--reps 20] [--calibration 8]
                               [--alpha 0.5] [--trace-only smoothed|int8] [--out FILE.json]"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from perf_vit import build, forward_flops  # noqa: E402
from perf_vit_fp8 import BF16, graph_of  # noqa: E402
from perf_vit_int8 import INT8, timed  # noqa: E402


def smoothed_graph_of(vit, scales):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(vit)
    fused.prepare(BF16, linear_dtype=INT8, smoothing=scales)
    return fused.to(BF16).eval()


def _summary(t: dict) -> dict:
    q = statistics.quantiles(t["times"], n=4)
    return {"ms": t["ms"], "iqr_ms": q[2] - q[0], "min_ms": t["min_ms"], "max_ms": t["max_ms"], "times": t["times"]}


def _compare(smooth: dict, plain: dict) -> dict:
    spread = max(smooth["iqr_ms"], plain["iqr_ms"])
    return {"smoothed_minus_unsmoothed_ms": smooth["ms"] - plain["ms"], "ratio": smooth["ms"] / plain["ms"], "spread_ms": spread,
            "slower_beyond_spread": bool(smooth["ms"] - plain["ms"] > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNI")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--depth", type=int, default=0, help="override the number of blocks (0: the model's own)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calibration", type=int, default=8, help="seeded patches the scales are calibrated on")
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--trace-only", default=None, choices=["smoothed", "int8"])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit_int8_smooth.py measures on a GPU; none is visible.")
    from tiatoolbox_amd.models.architecture import vit_fused as vf

    cfg, vit = build(args)
    flops = forward_flops(cfg, cfg["depth"], args.batch, args.side)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g).to(BF16).contiguous(memory_format=torch.channels_last)
    cal = torch.randn((args.calibration, 3, args.side, args.side), device="cuda", generator=g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scales = vf.calibrate_int8_smoothing(vit, [cal], alpha=args.alpha)
    torch.cuda.synchronize()
    calibration_s = time.perf_counter() - t0
    moved = sum(int((s != 1.0).sum()) for s in scales.values())
    print(f"calibration of {len(scales)} layers on {args.calibration} patches: {calibration_s:.2f} s (once per model); "
          f"{moved} of {sum(s.numel() for s in scales.values())} scales differ from 1", flush=True)
    if args.trace_only:
        graph = smoothed_graph_of(vit, scales) if args.trace_only == "smoothed" else graph_of(vit, INT8)
        with torch.inference_mode():
            graph(x)
            torch.cuda.synchronize()
            for _ in range(args.reps):
                graph(x)
            torch.cuda.synchronize()
        return
    graphs = {"int8 smoothed": smoothed_graph_of(copy.deepcopy(vit), scales), "int8": graph_of(copy.deepcopy(vit), INT8),
              "bf16": graph_of(copy.deepcopy(vit), None)}
    del vit
    torch.cuda.empty_cache()
    res = {name: _summary(t) for name, t in timed({name: (lambda gr=gr: gr(x)) for name, gr in graphs.items()}, args.warmup, args.reps).items()}
    print(f"{args.model} depth {cfg['depth']}  {args.batch} x {args.side}^2  ({flops['tokens']} tokens)  {flops['total'] / 1e12:.2f} TFLOP per forward  "
          f"on {torch.cuda.get_device_name(0)}")
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        print(f"FusedViT {name:14s} {r['ms']:9.2f} ms  iqr {r['iqr_ms']:.2f}  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  {r['patches_per_s']:8.1f} patches/s",
              flush=True)
    forward = _compare(res["int8 smoothed"], res["int8"])
    print(f"smoothed against unsmoothed int8: {forward['smoothed_minus_unsmoothed_ms']:+.2f} ms ({forward['ratio']:.4f}x) beside a spread of "
          f"{forward['spread_ms']:.2f} ms -> slower beyond the spread: {forward['slower_beyond_spread']};  against bf16: "
          f"{res['bf16']['ms'] / res['int8 smoothed']['ms']:.3f}x", flush=True)
    report = {"model": args.model, "config": cfg, "batch": args.batch, "side": args.side, "warmup": args.warmup, "reps": args.reps,
              "alpha": args.alpha, "calibration_patches": args.calibration, "calibration_s": calibration_s, "forward": res,
              "forward_comparison": forward}
    fc2 = graphs["int8 smoothed"].layers[0]["fc2"]
    if fc2.inv_smooth is not None:
        swiglu, n, s = graphs["int8"].swiglu, args.batch, flops["tokens"]
        src = torch.randn((n, s, fc2.cin * (2 if swiglu else 1)), device="cuda", generator=g).to(BF16)
        t = timed({"producer smoothed": lambda: vf.hip_act_rows_qi8_smooth(src, fc2.inv_smooth, swiglu=swiglu),
                   "producer": lambda: vf.hip_act_rows_qi8(src, swiglu=swiglu)}, args.warmup, args.reps)
        prod = {name: _summary(v) for name, v in t.items()}
        cmp_ = _compare(prod["producer smoothed"], prod["producer"])
        print(f"fc2's producer at [{n * s}, {fc2.cin}]: smoothed {prod['producer smoothed']['ms']:.3f} ms, unsmoothed {prod['producer']['ms']:.3f} ms "
              f"({cmp_['smoothed_minus_unsmoothed_ms']:+.3f} ms per layer, x {cfg['depth']} layers; spread {cmp_['spread_ms']:.3f} ms) -> slower "
              f"beyond the spread: {cmp_['slower_beyond_spread']}", flush=True)
        report["fc2_producer"] = {**prod, "comparison": cmp_, "shape": [n * s, fc2.cin]}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

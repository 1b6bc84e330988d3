"""What ``attention_head_fusion`` / ``attention_discard_ratio`` cost on the bfloat16 ``FusedViT`` graph, in ONE session,
alternating: the whole forward of a seeded ``--model`` on ``--batch`` x ``--side``^2 patches with maps off, with today's rollout (mean
fusion, nothing discarded: ``tia_mha_probs_h`` + ``tia_rollout_step_f32`` per block) and with the rollout of ``--fusion`` /
``--discard`` (``tia_mha_probs_fused_h`` + ``tia_rollout_discard_normalize_f32`` + ``tia_rollout_product_f32``).  One HIP event pair
per call, ``--warmup`` calls of each variant first, then ``--reps`` rounds with the variants in turn inside every round; the figure is
the median, the spread the inter-quartile range of the rounds.  The yardstick is today's rollout in the same session.

After the timed rounds -- never inside them: tracing slows the host -- one forward of each rollout variant runs under the torch
profiler, and the device time of every map kernel is added up per kernel name: where the added time goes.

Seeded random weights: no pretrained checkpoint is read.

usage: perf_vit_rollout_options.py [--model UNI] [--batch 256] [--side 224] [--depth N] [--fusion max] [--discard 0.9] [--warmup 3]
                                   [--reps 20] [--out FILE.json]"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from perf_vit import build, forward_flops  # noqa: E402
from perf_vit_fp8 import BF16, graph_of  # noqa: E402
from perf_vit_int8 import timed  # noqa: E402

MAP_KERNELS = ("mha_probs_kernel", "rollout_step_kernel", "kth_smallest_kernel", "discard_normalize_kernel")


def _summary(t: dict) -> dict:
    q = statistics.quantiles(t["times"], n=4)
    return {"ms": t["ms"], "iqr_ms": q[2] - q[0], "min_ms": t["min_ms"], "max_ms": t["max_ms"], "times": t["times"]}


def _short(name: str) -> str:
    """``rollout_step_kernel<false>`` of ``void (anonymous namespace)::rollout_step_kernel<false>(float const*, ...)``."""
    head = name.split("(anonymous namespace)::")[-1]
    return head.split("(")[0]


def _map_kernel_ms(fn) -> dict:
    """{kernel: [launches, total device ms]} of one call of ``fn``, the map kernels only."""
    from torch.profiler import ProfilerActivity, profile

    with torch.inference_mode(), profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    out: dict = {}
    for e in prof.events():
        if e.device_type is not None and "cuda" in str(e.device_type).lower() and any(k in e.name for k in MAP_KERNELS):
            entry = out.setdefault(_short(e.name), [0, 0.0])
            entry[0] += 1
            entry[1] += e.device_time / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNI")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--depth", type=int, default=0, help="override the number of blocks (0: the model's own)")
    ap.add_argument("--fusion", default="max")
    ap.add_argument("--discard", type=float, default=0.9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit_rollout_options.py measures on a GPU; none is visible.")
    cfg, vit = build(args)
    flops = forward_flops(cfg, cfg["depth"], args.batch, args.side)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g).to(BF16).contiguous(memory_format=torch.channels_last)
    graph = graph_of(copy.deepcopy(vit), None)
    del vit
    torch.cuda.empty_cache()
    option = f"rollout {args.fusion} {args.discard:g}"

    def run(kind, fusion="mean", discard=0.0):
        def fn():
            graph.return_attention, graph.attention_head_fusion, graph.attention_discard_ratio = kind, fusion, discard
            out = graph(x)
            graph.return_attention, graph.attention_head_fusion, graph.attention_discard_ratio = None, "mean", 0.0
            return out
        return fn

    variants = {"maps off": run(None), "rollout": run("rollout"), option: run("rollout", args.fusion, args.discard)}
    with torch.inference_mode():  # the maps must leave the features alone
        base = variants["maps off"]()
        same = {name: bool(torch.equal(fn(), base)) for name, fn in variants.items()}
    res = {name: _summary(t) for name, t in timed(variants, args.warmup, args.reps).items()}
    print(f"{args.model} depth {cfg['depth']}  {args.batch} x {args.side}^2  ({flops['tokens']} tokens)  {flops['total'] / 1e12:.2f} TFLOP per forward  "
          f"on {torch.cuda.get_device_name(0)};  features equal to maps off: {same}")
    off, today = res["maps off"], res["rollout"]
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        r["over_maps_off"] = r["ms"] / off["ms"]
        r["over_rollout"] = r["ms"] / today["ms"]
        print(f"FusedViT bf16 {name:16s} {r['ms']:9.2f} ms  iqr {r['iqr_ms']:.2f}  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  "
              f"{r['patches_per_s']:8.1f} patches/s  {r['over_maps_off']:.4f} x maps off  {r['over_rollout']:.4f} x today's rollout", flush=True)
    added_today, added_option = today["ms"] - off["ms"], res[option]["ms"] - off["ms"]
    print(f"added over the forward: today's rollout {added_today:.2f} ms, {option} {added_option:.2f} ms "
          f"({added_option / added_today:.2f} x)" if added_today > 0 else "added time of today's rollout is inside the spread", flush=True)
    kernels = {name: _map_kernel_ms(variants[name]) for name in ("rollout", option)}
    for name, table in kernels.items():
        for kernel, (launches, ms) in sorted(table.items(), key=lambda kv: -kv[1][1]):
            print(f"  {name:16s} {kernel:44s} {launches:4d} launches  {ms:9.3f} ms (profiler pass, one forward)", flush=True)
    report = {"model": args.model, "config": cfg, "batch": args.batch, "side": args.side, "warmup": args.warmup, "reps": args.reps,
              "fusion": args.fusion, "discard": args.discard, "features_equal": same, "forward": res,
              "added_ms": {"rollout": added_today, option: added_option}, "map_kernels_ms": kernels}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

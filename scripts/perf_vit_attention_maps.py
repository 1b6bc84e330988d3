"""What ``return_attention`` costs on the bfloat16 ``FusedViT`` graph, in ONE session, alternating: the whole forward of a
seeded ``--model`` on ``--batch`` x ``--side``^2 patches with maps off, with ``"class"`` (one ``tia_mha_probs_h`` launch in the last block)
and with ``"rollout"`` (``tia_mha_probs_h`` over all rows with the head mean and ``tia_rollout_step_f32``, per block).  One HIP event
pair per call, ``--warmup`` calls of each variant first, then ``--reps`` rounds with the variants in turn inside every round; the
figure is the median, the spread the inter-quartile range of the rounds (minimum and maximum are kept as well).

``--parent-file PATH``: a copy of ``models/architecture/vit_fused.py`` as the parent commit has it (``git show HEAD~1:...``).  It is loaded
as a module of its own beside the package and its ``FusedViT`` joins the rounds as "parent": the maps-off graph must be the parent's
-- the same kernels in the same order -- so the two medians may differ by no more than their spread.

Seeded random weights: no pretrained checkpoint is read.

usage: perf_vit_attention_maps.py [--model UNI] [--batch 256] [--side 224] [--depth N] [--warmup 3] [--reps 20] [--parent-file PATH]
                                  [--out FILE.json]"""
from __future__ import annotations

import argparse
import copy
import importlib.util
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


def _summary(t: dict) -> dict:
    q = statistics.quantiles(t["times"], n=4)
    return {"ms": t["ms"], "iqr_ms": q[2] - q[0], "min_ms": t["min_ms"], "max_ms": t["max_ms"], "times": t["times"]}


def _parent_graph(path: str, vit):
    spec = importlib.util.spec_from_file_location("parent_vit_fused", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["parent_vit_fused"] = mod
    spec.loader.exec_module(mod)
    fused = mod.FusedViT(vit)
    fused.prepare(BF16)
    return fused.to(BF16).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNI")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--depth", type=int, default=0, help="override the number of blocks (0: the model's own)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-file", default=None, help="the parent commit's vit_fused.py: its FusedViT is timed in the same rounds")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit_attention_maps.py measures on a GPU; none is visible.")
    cfg, vit = build(args)
    flops = forward_flops(cfg, cfg["depth"], args.batch, args.side)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g).to(BF16).contiguous(memory_format=torch.channels_last)
    graph = graph_of(copy.deepcopy(vit), None)
    parent = _parent_graph(args.parent_file, copy.deepcopy(vit)) if args.parent_file else None
    del vit
    torch.cuda.empty_cache()

    def run(kind):
        def fn():
            graph.return_attention = kind
            out = graph(x)
            graph.return_attention = None
            return out
        return fn

    variants = {"maps off": run(None), "class": run("class"), "rollout": run("rollout")}
    if parent is not None:
        variants["parent"] = lambda: parent(x)
    with torch.inference_mode():  # the maps must leave the features alone
        base = variants["maps off"]()
        same = {name: bool(torch.equal(fn(), base)) for name, fn in variants.items()}
        graph.return_attention = "rollout"
        graph(x)
        shape = tuple(graph.attention_maps.shape)
        graph.return_attention = None
    res = {name: _summary(t) for name, t in timed(variants, args.warmup, args.reps).items()}
    print(f"{args.model} depth {cfg['depth']}  {args.batch} x {args.side}^2  ({flops['tokens']} tokens)  {flops['total'] / 1e12:.2f} TFLOP per forward  "
          f"on {torch.cuda.get_device_name(0)};  rollout maps {shape};  features equal to maps off: {same}")
    off = res["maps off"]
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        r["over_maps_off"] = r["ms"] / off["ms"]
        print(f"FusedViT bf16 {name:9s} {r['ms']:9.2f} ms  iqr {r['iqr_ms']:.2f}  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  "
              f"{r['patches_per_s']:8.1f} patches/s  {r['over_maps_off']:.4f} x maps off", flush=True)
    report = {"model": args.model, "config": cfg, "batch": args.batch, "side": args.side, "warmup": args.warmup, "reps": args.reps,
              "rollout_shape": list(shape), "features_equal": same, "forward": res}
    if parent is not None:
        spread = max(off["iqr_ms"], res["parent"]["iqr_ms"])
        diff = off["ms"] - res["parent"]["ms"]
        report["parent_comparison"] = {"maps_off_minus_parent_ms": diff, "spread_ms": spread, "beyond_spread": bool(abs(diff) > spread)}
        print(f"maps off against the parent's graph: {diff:+.3f} ms beside a spread of {spread:.3f} ms -> beyond the spread: "
              f"{abs(diff) > spread}", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

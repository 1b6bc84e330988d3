"""``FusedViT`` on the float32 route (``prepare(torch.float32, linear_dtype="bfloat16x3")``) beside the float32 torch
module (what ``compute_dtype="float32"`` runs: library GEMMs) and the bfloat16 ``FusedViT`` graph, in ONE session, alternating:

1. whole forward of a seeded ``--model`` on ``--batch`` x ``--side``^2 patches: one HIP event pair per call, ``--warmup`` calls of each
   variant first, then ``--reps`` rounds with the variants in turn; the figure is the median, the spread is (max - min) / median;
2. per layer class (``patch``, ``qkv``, ``proj``, ``fc1``, ``fc2`` at the model's shapes and this batch's rows): the split-bf16 GEMM
   (``tia_conv2d_bf16x3_nhwc_f32``) beside the float32 GEMM (``tia_conv2d_nhwc_f32``) on the same tensors, bias (+ residual) fused;
   one event pair spans ``--inner`` back-to-back launches (a single 0.2 - 4 ms launch per pair showed spreads of 10 - 20 %);
3. ``--accuracy N``: N seeded patches through the float64 module on the CPU, the float32 route, the float32 torch module on the
   device and the bf16 graph: ``e = max |feat - ref| / max(max |ref|, 1)``.  Seeded random weights: no pretrained checkpoint is read.

``--trace-only``: warm up, run the float32 route ``--reps`` times and exit -- the program to put behind
``rocprofv3 --kernel-trace --stats -- python scripts/perf_vit_f32.py --trace-only`` (a run of its own).

usage: perf_vit_f32.py [--model UNI] [--batch 256] [--side 224] [--depth N] [--warmup 2] [--reps 7] [--accuracy N] [--inner 10]
                       [--no-layers] [--trace-only] [--out FILE.json]"""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from perf_vit import build, forward_flops  # noqa: E402
from perf_vit_fp8 import timed  # noqa: E402

SPLIT = "bfloat16x3"


def split_graph(vit):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(vit)
    fused.prepare(torch.float32, linear_dtype=SPLIT)
    return fused.eval()


def bf16_graph(vit):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(vit)
    fused.prepare(torch.bfloat16)
    return fused.to(torch.bfloat16).eval()


def spread(r: dict) -> float:
    return (r["max_ms"] - r["min_ms"]) / r["ms"]


def layer_table(graph, tokens: tuple[int, int], warmup: int, reps: int, inner: int) -> dict:
    """The five layer classes at this batch's rows: the split kernel beside the float32 kernel on the same tensors, ``inner`` launches
    back to back inside every event pair (the figures are per launch)."""
    from tiatoolbox_amd.models.architecture import vit_fused as vf

    n, s = tokens
    g = torch.Generator(device="cuda").manual_seed(2)
    out = {}
    layer = graph.layers[0]
    for name, lin, rows_s in (("patch", graph.patch, s - 1 - graph.reg_tokens), ("qkv", layer["qkv"], s), ("proj", layer["proj"], s),
                              ("fc1", layer["fc1"], s), ("fc2", layer["fc2"], s)):
        w = torch.randn((lin.cout, lin.cin), device="cuda", generator=g) / lin.cin ** 0.5
        a = torch.randn((n, rows_s, lin.cin), device="cuda", generator=g)
        res = torch.randn((n, rows_s, lin.cout), device="cuda", generator=g) if name in ("proj", "fc2") else None
        w3, w32 = vf.pack_linear_weights_split(w), vf.pack_linear_weights_f32(w)

        def launches(wp, a=a, r=res, lin=lin):
            for _ in range(inner):
                vf.hip_linear_f32(a, wp, lin.bias32, r, cout=lin.cout)

        variants = {"float32": lambda w=w32, run=launches: run(w)}
        if w3 is not None:
            variants["split"] = lambda w=w3, run=launches: run(w)
        t = timed(variants, warmup, reps)
        for r_ in t.values():  # per launch
            for key in ("ms", "min_ms", "max_ms"):
                r_[key] /= inner
        flops = 2.0 * n * rows_s * lin.cout * lin.cin
        row = {"shape": [n * rows_s, lin.cout, lin.cin], "float32_ms": t["float32"]["ms"], "float32_spread": spread(t["float32"]),
               "float32_tflops": flops / t["float32"]["ms"] / 1e9, "routed_to": "split" if lin.split else "float32"}
        if w3 is not None:
            row.update({"split_ms": t["split"]["ms"], "split_spread": spread(t["split"]), "split_tflops": flops / t["split"]["ms"] / 1e9})
        out[name] = row
    return out


def accuracy(vit, count: int, side: int) -> dict:
    g = torch.Generator().manual_seed(3)
    x = torch.randn((count, 3, side, side), generator=g)
    with torch.inference_mode():
        ref = copy.deepcopy(vit).cpu().double()(x.double())
        xin = x.cuda().contiguous(memory_format=torch.channels_last)
        got = {"float32 route": split_graph(copy.deepcopy(vit))(xin), "float32 torch module": copy.deepcopy(vit).cuda().float()(xin),
               "bf16 graph": bf16_graph(copy.deepcopy(vit))(xin.to(torch.bfloat16))}
    scale = max(float(ref.abs().max()), 1.0)
    return {name: {"e": float((v.cpu().double() - ref).abs().max()) / scale} for name, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNI")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--depth", type=int, default=0, help="override the number of blocks (0: the model's own)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--accuracy", type=int, default=0, help="patches for the accuracy figures (0: skip; runs the float64 module on the CPU)")
    ap.add_argument("--inner", type=int, default=10, help="launches inside one event pair of the per-layer-class table")
    ap.add_argument("--no-layers", action="store_true", help="skip the per-layer-class table")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit_f32.py measures on a GPU; none is visible.")
    cfg, vit = build(args)
    flops = forward_flops(cfg, cfg["depth"], args.batch, args.side)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    if args.trace_only:
        graph = split_graph(vit)
        with torch.inference_mode():
            graph(x)
            torch.cuda.synchronize()
            for _ in range(args.reps):
                graph(x)
            torch.cuda.synchronize()
        return
    report = {"model": args.model, "config": cfg, "batch": args.batch, "side": args.side, "warmup": args.warmup, "reps": args.reps, "inner": args.inner, "flops": flops}
    if args.accuracy:
        report["accuracy"] = accuracy(vit, args.accuracy, args.side)
        for name, r in report["accuracy"].items():
            print(f"accuracy {args.model} {name:22s} ({args.accuracy} patches, seeded random weights, against the float64 CPU module): e {r['e']:.3e}",
                  flush=True)
    f32_graph, half_graph, module = split_graph(copy.deepcopy(vit)), bf16_graph(copy.deepcopy(vit)), vit.cuda().float().eval()
    xh = x.to(torch.bfloat16)
    kinds = {name: ("split" if f32_graph.layers[0][name].split else "float32") for name in ("qkv", "proj", "fc1", "fc2")}
    kinds["patch"] = "split" if f32_graph.patch.split else "float32"
    res = timed({"torch module float32": lambda: module(x), "FusedViT bfloat16x3": lambda: f32_graph(x), "FusedViT bf16": lambda: half_graph(xh)},
                args.warmup, args.reps)
    print(f"{args.model} depth {cfg['depth']}  {args.batch} x {args.side}^2  ({flops['tokens']} tokens)  {flops['total'] / 1e12:.2f} TFLOP per forward  "
          f"on {torch.cuda.get_device_name(0)}  layers {kinds}")
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        r["tflops"] = flops["total"] / r["ms"] / 1e9
        print(f"{name:24s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}, spread {100 * spread(r):.1f} %]  "
              f"{r['patches_per_s']:8.1f} patches/s  {r['tflops']:7.1f} TFLOP/s", flush=True)
    print(f"float32 route against the float32 torch module: {res['torch module float32']['ms'] / res['FusedViT bfloat16x3']['ms']:.3f}x;  "
          f"against the bf16 graph: {res['FusedViT bf16']['ms'] / res['FusedViT bfloat16x3']['ms']:.3f}x")
    report["forward"] = res
    if not args.no_layers:
        del module, half_graph
        torch.cuda.empty_cache()
        report["layers"] = layer_table(f32_graph, (args.batch, flops["tokens"]), args.warmup, args.reps, args.inner)
        for name, r in report["layers"].items():
            split = (f"split {r['split_ms']:.3f} ms ({r['split_tflops']:.0f} TFLOP/s, spread {100 * r['split_spread']:.1f} %)  "
                     f"{r['float32_ms'] / r['split_ms']:.2f}x") if "split_ms" in r else "split: off the kernel's shapes"
            print(f"{name:5s} rows x N x K = {r['shape']}: float32 {r['float32_ms']:.3f} ms ({r['float32_tflops']:.0f} TFLOP/s, spread "
                  f"{100 * r['float32_spread']:.1f} %)  {split}  [routed to {r['routed_to']}]", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

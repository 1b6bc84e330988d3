"""``FusedViT`` with ``linear_dtype="float8_e4m3"`` beside the bfloat16 ``FusedViT`` graph, in ONE session, alternating:

1. whole forward of a seeded ``--model`` on ``--batch`` x ``--side``^2 patches: one HIP event pair per call, ``--warmup`` calls of each
   variant first, then ``--reps`` timed calls of each in turn; the figure is the median;
2. per layer class (``qkv``, ``fc1``, ``fc2`` at the model's shapes and this batch's rows): the half GEMM (``tia_conv2d_nhwc_h``, 1x1)
   beside the FP8 GEMM (``tia_linear_fp8_rows``), and the producer in front of each beside its quantising form, timed the same way;
   with the least time the shapes allow -- flops at the FP8 matrix rate (twice the bf16 rate) against operand and result bytes at
   the HBM rate -- and the fraction of it reached;
3. ``--accuracy N``: N seeded patches through the float32 module on the CPU, the bf16 graph and the FP8 graph: per-patch cosine
   similarity to the float32 features and ``e = max |feat - ref| / max(max |ref|, 1)``.  Seeded random weights: no pretrained
   checkpoint is read.

``--trace-only fp8|bf16``: warm up, run that graph ``--reps`` times and exit -- the program to put behind
``rocprofv3 --kernel-trace --stats -- python scripts/perf_vit_fp8.py --trace-only fp8`` (a run of its own).

usage: perf_vit_fp8.py [--model UNI] [--batch 256] [--side 224] [--depth N] [--warmup 3] [--reps 20] [--accuracy N] [--no-layers]
                       [--trace-only fp8|bf16] [--out FILE.json]"""
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

BF16 = torch.bfloat16
FP8 = "float8_e4m3"
PEAK_FP8_FLOPS, PEAK_BF16_FLOPS, PEAK_HBM = 5.0e15, 2.5e15, 8.0e12  # dense matrix rates and HBM3E bandwidth of one MI355X


def graph_of(vit, linear_dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(vit)
    fused.prepare(BF16, linear_dtype=linear_dtype)
    return fused.to(BF16).eval()


def timed(variants: dict, warmup: int, reps: int) -> dict:
    """{name: fn} -> {name: {"ms": median, "min_ms", "max_ms"}}: one event pair per call, the variants in turn inside every repetition."""
    with torch.inference_mode():
        for fn in variants.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(reps):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
    return {name: {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for name, t in times.items()}


def layer_table(fp8_graph, bf16_graph, rows: int, tokens: tuple[int, int], warmup: int, reps: int) -> dict:
    """The three layer classes of block 0 at this batch's rows: GEMM and producer, half beside FP8."""
    from tiatoolbox_amd.models.architecture import vit_fused as vf
    from tiatoolbox_amd.models.architecture.vit import LN_EPS

    n, s = tokens
    lf, lh = fp8_graph.layers[0], bf16_graph.layers[0]
    d = fp8_graph.embed_dim
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((n, s, d), device="cuda", generator=g).to(BF16)
    out = {}
    for name in ("qkv", "fc1", "fc2"):
        fp8, half = lf[name], lh[name]
        if not isinstance(fp8, vf._LinearFp8):  # noqa: SLF001
            out[name] = {"fp8": None, "shape": [rows, half.cout, half.cin]}
            continue
        res = x if name == "fc2" else None
        if name == "fc2":
            width_h = half.cin * (2 if fp8_graph.swiglu else 1)
            width_f = fp8.cin * (2 if fp8_graph.swiglu else 1)
            src_h = torch.randn((n, s, width_h), device="cuda", generator=g).to(BF16)
            src_f = torch.randn((n, s, width_f), device="cuda", generator=g).to(BF16)
            prod_h = (lambda t=src_h: vf.hip_swiglu_rows_h(t)) if fp8_graph.swiglu else (lambda t=src_h: vf.hip_gelu_rows_h_(t))
            prod_f = lambda t=src_f: vf.hip_act_rows_q8(t, swiglu=fp8_graph.swiglu)  # noqa: E731
        else:
            norm = lf["norm1" if name == "qkv" else "norm2"]
            prod_h = lambda nm=norm: vf.hip_layernorm_rows_h(x, *nm, eps=LN_EPS, rows=n * s, row_stride=d)  # noqa: E731
            prod_f = lambda nm=norm: vf.hip_layernorm_rows_q8(x, *nm, eps=LN_EPS)  # noqa: E731
        with torch.inference_mode():
            a_h = prod_h().view(n, s, -1)
            a_f = prod_f()
        t = timed({"gemm half": lambda a=a_h, lin=half, r=res: lin(a, residual=r), "gemm fp8": lambda a=a_f, lin=fp8, r=res: lin(a, residual=r),
                   "producer half": prod_h, "producer q8": prod_f}, warmup, reps)
        flops = 2.0 * rows * fp8.cout * fp8.cin
        bytes_fp8 = rows * fp8.cin + fp8.cout * fp8.cin + 2 * rows * fp8.cout * (2 if res is not None else 1) + 4 * (rows + fp8.cout)
        least_ms = max(flops / PEAK_FP8_FLOPS, bytes_fp8 / PEAK_HBM) * 1e3
        out[name] = {"shape": [rows, fp8.cout, fp8.cin], "half_ms": t["gemm half"]["ms"], "fp8_ms": t["gemm fp8"]["ms"],
                     "producer_half_ms": t["producer half"]["ms"], "producer_q8_ms": t["producer q8"]["ms"],
                     "fp8_tflops": flops / t["gemm fp8"]["ms"] / 1e9, "half_tflops": 2.0 * rows * half.cout * half.cin / t["gemm half"]["ms"] / 1e9,
                     "least_ms": least_ms, "bound": "flops" if flops / PEAK_FP8_FLOPS >= bytes_fp8 / PEAK_HBM else "bytes",
                     "fraction_of_bound": least_ms / t["gemm fp8"]["ms"]}
    return out


def accuracy(vit, count: int, side: int) -> dict:
    g = torch.Generator().manual_seed(3)
    x = torch.randn((count, 3, side, side), generator=g)
    with torch.inference_mode():
        ref = copy.deepcopy(vit).cpu().float()(x).double()
        xin = x.cuda().to(BF16).contiguous(memory_format=torch.channels_last)
        res = {}
        for name, linear_dtype in (("bf16 graph", None), ("fp8 graph", FP8)):
            got = graph_of(copy.deepcopy(vit), linear_dtype)(xin).cpu().double()
            cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
            res[name] = {"cosine_min": float(cos.min()), "cosine_mean": float(cos.mean()),
                         "e": float((got - ref).abs().max()) / max(float(ref.abs().max()), 1.0)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNI")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--depth", type=int, default=0, help="override the number of blocks (0: the model's own)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--accuracy", type=int, default=0, help="patches for the accuracy figures (0: skip; runs the float32 module on the CPU)")
    ap.add_argument("--no-layers", action="store_true", help="skip the per-layer-class table")
    ap.add_argument("--trace-only", default=None, choices=["fp8", "bf16"])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit_fp8.py measures on a GPU; none is visible.")
    cfg, vit = build(args)
    flops = forward_flops(cfg, cfg["depth"], args.batch, args.side)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g).to(BF16).contiguous(memory_format=torch.channels_last)
    if args.trace_only:
        graph = graph_of(vit, FP8 if args.trace_only == "fp8" else None)
        with torch.inference_mode():
            graph(x)
            torch.cuda.synchronize()
            for _ in range(args.reps):
                graph(x)
            torch.cuda.synchronize()
        return
    report = {"model": args.model, "config": cfg, "batch": args.batch, "side": args.side, "warmup": args.warmup, "reps": args.reps, "flops": flops}
    if args.accuracy:
        report["accuracy"] = accuracy(vit, args.accuracy, args.side)
        for name, r in report["accuracy"].items():
            print(f"accuracy {args.model} {name:10s} ({args.accuracy} patches, seeded random weights, against the float32 CPU module): "
                  f"cosine min {r['cosine_min']:.6f} mean {r['cosine_mean']:.6f}  e {r['e']:.3e}", flush=True)
    bf16_graph, fp8_graph = graph_of(copy.deepcopy(vit), None), graph_of(copy.deepcopy(vit), FP8)
    del vit
    torch.cuda.empty_cache()
    kinds = {name: type(fp8_graph.layers[0][name]).__name__ for name in ("qkv", "proj", "fc1", "fc2")}
    res = timed({"FusedViT bf16": lambda: bf16_graph(x), "FusedViT bf16 + fp8 linears": lambda: fp8_graph(x)}, args.warmup, args.reps)
    print(f"{args.model} depth {cfg['depth']}  {args.batch} x {args.side}^2  ({flops['tokens']} tokens)  {flops['total'] / 1e12:.2f} TFLOP per forward  "
          f"on {torch.cuda.get_device_name(0)}  layers {kinds}")
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        r["tflops"] = flops["total"] / r["ms"] / 1e9
        print(f"{name:30s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  {r['patches_per_s']:8.1f} patches/s  {r['tflops']:7.1f} TFLOP/s",
              flush=True)
    print(f"speed-up of the forward: {res['FusedViT bf16']['ms'] / res['FusedViT bf16 + fp8 linears']['ms']:.3f}x")
    report["forward"] = res
    if not args.no_layers:
        report["layers"] = layer_table(fp8_graph, bf16_graph, args.batch * flops["tokens"], (args.batch, flops["tokens"]), args.warmup, args.reps)
        for name, r in report["layers"].items():
            if r.get("fp8_ms") is None:
                print(f"{name}: {r['shape']} stays on the half kernel")
                continue
            print(f"{name:4s} rows x N x K = {r['shape']}: half {r['half_ms']:.3f} ms ({r['half_tflops']:.0f} TFLOP/s)  fp8 {r['fp8_ms']:.3f} ms "
                  f"({r['fp8_tflops']:.0f} TFLOP/s, {r['half_ms'] / r['fp8_ms']:.2f}x)  least {r['least_ms']:.3f} ms by {r['bound']}: "
                  f"{100 * r['fraction_of_bound']:.0f} % reached;  producer half {r['producer_half_ms']:.3f} ms  q8 {r['producer_q8_ms']:.3f} ms", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

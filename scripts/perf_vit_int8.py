"""``FusedViT`` with ``linear_dtype="int8"`` beside the bfloat16 ``FusedViT`` graph and the FP8 graph
(``linear_dtype="float8_e4m3"``), in ONE session, alternating:

1. whole forward of a seeded ``--model`` on ``--batch`` x ``--side``^2 patches: one HIP event pair per call, ``--warmup`` calls of each
   variant first, then ``--reps`` timed calls of each in turn; the figure is the median, the spread the rounds' minimum .. maximum;
2. per layer class (``qkv``, ``fc1``, ``fc2`` at block 0's shapes and this batch's rows): the half GEMM (``tia_conv2d_nhwc_h``, 1x1), the
   FP8 GEMM (``tia_linear_fp8_rows``) and the INT8 GEMM (``tia_linear_int8_rows``), and the producer in front of each in its three
   forms, timed the same way; the figure the routing rule of ``tia_linear_int8_serves`` looks at is GEMM + producer, int8 against
   half, per round: the class counts as faster when the medians differ by more than the rounds' spread, the wider of the two
   inter-quartile ranges (a single disturbed round on a shared machine does not move it; minimum and maximum are kept in the JSON); with the least time the shapes allow (flops at the 8-bit matrix rate, twice the bf16 rate,
   against operand and result bytes at the HBM rate);
3. ``--accuracy N``: N seeded patches through the float32 module on the CPU and the bf16, FP8 and INT8 graphs: per-patch cosine
   similarity to the float32 features and ``e = max |feat - ref| / max(max |ref|, 1)``.  Seeded random weights: no pretrained
   checkpoint is read, and what a real checkpoint's activation statistics do to either 8-bit format is not measured here.

``--trace-only int8|fp8|bf16``: warm up, run that graph ``--reps`` times and exit -- the program to put behind
``rocprofv3 --kernel-trace --stats -- python scripts/perf_vit_int8.py --trace-only int8`` (a run of its own, no counters).

usage: perf_vit_int8.py [--model UNI] [--batch 256] [--side 224] [--depth N] [--warmup 3] [--reps 20] [--accuracy N] [--no-layers]
                        [--trace-only int8|fp8|bf16] [--out FILE.json]"""
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
from perf_vit_fp8 import BF16, FP8, PEAK_FP8_FLOPS, PEAK_HBM, graph_of  # noqa: E402

INT8 = "int8"
LINEAR_DTYPES = {"bf16": None, "fp8": FP8, "int8": INT8}


def timed(variants: dict, warmup: int, reps: int) -> dict:
    """``perf_vit_fp8.timed`` with the rounds kept: {name: {"ms": median, "min_ms", "max_ms", "times": [...]}}, one event pair per call,
    the variants in turn inside every round."""
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
    return {name: {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "times": t} for name, t in times.items()}


def _class_rounds(t: dict, gemm: str, producer: str) -> tuple[float, float]:
    """(median, inter-quartile range) of a layer class's per-round time, GEMM + producer of the same round."""
    rounds = [a + b for a, b in zip(t[gemm]["times"], t[producer]["times"])]
    q = statistics.quantiles(rounds, n=4)
    return statistics.median(rounds), q[2] - q[0]


def layer_table(graphs: dict, rows: int, tokens: tuple[int, int], warmup: int, reps: int) -> dict:
    """The three layer classes of block 0 at this batch's rows: GEMM and producer on the half, FP8 and INT8 kernels."""
    from tiatoolbox_amd.models.architecture import vit_fused as vf
    from tiatoolbox_amd.models.architecture.vit import LN_EPS

    n, s = tokens
    layers = {k: g.layers[0] for k, g in graphs.items()}
    swiglu, d = graphs["int8"].swiglu, graphs["int8"].embed_dim
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((n, s, d), device="cuda", generator=g).to(BF16)
    out = {}
    for name in ("qkv", "fc1", "fc2"):
        half, fp8, int8 = (layers[k][name] for k in ("bf16", "fp8", "int8"))
        if not isinstance(int8, vf._LinearInt8) or not isinstance(fp8, vf._LinearFp8):  # noqa: SLF001
            out[name] = {"int8_ms": None, "shape": [rows, half.cout, half.cin]}
            continue
        res = x if name == "fc2" else None
        if name == "fc2":
            src_h = torch.randn((n, s, half.cin * (2 if swiglu else 1)), device="cuda", generator=g).to(BF16)
            src_q = torch.randn((n, s, int8.cin * (2 if swiglu else 1)), device="cuda", generator=g).to(BF16)
            prod_h = (lambda t=src_h: vf.hip_swiglu_rows_h(t)) if swiglu else (lambda t=src_h: vf.hip_gelu_rows_h_(t))
            prod_f = lambda t=src_q: vf.hip_act_rows_q8(t, swiglu=swiglu)  # noqa: E731
            prod_i = lambda t=src_q: vf.hip_act_rows_qi8(t, swiglu=swiglu)  # noqa: E731
        else:
            norm = layers["int8"]["norm1" if name == "qkv" else "norm2"]
            prod_h = lambda nm=norm: vf.hip_layernorm_rows_h(x, *nm, eps=LN_EPS, rows=n * s, row_stride=d)  # noqa: E731
            prod_f = lambda nm=norm: vf.hip_layernorm_rows_q8(x, *nm, eps=LN_EPS)  # noqa: E731
            prod_i = lambda nm=norm: vf.hip_layernorm_rows_qi8(x, *nm, eps=LN_EPS)  # noqa: E731
        with torch.inference_mode():
            a_h, a_f, a_i = prod_h().view(n, s, -1), prod_f(), prod_i()
        t = timed({"gemm half": lambda a=a_h, lin=half, r=res: lin(a, residual=r), "gemm fp8": lambda a=a_f, lin=fp8, r=res: lin(a, residual=r),
                   "gemm int8": lambda a=a_i, lin=int8, r=res: lin(a, residual=r), "producer half": prod_h, "producer q8": prod_f,
                   "producer qi8": prod_i}, warmup, reps)
        flops = 2.0 * rows * int8.cout * int8.cin
        nbytes = rows * int8.cin + int8.cout * int8.cin + 2 * rows * int8.cout * (2 if res is not None else 1) + 4 * (rows + int8.cout)
        least_ms = max(flops / PEAK_FP8_FLOPS, nbytes / PEAK_HBM) * 1e3
        # a class per round is GEMM + producer of that round; the rounds' spread is the wider inter-quartile range of the two
        # classes (one disturbed round of a shared machine does not move it; minimum and maximum are in "raw")
        class_half, iqr_half = _class_rounds(t, "gemm half", "producer half")
        class_int8, iqr_int8 = _class_rounds(t, "gemm int8", "producer qi8")
        spread = max(iqr_half, iqr_int8)
        out[name] = {"shape": [rows, int8.cout, int8.cin], "half_ms": t["gemm half"]["ms"], "fp8_ms": t["gemm fp8"]["ms"],
                     "int8_ms": t["gemm int8"]["ms"], "producer_half_ms": t["producer half"]["ms"], "producer_q8_ms": t["producer q8"]["ms"],
                     "producer_qi8_ms": t["producer qi8"]["ms"], "int8_tflops": flops / t["gemm int8"]["ms"] / 1e9,
                     "fp8_tflops": flops / t["gemm fp8"]["ms"] / 1e9, "half_tflops": 2.0 * rows * half.cout * half.cin / t["gemm half"]["ms"] / 1e9,
                     "class_half_ms": class_half, "class_int8_ms": class_int8, "class_fp8_ms": t["gemm fp8"]["ms"] + t["producer q8"]["ms"],
                     "spread_ms": spread, "int8_faster_beyond_spread": bool(class_half - class_int8 > spread),
                     "least_ms": least_ms, "bound": "flops" if flops / PEAK_FP8_FLOPS >= nbytes / PEAK_HBM else "bytes",
                     "fraction_of_bound": least_ms / t["gemm int8"]["ms"],
                     "raw": {k: {m: v[m] for m in ("ms", "min_ms", "max_ms")} for k, v in t.items()}}
    return out


def accuracy(vit, count: int, side: int) -> dict:
    g = torch.Generator().manual_seed(3)
    x = torch.randn((count, 3, side, side), generator=g)
    with torch.inference_mode():
        ref = copy.deepcopy(vit).cpu().float()(x).double()
        xin = x.cuda().to(BF16).contiguous(memory_format=torch.channels_last)
        res = {}
        for name, linear_dtype in LINEAR_DTYPES.items():
            got = graph_of(copy.deepcopy(vit), linear_dtype)(xin).cpu().double()
            cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
            res[f"{name} graph"] = {"cosine_min": float(cos.min()), "cosine_mean": float(cos.mean()),
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
    ap.add_argument("--trace-only", default=None, choices=list(LINEAR_DTYPES))
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit_int8.py measures on a GPU; none is visible.")
    cfg, vit = build(args)
    flops = forward_flops(cfg, cfg["depth"], args.batch, args.side)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g).to(BF16).contiguous(memory_format=torch.channels_last)
    if args.trace_only:
        graph = graph_of(vit, LINEAR_DTYPES[args.trace_only])
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
    graphs = {name: graph_of(copy.deepcopy(vit), linear_dtype) for name, linear_dtype in LINEAR_DTYPES.items()}
    del vit
    torch.cuda.empty_cache()
    kinds = {name: type(graphs["int8"].layers[0][name]).__name__ for name in ("qkv", "proj", "fc1", "fc2")}
    res = timed({f"FusedViT {name}": (lambda gr=gr: gr(x)) for name, gr in graphs.items()}, args.warmup, args.reps)
    print(f"{args.model} depth {cfg['depth']}  {args.batch} x {args.side}^2  ({flops['tokens']} tokens)  {flops['total'] / 1e12:.2f} TFLOP per forward  "
          f"on {torch.cuda.get_device_name(0)}  layers {kinds}")
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        r["tflops"] = flops["total"] / r["ms"] / 1e9
        print(f"{name:16s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  {r['patches_per_s']:8.1f} patches/s  {r['tflops']:7.1f} TFLOP/s",
              flush=True)
    print(f"int8 forward against bf16: {res['FusedViT bf16']['ms'] / res['FusedViT int8']['ms']:.3f}x, against fp8: "
          f"{res['FusedViT fp8']['ms'] / res['FusedViT int8']['ms']:.3f}x")
    report["forward"] = res
    if not args.no_layers:
        report["layers"] = layer_table(graphs, args.batch * flops["tokens"], (args.batch, flops["tokens"]), args.warmup, args.reps)
        for name, r in report["layers"].items():
            if r.get("int8_ms") is None:
                print(f"{name}: {r['shape']} stays on the half kernel")
                continue
            print(f"{name:4s} rows x N x K = {r['shape']}: GEMM half {r['half_ms']:.3f} ms ({r['half_tflops']:.0f} TFLOP/s)  fp8 {r['fp8_ms']:.3f} ms "
                  f"({r['fp8_tflops']:.0f})  int8 {r['int8_ms']:.3f} ms ({r['int8_tflops']:.0f} TFLOP/s; least {r['least_ms']:.3f} ms by {r['bound']}: "
                  f"{100 * r['fraction_of_bound']:.0f} % reached);  producer half {r['producer_half_ms']:.3f}  q8 {r['producer_q8_ms']:.3f}  "
                  f"qi8 {r['producer_qi8_ms']:.3f} ms;  class (GEMM + producer) half {r['class_half_ms']:.3f}  fp8 {r['class_fp8_ms']:.3f}  "
                  f"int8 {r['class_int8_ms']:.3f} ms, gain {r['class_half_ms'] - r['class_int8_ms']:.3f} ms beside a spread (inter-quartile "
                  f"range of the rounds) of {r['spread_ms']:.3f} ms -> int8 faster beyond the spread: {r['int8_faster_beyond_spread']}", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

"""``FusedViT`` with ``residual_dtype="float32"`` beside the default graph (the residual stream in the half type), in ONE
session, alternating, with DESIGN 4.29's protocol (``perf_vit.alternate``: every variant warmed twice, then ``--rounds`` passes of
``--reps`` forwards each; median [min .. max]):

1. whole forward of a seeded ``--model`` on ``--batch`` x ``--side``^2 patches in bfloat16 and float16, both residual forms;
2. the fused pass alone at the model's shape (``x += float(branch); a = LN(x)`` on ``[batch * tokens, D]``) beside the half LayerNorm it
   replaces, with the bytes each moves (12 and 4 per element) over the time;
3. ``--accuracy N``: N seeded patches through the float32 module on the CPU and both graphs in both half types: per-patch cosine
   similarity to the float32 features and ``e = max |feat - ref| / max(max |ref|, 1)``.  ``--layer-scale G`` sets every LayerScale gamma
   to ``G`` first (default: 1, the seeded models of DESIGN 4.34; timm's initial 1e-5 is the half stream's worst case).  Seeded random
   weights: no pretrained checkpoint is read.

``--trace-only DTYPE``: warm up, run the float32-stream graph ``--reps`` times and exit -- the program to put behind
``rocprofv3 --kernel-trace --stats -- python scripts/perf_vit_resid32.py --trace-only bfloat16`` (a run of its own, no counters).

usage: perf_vit_resid32.py [--model UNI] [--batch 256] [--side 224] [--depth N] [--rounds 5] [--reps 3] [--accuracy N] [--layer-scale G]
                           [--trace-only DTYPE] [--out FILE.json]"""
from __future__ import annotations

import argparse
import copy
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from perf_vit import HALVES, alternate, build, forward_flops  # noqa: E402

PEAK_HBM = 8.0e12  # HBM3E bandwidth of one MI355X, bytes per second
FORMS = {"half": None, "float32": "float32"}


def graph_of(vit, dtype, residual):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(vit)
    fused.prepare(dtype, residual_dtype=residual)
    return fused.to(dtype).eval()


def set_layer_scale(vit, value: float) -> None:
    with torch.no_grad():
        for name, prm in vit.named_parameters():
            if name.endswith("gamma"):
                prm.fill_(value)


def accuracy(vit, count: int, side: int) -> dict:
    g = torch.Generator().manual_seed(3)
    x = torch.randn((count, 3, side, side), generator=g)
    res = {}
    with torch.inference_mode():
        ref = copy.deepcopy(vit).cpu().float()(x).double()
        for name, dtype in HALVES.items():
            xin = x.cuda().to(dtype).contiguous(memory_format=torch.channels_last)
            for form, residual in FORMS.items():
                got = graph_of(copy.deepcopy(vit), dtype, residual)(xin).cpu().double()
                cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
                res[f"{name} residual {form}"] = {"cosine_min": float(cos.min()), "cosine_mean": float(cos.mean()),
                                                  "e": float((got - ref).abs().max()) / max(float(ref.abs().max()), 1.0)}
    return res


def fused_pass(rows: int, d: int, rounds: int, reps: int) -> dict:
    """The add + LayerNorm pass on ``[rows, d]`` beside the half LayerNorm, per half type: ms, bytes moved, fraction of the HBM rate."""
    from tiatoolbox_amd.models.architecture import vit_fused as vf
    from tiatoolbox_amd.models.architecture.vit import LN_EPS

    g = torch.Generator(device="cuda").manual_seed(2)
    gamma, beta = torch.rand(d, device="cuda", generator=g) + 0.5, torch.randn(d, device="cuda", generator=g) * 0.1
    out = {}
    for name, dtype in HALVES.items():
        x32 = torch.randn((1, rows, d), device="cuda", generator=g)
        branch = (torch.randn((1, rows, d), device="cuda", generator=g) * 1e-3).to(dtype)  # (small: x stays finite over the repeats)
        xh = x32.to(dtype)
        res = alternate({
            "add + LayerNorm (float32 stream)": lambda: vf.hip_add_layernorm_rows_f32(x32, branch, gamma, beta, eps=LN_EPS, rows=rows,  # noqa: B023
                                                                                      row_stride=d, dtype=dtype),  # noqa: B023
            "LayerNorm (half stream)": lambda: vf.hip_layernorm_rows_h(xh, gamma, beta, eps=LN_EPS, rows=rows, row_stride=d)},  # noqa: B023
            rounds, max(reps, 10))
        for what, per_element in (("add + LayerNorm (float32 stream)", 12), ("LayerNorm (half stream)", 4)):
            r = res[what]
            r["bytes"] = per_element * rows * d
            r["bytes_per_s"] = r["bytes"] / r["ms"] * 1e3
            r["fraction_of_hbm"] = r["bytes_per_s"] / PEAK_HBM
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNI")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--depth", type=int, default=0, help="override the number of blocks (0: the model's own)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--accuracy", type=int, default=0, help="patches for the accuracy figures (0: skip; runs the float32 module on the CPU)")
    ap.add_argument("--layer-scale", type=float, default=None, help="set every LayerScale gamma to this value (default: 1)")
    ap.add_argument("--no-timing", action="store_true", help="accuracy only")
    ap.add_argument("--trace-only", default=None, choices=sorted(HALVES))
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit_resid32.py measures on a GPU; none is visible.")
    cfg, vit = build(args)
    if args.layer_scale is not None:
        set_layer_scale(vit, args.layer_scale)
    flops = forward_flops(cfg, cfg["depth"], args.batch, args.side)
    if args.trace_only:
        dtype = HALVES[args.trace_only]
        g = torch.Generator(device="cuda").manual_seed(1)
        xin = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
        fused = graph_of(vit, dtype, "float32")
        with torch.inference_mode():
            fused(xin)
            torch.cuda.synchronize()
            for _ in range(args.reps):
                fused(xin)
            torch.cuda.synchronize()
        return
    report = {"model": args.model, "config": cfg, "layer_scale": 1.0 if args.layer_scale is None else args.layer_scale, "batch": args.batch,
              "side": args.side, "rounds": args.rounds, "reps": args.reps, "flops": flops}
    if args.accuracy:
        report["accuracy"] = accuracy(vit, args.accuracy, args.side)
        for name, r in report["accuracy"].items():
            print(f"accuracy {args.model} gamma {report['layer_scale']:g} {name:26s} ({args.accuracy} patches, seeded random weights, against the "
                  f"float32 CPU module): cosine min {r['cosine_min']:.6f} mean {r['cosine_mean']:.6f}  e {r['e']:.3e}", flush=True)
    if not args.no_timing:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g)
        variants = {}
        for name, dtype in HALVES.items():
            xin = x.to(dtype).contiguous(memory_format=torch.channels_last)
            for form, residual in FORMS.items():
                variants[f"FusedViT {name} residual {form}"] = lambda m=graph_of(copy.deepcopy(vit), dtype, residual), xi=xin: m(xi)
        del vit, x
        torch.cuda.empty_cache()
        res = alternate(variants, args.rounds, args.reps)
        print(f"{args.model} depth {cfg['depth']}  {args.batch} x {args.side}^2  ({flops['tokens']} tokens)  {flops['total'] / 1e12:.2f} TFLOP per "
              f"forward  on {torch.cuda.get_device_name(0)}")
        for name, r in res.items():
            r["patches_per_s"] = args.batch / r["ms"] * 1e3
            r["tflops"] = flops["total"] / r["ms"] / 1e9
            print(f"{name:36s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  {r['patches_per_s']:8.1f} patches/s  "
                  f"{r['tflops']:7.1f} TFLOP/s", flush=True)
        for name in HALVES:
            cost = res[f"FusedViT {name} residual float32"]["ms"] / res[f"FusedViT {name} residual half"]["ms"] - 1.0
            print(f"cost of the float32 stream, {name}: {100 * cost:+.1f} % of the forward")
        report["forward"] = res
        del variants
        torch.cuda.empty_cache()
        rows = args.batch * flops["tokens"]
        report["fused_pass"] = fused_pass(rows, cfg["embed_dim"], args.rounds, args.reps)
        for name, passes in report["fused_pass"].items():
            for what, r in passes.items():
                print(f"pass [{rows}, {cfg['embed_dim']}] {name:9s} {what:34s} {r['ms']:7.3f} ms  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]  "
                      f"{r['bytes_per_s'] / 1e12:5.2f} TB/s  ({100 * r['fraction_of_hbm']:.0f} % of 8 TB/s)", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

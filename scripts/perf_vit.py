"""``FusedViT`` (the Vision Transformer backbones on the hand-written kernels) beside the torch module cast to the same dtype
on the same device (library GEMMs and attention), in ONE session, alternating:

1. whole forward (normalised float patches in the run's dtype -> float32 features) of a seeded ``--model`` (default ``UNI``: ViT-L/16 with
   LayerScale; any name of ``VIT_CONFIGS`` / ``VIRCHOW_CONFIGS``, e.g. ``UNI2`` or ``H-optimus-0``, DESIGN 4.31, ``Virchow2``) on ``--batch`` x ``--side``^2 patches, in
   bfloat16 and float16;
2. the algorithmic flops of that forward (GEMMs and the two attention products, from the shapes) over the time: TFLOP/s end to end.

``--trace-only DTYPE``: warm up, then run the fused forward ``--reps`` times and exit -- the program to put behind
``rocprofv3 --kernel-trace --stats -- python scripts/perf_vit.py --trace-only bfloat16`` for the per-kernel shares (a run of its own, no
counters); ``scripts/prof_summarize.py`` condenses its CSV.

usage: perf_vit.py [--model UNI] [--batch 256] [--side 224] [--depth N] [--rounds 5] [--reps 3] [--no-cast] [--trace-only DTYPE] [--out FILE.json]
Times: HIP events on the launch stream around ``reps`` calls after a warm-up of every variant; variants alternate inside a round, the
figure reported is the median over rounds (min and max kept).  The input is made once; every forward allocates its own activations
through the caching allocator (warm after the first call), as the engines' batches do."""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

HALVES = {"bfloat16": torch.bfloat16, "float16": torch.float16}


def ev(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants: dict, rounds: int, reps: int) -> dict:
    """{name: fn} -> {name: {"ms": median, "min_ms", "max_ms"}}; every variant warmed first, then `rounds` passes over all of them."""
    with torch.inference_mode():
        for fn in variants.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                times[name].append(ev(fn, reps))
    return {name: {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for name, t in times.items()}


def forward_flops(cfg: dict, depth: int, batch: int, side: int) -> dict:
    """Multiply-adds x 2 of one forward, from the shapes: the GEMMs (patch embedding, qkv, proj, fc1, fc2) and attention (QK^T and PV).
    The packed SwiGLU's fc2 reads half of fc1's width; register tokens lengthen the sequence; the zero columns of a padded patch
    row are not counted (they are no work the algorithm needs)."""
    d, m, p = cfg["embed_dim"], cfg["mlp_dim"], cfg["patch_size"]
    g = (side // p) ** 2
    s = g + 1 + cfg.get("reg_tokens", 0)
    mlp = d * m + d * m // 2 if cfg.get("mlp_layer", "mlp") == "swiglu_packed" else 2 * d * m
    gemm = 2.0 * batch * (g * 3 * p * p * d + depth * s * (3 * d * d + d * d + mlp))
    attn = 2.0 * batch * depth * 2 * s * s * d
    return {"gemm": gemm, "attention": attn, "total": gemm + attn, "tokens": s}


def build(args):
    from tiatoolbox_amd.models.architecture.vit import VisionTransformer, vit_config

    cfg = dict(vit_config(args.model))
    if args.depth:
        cfg["depth"] = args.depth
    torch.manual_seed(0)
    with torch.device("cuda"):
        vit = VisionTransformer(**cfg).eval()
    if cfg.get("init_values"):
        with torch.no_grad():
            for name, prm in vit.named_parameters():
                if name.endswith("gamma"):
                    prm.fill_(1.0)  # (timm's 1e-5 is a training start: pretrained LayerScales are of order 0.1 .. 1)
    return cfg, vit


def fused_of(vit, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(vit)  # (shares the float32 parameters until `prepare` has packed its own)
    fused.prepare(dtype)
    return fused.to(dtype).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNI")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--depth", type=int, default=0, help="override the number of blocks (0: the model's own)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cast", action="store_true", help="skip the cast torch module (library GEMMs)")
    ap.add_argument("--trace-only", default=None, choices=sorted(HALVES))
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit.py measures on a GPU; none is visible.")
    cfg, vit = build(args)
    flops = forward_flops(cfg, cfg["depth"], args.batch, args.side)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((args.batch, 3, args.side, args.side), device="cuda", generator=g)
    if args.trace_only:
        dtype = HALVES[args.trace_only]
        fused = fused_of(vit, dtype)
        xin = x.to(dtype).contiguous(memory_format=torch.channels_last)
        with torch.inference_mode():
            fused(xin)
            torch.cuda.synchronize()
            for _ in range(args.reps):
                fused(xin)
            torch.cuda.synchronize()
        return
    variants = {}
    for name, dtype in HALVES.items():
        xin = x.to(dtype).contiguous(memory_format=torch.channels_last)
        if not args.no_cast:
            cast = copy.deepcopy(vit).to(dtype).eval()
            variants[f"cast torch module {name}"] = lambda m=cast, xi=xin: m(xi).float()
        variants[f"FusedViT {name}"] = lambda m=fused_of(copy.deepcopy(vit), dtype), xi=xin: m(xi)
    del vit
    torch.cuda.empty_cache()
    res = alternate(variants, args.rounds, args.reps)
    print(f"{args.model} depth {cfg['depth']}  {args.batch} x {args.side}^2  ({flops['tokens']} tokens)  {flops['total'] / 1e12:.2f} TFLOP per forward "
          f"(attention {100 * flops['attention'] / flops['total']:.1f} %)  on {torch.cuda.get_device_name(0)}")
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        r["tflops"] = flops["total"] / r["ms"] / 1e9
        print(f"{name:30s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  {r['patches_per_s']:8.1f} patches/s  "
              f"{r['tflops']:7.1f} TFLOP/s", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"model": args.model, "config": cfg, "batch": args.batch, "side": args.side, "rounds": args.rounds,
                                              "reps": args.reps, "flops": flops, "forward": res}, indent=1))


if __name__ == "__main__":
    main()

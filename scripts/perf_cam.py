"""What ``return_cam`` costs, and what the ``cam`` kernel reaches.  One session per ``--model`` and ``--dtype``:

* ``forward``: ``PatchPredictor(model).run`` on ``--patches`` x 224^2 device-resident uint8 patches (seeded synthetic H&E) without and
  with ``return_cam=True``, alternating inside every round: one HIP event pair per run, ``--warmup`` runs of each first, then
  ``--reps`` rounds; the figure is the median, the spread the inter-quartile range.  A run ends with its results on the host, the
  maps included (``patches * K * 49 * 4`` bytes).
* ``kernel``: ``hip_cam`` alone on ``[patches, C, 7, 7]`` feature maps of the model's width, ``|N(0, 1)|``, in enough rotating buffers
  that no launch finds its input in the 256 MiB Infinity Cache, timed by events per launch; the bytes are ``n hw c sizeof(x)`` read
  plus ``n k hw 4`` written, over the median time, beside 8 TB/s.  ``torch.einsum("nhwc,kc->nkhw")`` on the same buffers (in half:
  with the weights in the half type, a half result) is timed in the same rounds.
* ``--mode profile``: the kernel alone, ``--reps`` launches on the rotating buffers, for a ``rocprofv3 --kernel-trace --stats`` run of its
  own (the kernel's time without the host).

Seeded random weights: no pretrained checkpoint is read.  One GPU.

usage: perf_cam.py [--model resnet18-kather100k] [--dtype float32] [--patches 4096] [--batch 1024] [--warmup 3] [--reps 20]
                   [--mode forward,kernel | profile] [--out FILE.json]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

HBM_PEAK = 8e12  # bytes/s
L3_BYTES = 256 << 20


def timed(variants: dict, warmup: int, reps: int) -> dict:
    """Median / quartiles of ``reps`` rounds, the variants in turn inside every round, one event pair per call."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    out = {}
    for name, t in times.items():
        q = statistics.quantiles(t, n=4) if len(t) > 1 else [t[0]] * 3
        out[name] = {"ms": statistics.median(t), "iqr_ms": q[2] - q[0], "min_ms": min(t), "max_ms": max(t)}
    return out


def kernel_buffers(n: int, c: int, k: int, dtype: torch.dtype):
    per = n * 49 * c * torch.empty((), dtype=dtype).element_size()
    count = max(2, -(-2 * L3_BYTES // per))  # two caches' worth of other inputs between two uses of a buffer
    g = torch.Generator(device="cuda").manual_seed(3)
    xs = [torch.randn((n, 7, 7, c), device="cuda", generator=g).abs().to(dtype).permute(0, 3, 1, 2) for _ in range(count)]
    return xs, torch.randn((k, c), device="cuda", generator=g), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet18-kather100k")
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16", "bfloat16"])
    ap.add_argument("--patches", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mode", default="forward,kernel")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_cam.py measures on a GPU; none is visible.")
    from tiatoolbox_amd.models.architecture.fused import hip_cam
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.utils import synth

    dtype = getattr(torch, args.dtype)
    eng = PatchPredictor(args.model, batch_size=args.batch, device="cuda", verbose=False)
    k, c = eng.model.classifier.weight.shape
    report = {"model": args.model, "dtype": args.dtype, "patches": args.patches, "batch": args.batch, "classes": k, "channels": c,
              "device": torch.cuda.get_device_name(0)}
    modes = args.mode.split(",")

    if "profile" in modes:
        xs, w, _ = kernel_buffers(args.patches, c, k, dtype)
        out = torch.empty((args.patches, k, 7, 7), device="cuda")
        for i in range(args.warmup + args.reps):
            hip_cam(xs[i % len(xs)], w, out=out)
        torch.cuda.synchronize()
        print(f"{args.reps + args.warmup} launches of the cam kernel on {len(xs)} rotating buffers [{args.patches}, {c}, 7, 7] {args.dtype}, K = {k}")
        return

    if "forward" in modes:
        base = synth.g_he(64, 224, 224, seed=11)
        x = torch.from_numpy(base).cuda().repeat(-(-args.patches // 64), 1, 1, 1)[:args.patches].contiguous()
        kw = {"patch_mode": True, "compute_dtype": args.dtype}
        plain, maps = eng.run(x, **kw), eng.run(x, return_cam=True, **kw)
        same = bool((plain["predictions"] == maps["predictions"]).all())
        res = timed({"without": lambda: eng.run(x, **kw), "return_cam": lambda: eng.run(x, return_cam=True, **kw)}, args.warmup, args.reps)
        added = res["return_cam"]["ms"] - res["without"]["ms"]
        spread = max(res["without"]["iqr_ms"], res["return_cam"]["iqr_ms"])
        report["forward"] = res | {"added_ms": added, "spread_ms": spread, "inside_spread": bool(abs(added) <= spread),
                                   "predictions_equal": same, "cam_shape": list(maps["cam"].shape)}
        for name, r in res.items():
            print(f"{args.model} {args.dtype} run {name:10s} {r['ms']:9.3f} ms  iqr {r['iqr_ms']:.3f}  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]  "
                  f"{args.patches / r['ms'] * 1e3:9.1f} patches/s", flush=True)
        print(f"return_cam adds {added:+.3f} ms beside a spread of {spread:.3f} ms -> inside the spread: {abs(added) <= spread}; "
              f"cam {tuple(maps['cam'].shape)}; predictions equal: {same}", flush=True)
        del x
        torch.cuda.empty_cache()

    if "kernel" in modes:
        xs, w, per = kernel_buffers(args.patches, c, k, dtype)
        out = torch.empty((args.patches, k, 7, 7), device="cuda")
        wd = w.to(dtype)
        turn = {"cam": 0, "einsum": 0}

        def cam():
            turn["cam"] += 1
            hip_cam(xs[turn["cam"] % len(xs)], w, out=out)

        def einsum():
            turn["einsum"] += 1
            torch.einsum("nhwc,kc->nkhw", xs[turn["einsum"] % len(xs)].permute(0, 2, 3, 1), wd)

        res = timed({"tia_cam_nhwc": cam, "torch.einsum": einsum}, args.warmup, args.reps)
        nbytes = per + args.patches * k * 49 * 4
        for name, r in res.items():
            r["bytes"] = nbytes
            r["tb_per_s"] = nbytes / (r["ms"] * 1e-3) / 1e12
            r["share_of_8_tb_per_s"] = nbytes / (r["ms"] * 1e-3) / HBM_PEAK
            print(f"{name:14s} [{args.patches}, {c}, 7, 7] {args.dtype} K = {k}: {r['ms'] * 1e3:9.1f} us  iqr {r['iqr_ms'] * 1e3:.1f}  "
                  f"{nbytes / 1e6:.1f} MB -> {r['tb_per_s']:.2f} TB/s = {100 * r['share_of_8_tb_per_s']:.1f} % of 8 TB/s  "
                  f"({len(xs)} rotating buffers: not cache-resident; event-timed, launch included)", flush=True)
        report["kernel"] = res | {"buffers": len(xs)}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

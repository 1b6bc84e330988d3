"""The plain-encoder UNet on the fused graph (``FusedPlainUNet``) beside what ran before it -- the channels-last torch
module on library convolutions, cast for half -- all in ONE session, alternating:

1. the two streaming kernels alone on ``--batch`` x ``--side``^2 x 64 channels, float32 / fp16 / bf16, in bytes/s:
   ``hip_avgpool2x2`` against ``F.avg_pool2d(x, 2, 2)`` (1.25 elements moved per input element), ``hip_upsample2x_concat`` against
   ``torch.cat([F.interpolate(x, scale_factor=2), y], 1)`` (3.25 elements per element of ``y``), and
   ``tia_upsample2x_add_act_nhwc_*`` (``hip_upsample2x_add``, 2.25 elements per element of ``y``) on the same tensors as the
   yardstick of the same class of kernel;
2. the whole forward (float patches in the parameters' dtype, as ``infer_batch`` hands them over -> float32 logits) of seeded
   ``UNetModel(3, 2, "unet", decoder_block=[3])`` with ``skip_type`` ``"add"`` and ``"concat"``: float32 under ``conv_algo`` ``"auto"``
   and ``"direct"``, fp16, bf16 -- the fused graph and the torch module of the same dtype.

The verdict per row: the fused figure is not slower than the torch figure by more than the run-to-run spread (max - min over the
rounds) of the TORCH figure in this same call; both are printed next to the numbers.

usage: perf_unet_plain.py [--batch 16] [--side 1024] [--rounds 3] [--reps 2] [--out FILE.json]
Times: HIP events on the launch stream around ``reps`` calls ending in a synchronise, after a warm-up of every variant; variants
alternate inside a round and the figure reported is the median over rounds (min and max kept)."""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F  # noqa: N812

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tiatoolbox_amd.models.architecture import fused as K  # noqa: E402, N812

PEAK_BW = 8.0e12
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def ev(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants: dict, rounds: int, reps: int, *, progress: bool = False) -> dict:
    """{name: fn} -> {name: {"ms": median, "min_ms", "max_ms"}}; every variant warmed first, then `rounds` passes over all of them.
    ``progress``: a line per warm-up and per round (a library's first call of a shape can take minutes to pick or build its kernels)."""
    with torch.inference_mode():
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if progress:
                print(f"  warm-up {name:24s} {time.perf_counter() - t0:8.2f} s", flush=True)
        times = {name: [] for name in variants}
        for i in range(rounds):
            for name, fn in variants.items():
                times[name].append(ev(fn, reps))
            if progress:
                print(f"  round {i + 1} of {rounds}: " + "  ".join(f"{t[-1]:.1f}" for t in times.values()) + " ms", flush=True)
    return {name: {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for name, t in times.items()}


def verdict(new: dict, old: dict) -> dict:
    spread = old["max_ms"] - old["min_ms"]
    return {"parent_spread_ms": spread, "not_slower": new["ms"] <= old["ms"] + spread, "speedup": old["ms"] / new["ms"]}


def kernel_reps(args) -> int:
    return max(args.reps, 10)  # a kernel call is about a millisecond: time ten at the least


def kernel_table(args) -> list[dict]:
    n, side, c = args.batch, args.side, 64
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for name, dtype in DTYPES.items():
        big = torch.randn((n, side, side, c), device="cuda", generator=g).to(dtype).permute(0, 3, 1, 2)  # channels-last [n, c, side, side]
        small = torch.randn((n, side // 2, side // 2, c), device="cuda", generator=g).to(dtype).permute(0, 3, 1, 2)
        esz = big.element_size()
        nbytes = {"avgpool": 1.25 * esz * big.numel(), "concat": 3.25 * esz * big.numel(), "add": 2.25 * esz * big.numel()}
        variants = {
            "avgpool hip": lambda x=big: K.hip_avgpool2x2(x),
            "avgpool torch": lambda x=big: F.avg_pool2d(x, 2, 2),
            "concat hip": lambda x=small, y=big: K.hip_upsample2x_concat(x, y),
            "concat torch": lambda x=small, y=big: torch.cat([F.interpolate(x, scale_factor=2), y], 1),
            "add hip": lambda x=small, y=big: K.hip_upsample2x_add(x, y),
        }
        with torch.inference_mode():  # right results before anything is timed: the CPU's on the first image (equality), the device's torch ops
            assert torch.equal(K.hip_avgpool2x2(big[:1]).cpu(), F.avg_pool2d(big[:1].cpu(), 2, 2))
            assert torch.equal(variants["concat hip"](), variants["concat torch"]())
            gap = float((variants["avgpool hip"]().float() - variants["avgpool torch"]().float()).abs().max())
            print(f"{name}: avgpool == CPU avg_pool2d on image 0, max |diff| to the device's avg_pool2d {gap:.3e}; concat == torch.cat", flush=True)
        res = alternate(variants, args.rounds, kernel_reps(args))
        for vname, r in res.items():
            kind = vname.split()[0]
            row = {"kernel": kind, "variant": vname, "dtype": name, "shape": f"{n}x{side}x{side}x{c}", **r,
                   "gbytes": nbytes[kind] / 1e9, "tb_per_s": nbytes[kind] / r["ms"] / 1e9,
                   "fraction_of_8tbs": nbytes[kind] / PEAK_BW / (r["ms"] * 1e-3)}
            if vname.endswith("hip") and kind != "add":
                row.update(verdict(r, res[f"{kind} torch"]))
            rows.append(row)
            tail = (f"  x{row['speedup']:.2f} of torch (its spread {row['parent_spread_ms']:.3f} ms): "
                    f"{'not slower' if row['not_slower'] else 'SLOWER'}") if "speedup" in row else ""
            print(f"{vname:14s} {name:9s} {row['shape']:18s} {r['ms']:8.3f} ms  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]  "
                  f"{row['gbytes']:7.3f} GB  {row['tb_per_s']:5.2f} TB/s  {100 * row['fraction_of_8tbs']:5.1f} % of 8 TB/s{tail}", flush=True)
        del big, small, variants
        torch.cuda.empty_cache()
    return rows


def forward_table(args, skip: str) -> list[dict]:
    from tiatoolbox_amd.models.architecture.hovernet_fused import set_conv_algo
    from tiatoolbox_amd.models.architecture.unet import UNetModel
    from tiatoolbox_amd.models.architecture.unet_fused import FusedPlainUNet
    from tiatoolbox_amd.utils import synth

    base = torch.from_numpy(synth.g_he(4, args.side, args.side, seed=9)).cuda()
    x8 = base.repeat(-(-args.batch // 4), 1, 1, 1)[:args.batch].contiguous()  # NHWC uint8
    rows = []
    torch.manual_seed(1)
    model = UNetModel(3, 2, "unet", decoder_block=[3], skip_type=skip).eval()
    variants, pairs = {}, []
    for name, dtype in DTYPES.items():
        imgs = x8.to(dtype).permute(0, 3, 1, 2)  # what `infer_batch` passes: the parameters' dtype, channels-last
        cast = copy.deepcopy(model).cuda().to(dtype).to(memory_format=torch.channels_last).eval()
        variants[f"torch module {name}"] = lambda m=cast, xi=imgs: m(xi).float()
        for algo in (("auto", "direct") if dtype == torch.float32 else ("",)):
            fused = FusedPlainUNet(copy.deepcopy(model).cuda()).cuda()
            if dtype == torch.float32:
                set_conv_algo(fused, "winograd" if algo == "auto" else "direct")  # what the engines' conv_algo selects
            else:
                fused.prepare(dtype)
                fused = fused.to(dtype)
            fused = fused.to(memory_format=torch.channels_last).eval()
            label = f"fused {name}" + (f" ({algo})" if algo else "")
            variants[label] = lambda m=fused, xi=imgs: m(xi)
            pairs.append((label, f"torch module {name}"))
    res = alternate(variants, args.rounds, args.reps, progress=True)
    for new, old in pairs:
        row = {"skip_type": skip, "variant": new, "fused": res[new], "torch": res[old], **verdict(res[new], res[old]),
               "fused_patches_per_s": args.batch / res[new]["ms"] * 1e3, "torch_patches_per_s": args.batch / res[old]["ms"] * 1e3}
        rows.append(row)
        print(f"forward {args.batch} x {args.side}^2 skip={skip:6s} {new:24s} {res[new]['ms']:9.2f} ms "
              f"[{res[new]['min_ms']:.2f} .. {res[new]['max_ms']:.2f}] {row['fused_patches_per_s']:7.1f} patches/s | torch module "
              f"{res[old]['ms']:9.2f} ms [{res[old]['min_ms']:.2f} .. {res[old]['max_ms']:.2f}] {row['torch_patches_per_s']:7.1f} patches/s | "
              f"x{row['speedup']:.2f}, torch spread {row['parent_spread_ms']:.2f} ms: {'not slower' if row['not_slower'] else 'SLOWER'}",
              flush=True)
    del variants
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_unet_plain.py measures on a GPU; none is visible.")
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "side": args.side, "rounds": args.rounds, "reps": args.reps}
    result["kernel_reps"] = kernel_reps(args)
    print(f"{result['device']}: {args.batch} patches of {args.side}^2, median of {args.rounds} rounds; {kernel_reps(args)} calls per round in the "
          f"kernel table, {args.reps} in the forward table", flush=True)

    def save():  # after every table: a run that is cut short keeps what it has measured
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result, indent=1))

    result["kernels"] = kernel_table(args)
    save()
    result["forward"] = []
    for skip in ("add", "concat"):
        result["forward"] += forward_table(args, skip)
        save()


if __name__ == "__main__":
    main()

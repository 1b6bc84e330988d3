"""The half-precision ``FusedHoVerNet`` (``compute_dtype="float16" | "bfloat16"`` of ``NucleusInstanceSegmentor`` / ``MultiTaskSegmentor``,
DESIGN 4.24) beside the float32 one and beside what the option ran before (the torch module cast to the dtype), all in ONE session,
alternating:

1. whole forward (float tiles in the copy's dtype -> float32 logits) of seeded ``hovernet_fast-pannuke`` on ``--batch`` x 256^2 tiles:
   (i) float32 ``FusedHoVerNet`` under ``conv_algo="auto"``, (ii) half ``FusedHoVerNet`` fp16 / bf16, (iii)
   ``copy.deepcopy(model).cuda().to(dtype)``;
2. the four new kernels at the network's own shapes: time, algorithmic bytes, fraction of 8 TB/s, the float32 kernel beside it
   (grouped valid: every input element once + the 32 new channels; view activation: in + out; conv3 + shortcut with both outputs:
   x + residual + y + y2 + weights; stem: 12 bytes per input pixel + the output map);
3. ``NucleusInstanceSegmentor.run`` on the 256 tiles of ``bench_configs.bench_hovernet`` (the same recipe), tiles/s for float32 /
   float16 / bfloat16.

usage: perf_hovernet_half.py [--batch 32] [--rounds 3] [--reps 3] [--tiles 256] [--no-engine] [--no-cast] [--out FILE.json]
Times: HIP events on the launch stream around ``reps`` calls after a warm-up of every variant; variants alternate inside a round and
the figure reported is the median over rounds (min and max kept in the JSON)."""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import time
import warnings
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tiatoolbox_amd.models.architecture import fused as K  # noqa: E402, N812

PEAK_BW = 8.0e12
HALVES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
ALL = (("float32", torch.float32), *HALVES.items())


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
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                times[name].append(ev(fn, reps))
    return {name: {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for name, t in times.items()}


def forward_table(args) -> dict:
    from tiatoolbox_amd.models.architecture import get_pretrained_model
    from tiatoolbox_amd.models.architecture.hovernet_fused import FusedHoVerNet, set_conv_algo
    from tiatoolbox_amd.utils import synth

    model, _ = get_pretrained_model("hovernet_fast-pannuke")
    model = model.eval()
    base = torch.from_numpy(synth.g_he(4, 256, 256, seed=5)).cuda()
    x = base.repeat(-(-args.batch // 4), 1, 1, 1)[:args.batch].float().permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
    variants = {}
    f32 = FusedHoVerNet(copy.deepcopy(model).cuda()).cuda().to(memory_format=torch.channels_last).eval()
    set_conv_algo(f32, "winograd")  # what the engines' conv_algo="auto" selects
    variants["fused float32 (auto)"] = lambda: f32(x)
    for name, dtype in HALVES.items():
        half = FusedHoVerNet(copy.deepcopy(model).cuda())
        half.prepare(dtype)
        half = half.to(dtype).to(memory_format=torch.channels_last).eval()
        xin = x.to(dtype).contiguous(memory_format=torch.channels_last)
        variants[f"fused {name}"] = lambda m=half, xi=xin: m(xi)
        if not args.no_cast:
            cast = copy.deepcopy(model).cuda().to(dtype).to(memory_format=torch.channels_last).eval()
            variants[f"cast torch module {name}"] = lambda m=cast, xi=xin: {k: v.float() for k, v in m(xi).items()}
    res = alternate(variants, args.rounds, args.reps)
    for name, r in res.items():
        r["tiles_per_s"] = args.batch / r["ms"] * 1e3
        print(f"forward {args.batch} x 256^2  {name:28s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  "
              f"{r['tiles_per_s']:8.1f} tiles/s", flush=True)
    return res


def kernel_table(args) -> list[dict]:
    n = args.batch
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []

    def rand(shape, dtype):
        return torch.randn(shape, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)

    def add(kernel, shape, nbytes, variants):
        res = alternate(variants, args.rounds, max(args.reps, 10))
        for name, r in res.items():
            row = {"kernel": kernel, "shape": shape, "variant": name, "ms": r["ms"], "min_ms": r["min_ms"], "max_ms": r["max_ms"],
                   "gbytes": nbytes[name] / 1e9, "tb_per_s": nbytes[name] / r["ms"] / 1e9, "fraction_of_8tbs": nbytes[name] / PEAK_BW / (r["ms"] * 1e-3)}
            rows.append(row)
            print(f"{kernel:14s} {shape:26s} {name:9s} {r['ms']:8.3f} ms  {row['gbytes']:7.3f} GB  {row['tb_per_s']:5.2f} TB/s  "
                  f"{100 * row['fraction_of_8tbs']:5.1f} % of 8 TB/s", flush=True)

    # the dense units' grouped convolution: fast mode (k = 3) at the two ends of the network's range of maps (46^2 and 88^2
    # outputs), original mode (k = 5) on a map in between
    for k, side in ((3, 48), (3, 90), (5, 60)):
        variants, nbytes = {}, {}
        w32 = torch.randn((32, 32, k, k), device="cuda", generator=g) * 0.1
        for name, dtype in ALL:
            x = rand((n, 128, side, side), dtype)
            out = torch.empty((n, 32, side - k + 1, side - k + 1), dtype=dtype, device="cuda", memory_format=torch.channels_last)
            if dtype == torch.float32:
                wp = w32.view(4, 8, 32, k, k).permute(0, 3, 4, 2, 1).contiguous()
                variants[name] = lambda x=x, wp=wp, out=out, k=k: K.hip_grouped_conv_valid(x, wp, groups=4, kernel=k, out=out)
            else:
                wp = K.pack_grouped_conv_valid_weights_h(w32, 4, dtype)
                variants[name] = lambda x=x, wp=wp, out=out, k=k: K.hip_grouped_conv_valid_h(x, wp, groups=4, kernel=k, out=out)
            nbytes[name] = x.element_size() * (x.numel() + out.numel())
        add(f"grouped k{k}", f"{n}x{side}x{side}x128->32", nbytes, variants)
    # the dense units' pre-activation: a channel prefix of the feature buffer (u3: 256 + 32 i of 512 channels; u2: 128 + 32 i of 256)
    for c, ctot, side in ((256, 512, 48), (480, 512, 34), (128, 256, 88)):
        variants, nbytes = {}, {}
        for name, dtype in ALL:
            buf = rand((n, ctot, side, side), dtype)
            sc, sh = torch.rand(c, device="cuda", generator=g) + 0.5, torch.randn(c, device="cuda", generator=g)
            view = buf[:, :c, 1:side - 1, 1:side - 1]
            variants[name] = lambda v=view, sc=sc, sh=sh: K.hip_scale_shift_act_view(v, sc, sh)
            nbytes[name] = 2 * buf.element_size() * view.numel()
        add("view act", f"{n}x{side - 2}x{side - 2}x{c} of {ctot}", nbytes, variants)
    # conv3 + shortcut with the raw sum and the activated copy (d0: 64 -> 256 on 256^2; d2: 256 -> 1024 on 64^2)
    for cin, cout, side in ((64, 256, 256), (256, 1024, 64)):
        variants, nbytes = {}, {}
        conv = torch.nn.Conv2d(cin, cout, 1, bias=True).cuda()
        sc, sh = torch.rand(cout, device="cuda", generator=g) + 0.5, torch.randn(cout, device="cuda", generator=g)
        for name, dtype in ALL:
            x, res = rand((n, cin, side, side), dtype), rand((n, cout, side, side), dtype)
            bias = conv.bias.detach()
            if dtype == torch.float32:
                wp = K.pack_conv_weights(conv)
                variants[name] = lambda x=x, wp=wp, b=bias, r=res, sc=sc, sh=sh: K.hip_conv2d_post(
                    x, wp, b, r, kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False, post_scale=sc, post_shift=sh)
            else:
                wp = K.pack_conv_weights_h(conv, dtype)
                variants[name] = lambda x=x, wp=wp, b=bias, r=res, sc=sc, sh=sh, co=cout: K.hip_conv2d_h_ex(
                    x, wp, b, r, cout=co, kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False, post_scale=sc, post_shift=sh)
                variants[name + " y only"] = lambda x=x, wp=wp, b=bias, r=res, co=cout: K.hip_conv2d_h(
                    x, wp, b, r, cout=co, kernel=1, stride=1, padding=0, relu=False)
                nbytes[name + " y only"] = x.element_size() * (x.numel() + 2 * res.numel() + cin * cout)
            nbytes[name] = x.element_size() * (x.numel() + 3 * res.numel() + cin * cout)
        add("conv3+post", f"{n}x{side}x{side}x{cin}->{cout}", nbytes, variants)
    # the stem: float32 arithmetic in every dtype, the output map in the dtype
    conv = torch.nn.Conv2d(3, 64, 7).cuda()
    wp, bias = K.pack_thin_conv_weights(conv.weight), conv.bias.detach()
    xs = torch.rand((n, 3, 256, 256), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    variants, nbytes = {}, {}
    for name, dtype in ALL:
        variants[name] = lambda dtype=dtype: K.hip_conv2d_thin(xs, wp, bias, kernel=7, stride=1, pad_lo=3, pad_hi=3, relu=True, out_dtype=dtype)
        nbytes[name] = n * 256 * 256 * (12 + 64 * torch.empty((), dtype=dtype).element_size())
    add("stem 7x7", f"{n}x256x256x3", nbytes, variants)
    return rows


def engine_table(args) -> list[dict]:
    from tiatoolbox_amd.models.engine.nucleus_instance_segmentor import NucleusInstanceSegmentor
    from tiatoolbox_amd.utils import synth

    n = args.tiles
    host = synth.g_he(min(n, 64), 256, 256, seed=5)
    tiles = np.ascontiguousarray(np.tile(host, ((n + len(host) - 1) // len(host), 1, 1, 1))[:n])
    dtypes = ("float32", "float16", "bfloat16")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        engines = {d: NucleusInstanceSegmentor("hovernet_fast-pannuke", batch_size=args.batch, device="cuda", verbose=False) for d in dtypes}
    counts = {}

    def step(d):
        out = engines[d].run(tiles, patch_mode=True, compute_dtype=d)
        torch.cuda.synchronize()
        counts[d] = sum(len(b) for b in out["box"])

    for d in dtypes:
        step(d)  # lazy loads, weight packing
    times = {d: [] for d in dtypes}
    for _ in range(args.rounds):
        for d in dtypes:
            t0 = time.perf_counter()
            step(d)
            times[d].append(time.perf_counter() - t0)
    rows = []
    for d in dtypes:
        t = statistics.median(times[d])
        rows.append({"compute_dtype": d, "inference_copy": type(engines[d]._inference_model(  # noqa: SLF001
            {"float32": torch.float32, **HALVES}[d])).__name__, "tiles": n, "seconds": t, "min_s": min(times[d]), "max_s": max(times[d]),
            "tiles_per_s": n / t, "nuclei": counts[d]})
        print(f"engine {n} tiles compute_dtype={d:9s} {t:7.3f} s  [{min(times[d]):.3f} .. {max(times[d]):.3f}]  {n / t:7.1f} tiles/s  "
              f"{counts[d]} nuclei  ({rows[-1]['inference_copy']})", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--no-cast", action="store_true", help="skip the cast torch module (library convolutions)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_hovernet_half.py measures on a GPU; none is visible.")
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "rounds": args.rounds, "reps": args.reps}
    result["kernels"] = kernel_table(args)
    torch.cuda.empty_cache()
    result["forward"] = forward_table(args)
    torch.cuda.empty_cache()
    if not args.no_engine:
        result["engine"] = engine_table(args)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

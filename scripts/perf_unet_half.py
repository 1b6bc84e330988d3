"""The half-precision ``FusedUNet`` (``compute_dtype="float16" | "bfloat16"`` of ``SemanticSegmentor``) beside the float32
one and beside what the option ran before (the torch module cast to the dtype), all in ONE session, alternating:

1. whole forward (uint8 patches -> float32 logits) of seeded ``fcn_resnet50_unet-bcss`` on ``--batch`` x ``--side``^2 patches:
   (i) float32 ``FusedUNet`` under ``conv_algo="auto"``, (ii) half ``FusedUNet`` fp16 / bf16, (iii) ``copy.deepcopy(model).cuda().to(dtype)``;
2. the three glue kernels at the UNet's own shapes: time, algorithmic bytes, fraction of 8 TB/s, the float32 kernel beside it
   (upsample-add: 4.5 bytes per output element in half, 9 in float32; head: 2 * 64 + 4 * cout bytes per pixel, 4 * 64 + 4 * cout in
   float32; stem: 3 bytes per input pixel + both output maps);
3. ``SemanticSegmentor`` in WSI mode on the synthetic slide of ``bench_configs.bench_semantic`` (the same recipe: that function builds
   it inline), patches/s for float32 / float16 / bfloat16.

usage: perf_unet_half.py [--batch 16] [--side 1024] [--rounds 3] [--reps 3] [--slide 20000] [--no-wsi] [--no-cast] [--out FILE.json]
Times: HIP events on the launch stream around ``reps`` calls after a warm-up of every variant; variants alternate inside a round and
the figure reported is the median over rounds (min and max kept in the JSON)."""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tiatoolbox_amd.models.architecture import fused as K  # noqa: E402, N812

PEAK_BW = 8.0e12
HALVES = {"float16": torch.float16, "bfloat16": torch.bfloat16}


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
    from tiatoolbox_amd.models.architecture.hovernet_fused import set_conv_algo
    from tiatoolbox_amd.models.architecture.unet_fused import FusedUNet
    from tiatoolbox_amd.utils import synth

    model, _ = get_pretrained_model("fcn_resnet50_unet-bcss")
    model = model.eval()
    base = torch.from_numpy(synth.g_he(4, args.side, args.side, seed=9)).cuda()
    x = base.repeat(-(-args.batch // 4), 1, 1, 1)[:args.batch].contiguous()  # NHWC uint8
    imgs = x.permute(0, 3, 1, 2)
    variants = {}
    f32 = FusedUNet(copy.deepcopy(model).cuda()).cuda().to(memory_format=torch.channels_last).eval()
    set_conv_algo(f32, "winograd")  # what the engines' conv_algo="auto" selects
    variants["fused float32 (auto)"] = lambda: f32(imgs)
    for name, dtype in HALVES.items():
        half = FusedUNet(copy.deepcopy(model).cuda())
        half.prepare(dtype)
        half = half.to(dtype).to(memory_format=torch.channels_last).eval()
        variants[f"fused {name}"] = lambda m=half: m(imgs)
        if not args.no_cast:
            cast = copy.deepcopy(model).cuda().to(dtype).to(memory_format=torch.channels_last).eval()
            xin = imgs.to(dtype).contiguous(memory_format=torch.channels_last)
            variants[f"cast torch module {name}"] = lambda m=cast, xi=xin: m(xi).float()
    res = alternate(variants, args.rounds, args.reps)
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        print(f"forward {args.batch} x {args.side}^2  {name:28s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  "
              f"{r['patches_per_s']:8.1f} patches/s", flush=True)
    return res


def kernel_table(args) -> list[dict]:
    n, side = args.batch, args.side
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []

    def add(kernel, shape, nbytes, variants):
        res = alternate(variants, args.rounds, max(args.reps, 10))
        for name, r in res.items():
            row = {"kernel": kernel, "shape": shape, "variant": name, "ms": r["ms"], "min_ms": r["min_ms"], "max_ms": r["max_ms"],
                   "gbytes": nbytes[name] / 1e9, "tb_per_s": nbytes[name] / r["ms"] / 1e9, "fraction_of_8tbs": nbytes[name] / PEAK_BW / (r["ms"] * 1e-3)}
            rows.append(row)
            print(f"{kernel:13s} {shape:26s} {name:9s} {r['ms']:8.3f} ms  {row['gbytes']:7.3f} GB  {row['tb_per_s']:5.2f} TB/s  "
                  f"{100 * row['fraction_of_8tbs']:5.1f} % of 8 TB/s", flush=True)

    # upsample2x + skip + BN + ReLU: the four decoder stages (output map = side / 16 .. side / 2)
    for c, div in ((1024, 32), (512, 16), (256, 8), (64, 4)):
        h = side // div
        variants, nbytes = {}, {}
        for name, dtype in (("float32", torch.float32), *HALVES.items()):
            x = torch.randn((n, c, h, h), device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
            y = torch.randn((n, c, 2 * h, 2 * h), device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
            sc, sh = torch.rand(c, device="cuda", generator=g) + 0.5, torch.randn(c, device="cuda", generator=g)
            variants[name] = lambda x=x, y=y, sc=sc, sh=sh: K.hip_upsample2x_add(x, y, sc, sh)
            nbytes[name] = (2.25 * x.element_size()) * y.numel()  # y + out + x / 4 per output element: 9 / 4.5 bytes
        add("upsample_add", f"{n}x{2 * h}x{2 * h}x{c}", nbytes, variants)
    # the stem with its pre-pool map
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3).cuda()
    wp, bias = K.pack_stem_weights(conv), conv.bias.detach()
    xs = torch.randint(0, 256, (n, side, side, 3), device="cuda", generator=g, dtype=torch.uint8)
    variants, nbytes = {}, {}
    for name, dtype in (("float32", torch.float32), *HALVES.items()):
        variants[name] = lambda dtype=dtype: K.hip_stem_conv_pool(xs, wp, bias, out_dtype=dtype, return_conv=True)
        esz = torch.empty((), dtype=dtype).element_size()
        nbytes[name] = n * side * side * 3 + esz * n * 64 * ((side // 2) ** 2 + (side // 4) ** 2)
    add("stem+conv_out", f"{n}x{side}x{side}x3 u8", nbytes, variants)
    # the head: 64 -> 5 classes on the side / 2 map
    h = side // 2
    wgt, hb = torch.randn((5, 64), device="cuda", generator=g), torch.randn(5, device="cuda", generator=g)
    variants, nbytes = {}, {}
    for name, dtype in (("float32", torch.float32), *HALVES.items()):
        x = torch.randn((n, 64, h, h), device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
        variants[name] = lambda x=x: K.hip_conv1x1_head(x, wgt, hb)
        nbytes[name] = n * h * h * (x.element_size() * 64 + 4 * 5)
    add("head 64->5", f"{n}x{h}x{h}x64", nbytes, variants)
    return rows


def wsi_table(args) -> list[dict]:
    from tiatoolbox_amd.models.engine.semantic_segmentor import SemanticSegmentor
    from tiatoolbox_amd.utils import synth
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    side = args.slide
    # the slide of bench_configs.bench_semantic: a G-he tile mosaic on a bright background (20 % margin + gutters)
    tile = torch.from_numpy(synth.g_he(1, 2048, 2048, seed=3)[0]).cuda()
    slide = torch.full((side, side, 3), 243, dtype=torch.uint8, device="cuda")
    lo, hi = side // 10, side - side // 10
    for y in range(lo, hi, 2048 + 256):
        for x in range(lo, hi, 2048 + 256):
            h, w = min(2048, hi - y), min(2048, hi - x)
            slide[y:y + h, x:x + w] = tile[:h, :w]
    reader = ArrayWSIReader(slide, mpp=0.25, power=40.0)
    scratch = Path(tempfile.mkdtemp(prefix="tia_unet_half_", dir="/dev/shm" if Path("/dev/shm").is_dir() else None))
    dtypes = ("float32", "float16", "bfloat16")
    engines = {d: SemanticSegmentor("fcn_resnet50_unet-bcss", batch_size=args.batch, device="cuda", verbose=False) for d in dtypes}

    def step(d):
        engines[d].run([reader], patch_mode=False, save_dir=scratch / d, overwrite=True, compute_dtype=d)
        torch.cuda.synchronize()

    for d in dtypes:
        step(d)  # lazy loads, weight packing
    mask_reader = reader.tissue_mask(resolution=1.25, units="power")
    _, _, keep = engines["float32"].get_coordinates(reader, mask_reader)
    n_patches = int(keep.sum())
    times = {d: [] for d in dtypes}
    for _ in range(args.rounds):
        for d in dtypes:
            t0 = time.perf_counter()
            step(d)
            times[d].append(time.perf_counter() - t0)
    import shutil

    shutil.rmtree(scratch, ignore_errors=True)
    rows = []
    for d in dtypes:
        t = statistics.median(times[d])
        rows.append({"compute_dtype": d, "inference_copy": type(engines[d]._inference_model(  # noqa: SLF001
            {"float32": torch.float32, **HALVES}[d])).__name__, "slide": side, "patches": n_patches, "seconds": t, "min_s": min(times[d]),
            "max_s": max(times[d]), "patches_per_s": n_patches / t})
        print(f"WSI {side}^2 ({n_patches} patches) compute_dtype={d:9s} {t:7.3f} s  [{min(times[d]):.3f} .. {max(times[d]):.3f}]  "
              f"{n_patches / t:7.1f} patches/s  ({rows[-1]['inference_copy']})", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slide", type=int, default=20000)
    ap.add_argument("--no-wsi", action="store_true")
    ap.add_argument("--no-cast", action="store_true", help="skip the cast torch module (library convolutions)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_unet_half.py measures on a GPU; none is visible.")
    result = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "side": args.side, "rounds": args.rounds, "reps": args.reps}
    result["kernels"] = kernel_table(args)
    torch.cuda.empty_cache()
    result["forward"] = forward_table(args)
    torch.cuda.empty_cache()
    if not args.no_wsi:
        result["wsi"] = wsi_table(args)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

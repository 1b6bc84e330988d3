"""The grouped 3x3 convolution of ResNeXt (``tia_conv3x3_grouped_nhwc_f32``) per stage of resnext50_32x4d at 224^2 patches, against
its roofline bound and MIOpen's grouped convolution (``F.conv2d(..., groups=32)``, channels-last float32) on the same tensors; then
``PatchPredictor`` patches/s of the ResNet-family classifiers.

usage: perf_grouped_conv.py [--n 4096] [--out FILE.json] [--no-engine]
Bounds from shapes: flops = 2 * n * ho * wo * c * cg * 9; bytes = input + output (float32, each once); bound = max(flops / 157.3
TFLOP/s, bytes / 8.0 TB/s) (MI355X float32 vector / matrix peak and HBM peak).  Times: HIP events on the launch stream, mean of
10 launches after one warm-up."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F  # noqa: N812

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_grouped, pack_grouped_conv_weights  # noqa: E402

PEAK_FLOPS, PEAK_BW = 157.3e12, 8.0e12
# resnext50_32x4d conv2 shapes at 224^2: (stage, channels, input map, stride)
STAGES = [("layer1", 128, 56, 1), ("layer2", 256, 28, 1), ("layer3", 512, 14, 1), ("layer4", 1024, 7, 1),
          ("layer2.0", 256, 56, 2), ("layer3.0", 512, 28, 2), ("layer4.0", 1024, 14, 2)]
MODELS = ["resnet50-kather100k", "resnet101-kather100k", "resnext50_32x4d-kather100k", "resnext101_32x8d-kather100k",
          "wide_resnet50_2-kather100k", "wide_resnet101_2-kather100k"]


def ev(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(n: int) -> list[dict]:
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for stage, c, hw, stride in STAGES:
        cg = c // 32
        conv = torch.nn.Conv2d(c, c, 3, stride, 1, groups=32).cuda()
        x = torch.randn((n, c, hw, hw), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
        wp = pack_grouped_conv_weights(conv)
        ho = (hw - 1) // stride + 1
        flops = 2.0 * n * ho * ho * c * cg * 9
        nbytes = 4.0 * n * c * (hw * hw + ho * ho)
        bound_ms = max(flops / PEAK_FLOPS, nbytes / PEAK_BW) * 1e3
        t_hip = ev(lambda: hip_conv3x3_grouped(x, wp, conv.bias, stride=stride, relu=True))  # noqa: B023
        with torch.inference_mode():
            t_lib = ev(lambda: F.relu(F.conv2d(x, conv.weight, conv.bias, stride=stride, padding=1, groups=32)))  # noqa: B023
            t_lib_conv = ev(lambda: F.conv2d(x, conv.weight, conv.bias, stride=stride, padding=1, groups=32))  # noqa: B023
        row = {"stage": stage, "n": n, "c": c, "cg": cg, "map": hw, "stride": stride, "gflop": flops / 1e9, "gbytes": nbytes / 1e9,
               "intensity": flops / nbytes, "bound": "compute" if flops / PEAK_FLOPS > nbytes / PEAK_BW else "HBM",
               "bound_ms": bound_ms, "hip_ms": t_hip, "fraction_of_bound": bound_ms / t_hip, "hip_tflops": flops / t_hip / 1e9,
               "miopen_conv_relu_ms": t_lib, "miopen_conv_ms": t_lib_conv, "speedup_vs_miopen": t_lib / t_hip}
        rows.append(row)
        print(f"{stage:9s} c={c:5d} cg={cg:2d} {hw:2d}^2 s{stride}: hip {t_hip:8.3f} ms ({row['hip_tflops']:6.1f} TF/s, "
              f"{100 * row['fraction_of_bound']:5.1f} % of the {row['bound']} bound {bound_ms:.3f} ms) | MIOpen conv+relu {t_lib:8.3f} ms"
              f" (conv {t_lib_conv:.3f}) -> x{row['speedup_vs_miopen']:.2f}", flush=True)
        del x
        torch.cuda.empty_cache()
    return rows


def engines(n: int) -> list[dict]:
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.utils import synth

    base = torch.from_numpy(synth.g_he(64, 224, 224, seed=9)).cuda()
    x = base.repeat(n // 64, 1, 1, 1).contiguous()
    rows = []
    for name in MODELS:
        eng = PatchPredictor(name, batch_size=512, device="cuda", verbose=False)
        eng.run(x[:512], patch_mode=True, return_probabilities=True)  # builds and packs the inference copy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(x, patch_mode=True, return_probabilities=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rows.append({"model": name, "patches": n, "seconds": dt, "patches_per_s": n / dt})
        print(f"{name:30s} {n} x 224^2: {dt:7.3f} s  {n / dt:9.1f} patches/s", flush=True)
        del eng
        torch.cuda.empty_cache()
    ref = rows[0]["patches_per_s"]
    for r in rows:
        r["relative_to_resnet50"] = r["patches_per_s"] / ref
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "kernels": kernels(args.n)}
    if not args.no_engine:
        result["engines"] = engines(args.n)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

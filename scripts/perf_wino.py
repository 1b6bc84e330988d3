"""Winograd F(2x2, 3x3), F(4x2, 3x3) and the split-operand F(2x2, 3x3) (bf16 matrix cores) vs the direct tap-reuse kernel, per
3x3 / stride-1 layer of resnet18 at a batch and patch size, and the whole trunk; per form the best of three interleaved warmed-up rounds, their
spread, and the error of two images against a float64 convolution.  usage: perf_wino.py [batch=1024] [patch=256]  (HIP events on the launch stream; TFLOP/s are DIRECT-convolution flops / time,
i.e. 'effective' for the Winograd rows, whose executed MFMA flops are 16/36 (F(2x2)) and 24/72 (F(4x2)) of that -- printed as `exec`).
On maps of at most 8 x 8 the split column is the four-images-per-block geometry (W8), labelled so; with
``TIA_DEV=1 TIA_WINO_SPLIT_NO_W8=1`` in the environment it is the 16 x 16-block geometry on those rows as well."""
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tiatoolbox_amd.models.architecture.fused import (hip_conv2d, hip_conv3x3_wino, pack_conv_weights, pack_conv_weights_wino,
                                                      pack_conv_weights_wino42, pack_conv_weights_wino_split)


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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    patch = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    pmc = len(sys.argv) > 3 and sys.argv[3] == "pmc"
    g = torch.Generator(device="cuda").manual_seed(0)
    tot_d = tot_w = tot_4 = tot_s = 0.0
    for c, div, count in ((64, 4, 4), (128, 8, 3), (256, 16, 3), (512, 32, 3)):
        hw = patch // div
        w8 = hw <= 8 and not (os.environ.get("TIA_DEV", "")[:1] == "1" and "TIA_WINO_SPLIT_NO_W8" in os.environ)
        split_name = "split F(2x2) W8 (four images per block)" if w8 else "split F(2x2)"
        conv = torch.nn.Conv2d(c, c, 3, padding=1).cuda()
        x = torch.randn((n, c, hw, hw), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
        res = torch.randn_like(x)
        wp, up, u4, us = pack_conv_weights(conv), pack_conv_weights_wino(conv), pack_conv_weights_wino42(conv), pack_conv_weights_wino_split(conv)
        flops = 2.0 * n * hw * hw * c * c * 9
        f0 = lambda: hip_conv2d(x, wp, conv.bias, res, kernel=3, stride=1, padding=1, relu=True)  # noqa: E731
        f2 = lambda: hip_conv3x3_wino(x, up, conv.bias, res, padding=1, relu=True)  # noqa: E731
        f4 = lambda: hip_conv3x3_wino(x, u4, conv.bias, res, padding=1, relu=True)  # noqa: E731
        fs = lambda: hip_conv3x3_wino(x, us, conv.bias, res, padding=1, relu=True)  # noqa: E731
        if pmc:  # counter-pass workload: the 13 Winograd launches of exactly two forwards (see perf_trunk.py "pmc")
            for _ in range(2 * count):
                (f2 if len(sys.argv) > 4 and sys.argv[4] == "f22" else f4)()
            continue
        for _ in range(30):  # the clocks ramp up over the first tens of milliseconds of load: an unwarmed first column reads 5-10 % slow
            f0()             # (the "direct" column of profiles/r05b..r05o_perf_wino*.txt was measured without this and is pessimistic)
        rounds = [[ev(f) for f in (f0, f2, f4, fs)] for _ in range(3)]  # interleaved rounds, best of three
        td, tw, t4, ts = (min(r[k] for r in rounds) for k in range(4))
        sp = [100.0 * (max(r[k] for r in rounds) - min(r[k] for r in rounds)) / min(r[k] for r in rounds) for k in range(4)]
        a = hip_conv2d(x, wp, conv.bias, res, kernel=3, stride=1, padding=1, relu=False)
        b = hip_conv3x3_wino(x, up, conv.bias, res, padding=1, relu=False)
        b4 = hip_conv3x3_wino(x, u4, conv.bias, res, padding=1, relu=False)
        bs = hip_conv3x3_wino(x, us, conv.bias, res, padding=1, relu=False)
        rel = ((a - b).abs().max() / a.abs().max()).item()
        rel4 = ((a - b4).abs().max() / a.abs().max()).item()
        # two images against a float64 convolution on the host, relative to max |y|
        ref = (torch.nn.functional.conv2d(x[:2].double().cpu(), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), padding=1)
               + res[:2].double().cpu())
        e64 = [((t[:2].double().cpu() - ref).abs().max() / ref.abs().max()).item() for t in (b, b4, bs)]
        tot_d += td * count
        tot_w += tw * count
        tot_4 += t4 * count
        tot_s += ts * count
        print(f"3x3 {c:3d}->{c:3d} @{hw:3d} n={n}: direct {td:6.3f} ms {flops / td / 1e9:6.1f} TF/s | winograd {tw:6.3f} ms "
              f"{flops / tw / 1e9:6.1f} TF/s effective, {flops * 16 / 36 / tw / 1e9:6.1f} exec | x{td / tw:4.2f} | max rel diff {rel:.1e} || F(4x2) "
              f"{t4:6.3f} ms {flops / t4 / 1e9:6.1f} TF/s effective, {flops * 24 / 72 / t4 / 1e9:6.1f} exec | x{tw / t4:4.2f} vs F(2x2) | "
              f"max rel diff {rel4:.1e} || {split_name} {ts:6.3f} ms {flops / ts / 1e9:6.1f} TF/s effective | x{tw / ts:4.2f} vs F(2x2), x{t4 / ts:4.2f} vs F(4x2) | "
              f"spread of the rounds: direct {sp[0]:.1f} %, F(2x2) {sp[1]:.1f} %, F(4x2) {sp[2]:.1f} %, split {sp[3]:.1f} % | "
              f"error vs float64: F(2x2) {e64[0]:.1e}, F(4x2) {e64[1]:.1e}, split {e64[2]:.1e}", flush=True)
    if pmc:
        torch.cuda.synchronize()
        print("PMC forwards=2")
        return
    print(f"13 stride-1 3x3 launches of one resnet18 forward: direct {tot_d:.2f} ms, winograd F(2x2) {tot_w:.2f} ms (x{tot_d / tot_w:.2f}), "
          f"F(4x2) {tot_4:.2f} ms (x{tot_w / tot_4:.2f} vs F(2x2)), split F(2x2) {tot_s:.2f} ms")


if __name__ == "__main__":
    main()

"""The split-operand bf16 kernel (``tia_conv2d_bf16x3_nhwc_f32``) against the float32 ring kernel (``tia_conv2d_nhwc_f32``) on the same
tensors, per strided layer of resnet18 (3x3 / 2 and 1x1 / 2 of layers 2-4).  usage: perf_conv_split.py [batch=4096] [patch=256 224 ...]
HIP events on the launch stream, warmed up, three interleaved rounds (best, and the spread of the three); TFLOP/s are direct-convolution
flops / time; errors are max |y - float64| / max |y| on a sample of output pixels (torch float64 on the CPU)."""
import sys
from pathlib import Path

import torch
import torch.nn.functional as F  # noqa: N812

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tiatoolbox_amd import _lib
from tiatoolbox_amd.models.architecture.fused import hip_conv2d, hip_conv2d_split, pack_conv_weights, pack_conv_weights_split


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


def sample_error(x, conv, k, pad, ys, images=4):
    """max |y - float64 reference| / max |reference| over the first `images` images (the whole map of each), for each output in `ys`."""
    with torch.inference_mode():
        ref = F.conv2d(x[:images].double().cpu().contiguous(), conv.weight.double().cpu(), conv.bias.double().cpu(), 2, pad)
    return [((y[:images].double().cpu() - ref).abs().max() / ref.abs().max()).item() for y in ys]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    patches = [int(a) for a in sys.argv[2:]] or [256, 224]
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for patch in patches:
        tot_f = tot_s = 0.0
        for cin, div in ((64, 4), (128, 8), (256, 16)):
            hw, cout = patch // div, 2 * cin
            x = torch.relu(torch.randn((n, cin, hw, hw), device="cuda", generator=g)).contiguous(memory_format=torch.channels_last)
            for k, pad in ((3, 1), (1, 0)):
                conv = torch.nn.Conv2d(cin, cout, k, stride=2, padding=pad).cuda()
                ho = (hw + 2 * pad - k) // 2 + 1
                wp, w3 = pack_conv_weights(conv), pack_conv_weights_split(conv)
                route = lib.tia_conv2d_route_f32(n, hw, hw, cin, cout, k, k, 2, pad, pad, ho, ho)
                serves = lib.tia_conv2d_bf16x3_serves(n, hw, hw, cin, cout, k, k, 2, pad, pad, ho, ho)
                flops = 2.0 * n * ho * ho * cin * cout * k * k
                f0 = lambda: hip_conv2d(x, wp, conv.bias, None, kernel=k, stride=2, padding=pad, relu=True)  # noqa: E731, B023
                f1 = lambda: hip_conv2d_split(x, w3, conv.bias, None, kernel=k, stride=2, padding=pad, relu=True)  # noqa: E731, B023
                for _ in range(30):  # the clocks ramp up over the first tens of milliseconds of load
                    f0()
                rounds = [(ev(f0), ev(f1)) for _ in range(3)]
                tf, ts = min(r[0] for r in rounds), min(r[1] for r in rounds)
                sf, ss = max(r[0] for r in rounds) / tf - 1, max(r[1] for r in rounds) / ts - 1
                ef, es = sample_error(x, conv, k, pad, [hip_conv2d(x, wp, conv.bias, None, kernel=k, stride=2, padding=pad, relu=False),
                                                        hip_conv2d_split(x, w3, conv.bias, None, kernel=k, stride=2, padding=pad, relu=False)])
                if k == 3:  # noqa: PLR2004
                    tot_f += tf
                    tot_s += ts
                print(f"{k}x{k}/2 {cin:3d}->{cout:3d} @{hw:3d} n={n} (route {route}, serves {serves}): float32 ring {tf:6.3f} ms "
                      f"{flops / tf / 1e9:6.1f} TF/s (spread {sf * 100:4.1f} %) err {ef:.1e} | split {ts:6.3f} ms {flops / ts / 1e9:6.1f} TF/s "
                      f"(spread {ss * 100:4.1f} %) err {es:.1e} | x{tf / ts:4.2f}", flush=True)
        print(f"patch {patch}: the three 3x3 / 2 launches: float32 ring {tot_f:.2f} ms, split {tot_s:.2f} ms", flush=True)


if __name__ == "__main__":
    main()

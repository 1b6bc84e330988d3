"""The split-operand convolution on the bf16 matrix cores (``tia_conv2d_bf16x3_nhwc_f32``) on the GPU.

All kernel cases call ``hip_conv2d_split`` directly on small tensors.  The kernel's units are a 256-pixel tile, a 128-channel column
tile, a 16-channel slice and a two-stage ring; the shapes (19 x 13 maps, 3 / 5 images, 16 / 48 / 64 input and 128 / 256 output channels)
are the smallest that cross each of them.  The 1e-5 gate cannot see a lost ``lo`` plane (3e-6: the table of DESIGN 4.27), so the EXACT
cases -- results without a rounded sum, bit for bit -- are what pins the three planes of both operands, the mid x mid product and
the addressing.
"""

from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from _conv_split_cases import (GEOMETRIES, case_integers, case_mid_mid, case_power_of_two_activations, case_single_tap, packed_index)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TIA_EINVAL, TIA_ESIZE = -1, -3


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _split_conv(x: torch.Tensor, w: torch.Tensor, bias, residual, *, k: int, stride: int, pad: int, relu: bool) -> torch.Tensor:
    """``hip_conv2d_split`` of CPU NCHW tensors; the result back on the CPU."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv2d_split, pack_conv_weights_split

    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], k, stride=stride, padding=pad, bias=False)
    conv.weight = torch.nn.Parameter(w.clone(), requires_grad=False)
    w3 = pack_conv_weights_split(conv.cuda())
    assert w3 is not None
    y = hip_conv2d_split(_nhwc(x), w3, None if bias is None else bias.cuda(), None if residual is None else _nhwc(residual), kernel=k,
                         stride=stride, padding=pad, relu=relu)
    torch.cuda.synchronize()
    return y.cpu().contiguous()


def _float32_conv(x, w, bias, *, k, stride, pad):
    from tiatoolbox_amd.models.architecture.fused import hip_conv2d, pack_conv_weights

    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], k, stride=stride, padding=pad, bias=False)
    conv.weight = torch.nn.Parameter(w.clone(), requires_grad=False)
    return hip_conv2d(_nhwc(x), pack_conv_weights(conv.cuda()), None if bias is None else bias.cuda(), None, kernel=k, stride=stride,
                      padding=pad, relu=False).cpu().contiguous()


def _random_layer(n, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((n, cin, 19, 13), generator=g))
    w = torch.randn((cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5
    b = torch.randn((cout,), generator=g)
    return x, w, b


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_error_against_float64_is_within_the_summation_order_gate(geometry, n):
    """max |y - float64| <= 1e-5 max |y| (the gate of ``test_engine.py::test_winograd_conv_matches_torch_cpu_fp32``) for every channel
    combination; the float32 kernel's error on the same tensors is printed beside it where that entry takes the shape (cin % 32)."""
    k, stride, pad = geometry
    for cin in (16, 48, 64):
        for cout in (128, 256):
            x, w, b = _random_layer(n, cin, cout, k, seed=n * 1000 + cin + cout + 7 * k + stride + pad)
            ref = F.conv2d(x.double(), w.double(), b.double(), stride, pad)
            got = _split_conv(x, w, b, None, k=k, stride=stride, pad=pad, relu=False)
            assert got.shape == ref.shape
            err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
            beside = ""
            if cin % 32 == 0:
                e32 = ((_float32_conv(x, w, b, k=k, stride=stride, pad=pad).double() - ref).abs().max() / ref.abs().max()).item()
                beside = f"; float32 kernel {e32:.2e}"
            print(f"{k}x{k}/{stride} pad {pad} n={n} {cin}->{cout}: split {err:.2e}{beside}")
            assert err <= 1e-5, (cin, cout, err)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_every_epilogue_combination(with_bias, with_residual, relu):
    x, w, b = _random_layer(5, 48, 256, 3, seed=77)
    ref = F.conv2d(x.double(), w.double(), b.double() if with_bias else None, 2, 1)
    res = torch.randn(ref.shape, generator=torch.Generator().manual_seed(78)) if with_residual else None
    if with_residual:
        ref = ref + res.double()
    if relu:
        ref = torch.relu(ref)
    got = _split_conv(x, w, b if with_bias else None, res, k=3, stride=2, pad=1, relu=relu)
    err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
    assert err <= 1e-5, err
    if relu:
        assert got.min() >= 0 and (got == 0).any()


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_exact_single_tap_weights_return_the_shifted_input(geometry):
    """(i) every tap position, stride and padding column; all three activation planes (random 24-bit significands)."""
    k, stride, pad = geometry
    x, w, ref = case_single_tap(k, stride, pad)
    got = _split_conv(x, w, None, None, k=k, stride=stride, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_exact_power_of_two_activations_return_the_scaled_weight(geometry):
    """(ii) all three weight planes."""
    k, stride, pad = geometry
    x, w, ref = case_power_of_two_activations(k, stride, pad)
    got = _split_conv(x, w, None, None, k=k, stride=stride, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@pytest.mark.parametrize("geometry", [GEOMETRIES[0], GEOMETRIES[2], GEOMETRIES[4]])
def test_exact_mid_times_mid(geometry):
    """(iii) (1 + 2^-10)^2 = 1 + 2^-9 + 2^-20."""
    k, stride, pad = geometry
    x, w, ref = case_mid_mid(k, stride, pad)
    got = _split_conv(x, w, None, None, k=k, stride=stride, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


def test_exact_integer_accumulation():
    """(iv) integer operands, every partial sum below 2^24: integer arithmetic across taps, slices and padding."""
    x, w, ref = case_integers()
    got = _split_conv(x, w, None, None, k=3, stride=2, pad=1, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


def _reads(shape, k, stride, pad, positions) -> torch.Tensor:
    """Boolean [n, 1, ho, wo]: the outputs whose window contains one of the input ``positions`` (image, row, column)."""
    mark = torch.zeros((shape[0], 1, shape[2], shape[3]), dtype=torch.float64)
    for b, yy, xx in positions:
        mark[b, 0, yy, xx] = 1
    return F.conv2d(mark, torch.ones((1, 1, k, k), dtype=torch.float64), None, stride, pad) > 0


def test_non_finite_and_overflowing_activations_never_give_a_finite_wrong_value():
    """One NaN, one +inf and one activation whose leading part overflows (3.4e38: bf16 rounds it to infinity): every output that
    reads one of them is non-finite, every other output is bit for bit the clean run's.  3.39e38 lies between the largest bf16
    number 2^127 (2 - 2^-7) = 3.3895e38 and the rounding boundary 2^127 (2 - 2^-8) = 3.3961e38: its leading part is FINITE, the
    split exact, and its outputs are the correct (finite or overflowed) float32 values -- checked against float64."""
    k, stride, pad = 3, 2, 1
    x, w, b = _random_layer(5, 48, 128, k, seed=5)
    clean = _split_conv(x, w, b, None, k=k, stride=stride, pad=pad, relu=False)
    bad = {(0, 3, 4, 7): float("nan"), (1, 20, 0, 0): float("inf"), (4, 47, 18, 12): 3.4e38}
    xb = x.clone()
    for (bi, c, yy, xx), v in bad.items():
        xb[bi, c, yy, xx] = v
    got = _split_conv(xb, w, b, None, k=k, stride=stride, pad=pad, relu=False)
    reads = _reads(x.shape, k, stride, pad, [(bi, yy, xx) for bi, _, yy, xx in bad]).expand_as(got)
    assert reads.any() and not reads.all()
    assert not torch.isfinite(got[reads]).any()
    assert torch.equal(got[~reads], clean[~reads])
    # 3.39e38
    xh = x.clone()
    xh[2, 9, 6, 6] = 3.39e38
    got = _split_conv(xh, w, b, None, k=k, stride=stride, pad=pad, relu=False)
    reads = _reads(x.shape, k, stride, pad, [(2, 6, 6)]).expand_as(got)
    ref = F.conv2d(xh.double(), w.double(), b.double(), stride, pad)
    assert torch.equal(got[~reads], clean[~reads])
    over = ref.abs() > torch.finfo(torch.float32).max
    assert not torch.isfinite(got[reads & over]).any()
    sel = reads & ~over
    assert bool(((got[sel].double() - ref[sel]).abs() <= 1e-5 * ref[sel].abs().max()).all())


def test_denormal_activations_cost_at_most_their_flushed_products():
    """Image 0 holds only denormal activations (parts below the bf16 normal range may be flushed): its outputs are within
    2^-126 sum |w| of the clean run (the same batch with zeros in their place); the other images are unchanged."""
    k, stride, pad = 3, 2, 1
    x, w, _ = _random_layer(3, 48, 128, k, seed=9)
    xc = x.clone()
    xc[0] = 0
    xd = xc.clone()
    g = torch.Generator().manual_seed(10)
    xd[0] = (torch.rand(x[0].shape, generator=g) - 0.5) * 2.0 ** -127
    assert (xd[0].abs() < 2.0 ** -126).all() and (xd[0] != 0).any()
    clean = _split_conv(xc, w, None, None, k=k, stride=stride, pad=pad, relu=False)
    got = _split_conv(xd, w, None, None, k=k, stride=stride, pad=pad, relu=False)
    bound = 2.0 ** -126 * w.double().abs().sum((1, 2, 3)).view(1, -1, 1, 1)
    assert bool(((got.double() - clean.double()).abs() <= bound).all())
    assert torch.equal(got[1:], clean[1:])


def test_packed_layout_matches_the_restatement():
    from tiatoolbox_amd.models.architecture.fused import pack_conv_weights_split, split_stem_weights

    conv = torch.nn.Conv2d(48, 256, 3, stride=2, padding=1).cuda()
    packed = pack_conv_weights_split(conv)
    parts = split_stem_weights(conv.weight.detach())[0].cpu()
    expect = parts.reshape(-1)[packed_index(256, 48, 3, 3).reshape(-1)].reshape(packed.shape)
    assert packed.dtype == torch.bfloat16 and torch.equal(packed.cpu().float(), expect)


def test_argument_checks_return_the_float32_entrys_codes_and_launch_nothing():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    stream = _lib.current_stream()
    x = torch.randn((2, 16, 16, 64), device="cuda")  # NHWC memory, more than any case below reads
    w3 = torch.zeros((9 * 64 * 128 * 3,), dtype=torch.bfloat16, device="cuda")
    y = torch.full((2 * 8 * 8 * 128,), 7.0, device="cuda")

    def split(xp, wp, yp, cin, cout):
        return lib.tia_conv2d_bf16x3_nhwc_f32(xp, wp, 0, 0, yp, 2, 16, 16, cin, cout, 3, 3, 2, 1, 1, 0, stream)

    def plain(xp, wp, yp, cin, cout):
        return lib.tia_conv2d_nhwc_f32(xp, wp, 0, 0, yp, 2, 16, 16, cin, cout, 3, 3, 2, 1, 0, stream)

    assert split(x.data_ptr(), w3.data_ptr(), y.data_ptr(), 24, 128) == TIA_ESIZE == plain(x.data_ptr(), w3.data_ptr(), y.data_ptr(), 24, 128)
    assert split(x.data_ptr(), w3.data_ptr(), y.data_ptr(), 64, 64) == TIA_ESIZE  # (the float32 entry's code for its own multiples)
    for args in ((0, w3.data_ptr(), y.data_ptr()), (x.data_ptr(), 0, y.data_ptr()), (x.data_ptr(), w3.data_ptr(), 0),
                 (x.data_ptr() + 4, w3.data_ptr(), y.data_ptr())):
        assert split(*args, 64, 128) == TIA_EINVAL == plain(*args, 64, 128), args
    assert split(x.data_ptr(), w3.data_ptr(), y.data_ptr(), 64, 128) == 0  # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert lib.tia_conv_pack_weights_bf16x3(x.data_ptr(), 64, 64, 3, 3, w3.data_ptr(), stream) == TIA_ESIZE
    assert lib.tia_conv_pack_weights_bf16x3(0, 128, 64, 3, 3, w3.data_ptr(), stream) == TIA_EINVAL


def test_rejected_calls_leave_the_output_untouched():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    x = torch.randn((2, 16, 16, 64), device="cuda")
    w3 = torch.zeros((9 * 64 * 128 * 3,), dtype=torch.bfloat16, device="cuda")
    y = torch.full((2 * 8 * 8 * 128,), 7.0, device="cuda")
    for xp, cin, cout in ((x.data_ptr(), 24, 128), (x.data_ptr(), 64, 64), (x.data_ptr() + 4, 64, 128), (0, 64, 128)):
        assert lib.tia_conv2d_bf16x3_nhwc_f32(xp, w3.data_ptr(), 0, 0, y.data_ptr(), 2, 16, 16, cin, cout, 3, 3, 2, 1, 1, 0, _lib.current_stream()) < 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_a_batch_beyond_two_gib_runs_in_groups_bit_identical_to_its_halves():
    """n x 64 x 64 x 64 float32 is 1 MiB per image: 2049 images are just over 2 GiB and run as 1025 + 1024 (equal groups); 1x1 / 2."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv2d_split, pack_conv_weights_split

    n = 2049
    conv = torch.nn.Conv2d(64, 128, 1, stride=2).cuda()
    w3 = pack_conv_weights_split(conv)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((n, 64, 64, 64), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    assert x.numel() * 4 > 2 ** 31
    y = hip_conv2d_split(x, w3, conv.bias, None, kernel=1, stride=2, padding=0, relu=True)
    cut = 1025
    for part in (slice(0, cut), slice(cut, n)):  # (one half at a time: under 4 GB in all)
        half = hip_conv2d_split(x[part], w3, conv.bias, None, kernel=1, stride=2, padding=0, relu=True)
        assert torch.equal(y[part], half)
        del half
    assert bool((y[-1] != 0).any()) and bool(torch.isfinite(y).all())


# ---- routing ------------------------------------------------------------------------------------------------------------------------
def _resnet18_layers(patch: int):
    """(map side, cin, cout, kernel, stride, padding) of every block convolution of resnet18 on ``patch``-sized inputs."""
    layers, side, c = [], patch // 4, 64
    for stage in range(4):
        cout = 64 << stage
        if stage:
            layers += [(side, c, cout, 3, 2, 1), (side, c, cout, 1, 2, 0)]
            side //= 2
        else:
            layers += [(side, c, cout, 3, 1, 1)]
        layers += [(side, cout, cout, 3, 1, 1)] * 3
        c = cout
    return layers


def _serves(lib, n, side, cin, cout, k, stride, pad) -> int:
    ho = (side + 2 * pad - k) // stride + 1
    return lib.tia_conv2d_bf16x3_serves(n, side, side, cin, cout, k, k, stride, pad, pad, ho, ho)


# the layers DESIGN 4.27's table admits at 4096 x 256^2: the three 3x3 / stride-2 convolutions and the three 1x1 / stride-2 projections
ADMITTED_256 = [(64, 64, 128, 3, 2, 1), (64, 64, 128, 1, 2, 0), (32, 128, 256, 3, 2, 1), (32, 128, 256, 1, 2, 0), (16, 256, 512, 3, 2, 1),
                (16, 256, 512, 1, 2, 0)]


def test_route_query_names_the_measured_layers_only():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    assert all(_serves(lib, 8, *layer) == 0 for layer in _resnet18_layers(224))
    took = [layer for layer in dict.fromkeys(_resnet18_layers(256)) if _serves(lib, 4096, *layer) == 1]
    assert took == ADMITTED_256, took
    # the developer switch, read once per process: a fresh child
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from tiatoolbox_amd import _lib; lib = _lib.load(); "
            "print(lib.tia_conv2d_bf16x3_serves(4096, 64, 64, 64, 128, 3, 3, 2, 1, 1, 32, 32))")
    for env, expect in (({"TIA_DEV": "1", "TIA_CONV_NO_SPLIT": "1"}, "0"), ({"TIA_CONV_NO_SPLIT": "1"}, "1")):
        out = subprocess.run([sys.executable, "-c", code, str(ROOT)], env={**os.environ, **env}, check=True, capture_output=True, text=True)
        assert out.stdout.strip() == expect, (env, out.stdout, out.stderr)


def test_engine_takes_the_split_kernel_under_auto_only():
    """The smallest batch of 128 x 128 patches for which the query takes layer 2's strided 3x3 (asked, not hard-coded): a
    ``PatchPredictor`` run of that batch launches ``conv_ring_bf16x3_kernel`` under ``auto`` and not under ``direct``; probabilities
    within 1e-5, equal predictions."""
    from torch.profiler import ProfilerActivity, profile

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.utils import synth

    lib = _lib.load()
    batch = next((n for n in range(8, 4097, 4) if _serves(lib, n, 32, 64, 128, 3, 2, 1) == 1), None)
    assert batch is not None
    print("smallest batch of 128 x 128 patches on the split kernel:", batch)
    patches = synth.g_he(batch, 128, 128, seed=31)
    eng = PatchPredictor("resnet18-kather100k", batch_size=batch, device="cuda", verbose=False)
    eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(128, 128))  # builds the inference copy
    outs, seen = {}, {}
    for algo in ("auto", "direct"):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            outs[algo] = eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(128, 128), conv_algo=algo)
            torch.cuda.synchronize()
        seen[algo] = any("conv_ring_bf16x3_kernel" in e.name for e in prof.events())
    assert seen == {"auto": True, "direct": False}, seen
    dp = np.abs(np.asarray(outs["auto"]["probabilities"], np.float64) - np.asarray(outs["direct"]["probabilities"], np.float64)).max()
    print(f"max |auto - direct| probability = {dp:.3e}")
    assert dp <= 1e-5, dp
    assert np.array_equal(outs["auto"]["predictions"], outs["direct"]["predictions"])

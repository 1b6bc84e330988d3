"""The four-images-per-block geometry (W8) of the split-operand Winograd F(2x2, 3x3) kernel (``conv3x3_wino_bf16x3_kernel<W8, ..>``,
DESIGN 4.40): ``tia_conv3x3_wino_bf16x3_nhwc_f32`` takes it by itself for maps of at most 8 x 8 outputs.

Its units are a block of four images, a 64-channel column block, a 16-channel slice and two patch buffers; the shapes are the smallest
that cross each of them: 8 x 8 (a full block), 7 x 7, 5 x 8 and 4 x 4 maps (dead pixels inside every image of the block); 5 and 8 images
(three dead images in the last block | two full blocks); 16 / 32 / 48 input channels (one, two, three slices; the persistent form needs
an even count); 64 / 128 output channels.  The per-output operation order is that of the 16 x 16-block geometry, so the two must agree
bit for bit; the other geometry, and the other launch form, come from a fresh child process with the developer switch (read once per
process).  The route test needs no device.
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

from _wino_split_cases import case_integers, case_isolated_activations, case_isolated_powers_of_two, case_mid_mid

gpu = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

MAPS = ((8, 8), (7, 7), (5, 8), (4, 4))
LAYERS = ((5, 16, 64), (8, 32, 128), (5, 48, 128), (8, 48, 64))  # (n, cin, cout)


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _wino(x, w, bias, residual, *, pad: int, relu: bool) -> torch.Tensor:
    """``hip_conv3x3_wino`` of CPU NCHW tensors through the split form; the result back on the CPU."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_wino, pack_conv_weights_wino_split

    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, padding=pad, bias=False)
    conv.weight = torch.nn.Parameter(w.clone(), requires_grad=False)
    u = pack_conv_weights_wino_split(conv.cuda())
    assert u is not None and u.dtype == torch.bfloat16
    y = hip_conv3x3_wino(_nhwc(x), u, None if bias is None else bias.cuda(), None if residual is None else _nhwc(residual), padding=pad,
                         relu=relu)
    torch.cuda.synchronize()
    return y.cpu().contiguous()


def _random_layer(n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((n, cin, h, w), generator=g))
    wt = torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5
    return x, wt, torch.randn((cout,), generator=g)


@gpu
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("hw", MAPS)
def test_error_against_float64_is_within_the_summation_order_gate(hw, pad):
    """max |y - float64| <= 1e-5 max |y| (the gate of test_wino_split_gpu.py) for every layer of LAYERS.  (Padding 2 makes the output
    two pixels larger than the input: the 4 x 4 map stays on this geometry, the others cross to 16 x 16 blocks.)"""
    h, w = hw
    for n, cin, cout in LAYERS:
        x, wt, b = _random_layer(n, cin, cout, h, w, seed=1000 * n + cin + cout + 7 * h + w + pad)
        ref = F.conv2d(x.double(), wt.double(), b.double(), 1, pad)
        got = _wino(x, wt, b, None, pad=pad, relu=False)
        assert got.shape == ref.shape
        err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
        print(f"{h}x{w} pad {pad} n={n} {cin}->{cout}: split {err:.2e}")
        assert err <= 1e-5, (n, cin, cout, err)


@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_every_epilogue_combination(with_bias, with_residual, relu):
    x, wt, b = _random_layer(5, 48, 128, 7, 7, seed=77)
    ref = F.conv2d(x.double(), wt.double(), b.double() if with_bias else None, 1, 1)
    res = torch.randn(ref.shape, generator=torch.Generator().manual_seed(78)) if with_residual else None
    if with_residual:
        ref = ref + res.double()
    if relu:
        ref = torch.relu(ref)
    got = _wino(x, wt, b if with_bias else None, res, pad=1, relu=relu)
    err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
    assert err <= 1e-5, err
    if relu:
        assert got.min() >= 0 and (got == 0).any()


# argv: repository root, output file, then cases "n,cin,cout,h,w,pad" -- every case with bias, residual and ReLU, tensors from seeds
_CASES_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import torch
from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_wino, pack_conv_weights_wino_split
outs = []
for k, case in enumerate(sys.argv[3:]):
    n, cin, cout, h, w, pad = (int(v) for v in case.split(","))
    g = torch.Generator().manual_seed(900 + k)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=pad)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (9 * cin) ** 0.5)
        conv.bias.copy_(torch.randn((cout,), generator=g))
    conv = conv.cuda()
    x = torch.randn((n, cin, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last)
    res = torch.randn((n, cout, h + 2 * pad - 2, w + 2 * pad - 2), generator=g).cuda().contiguous(memory_format=torch.channels_last)
    y = hip_conv3x3_wino(x, pack_conv_weights_wino_split(conv), conv.bias, res, padding=pad, relu=True)
    torch.cuda.synchronize()
    outs.append(y.cpu())
torch.save(outs, sys.argv[2])
"""


def _run_cases(path: Path, cases, env: dict) -> list[torch.Tensor]:
    args = [",".join(str(v) for v in c) for c in cases]
    subprocess.run([sys.executable, "-c", _CASES_CHILD, str(ROOT), str(path), *args], env={**os.environ, **env}, check=True)
    return torch.load(path)


@gpu
def test_four_image_blocks_are_bit_identical_to_16x16_blocks(tmp_path):
    """The same tensors through this geometry and, in a fresh child with ``TIA_DEV=1 TIA_WINO_SPLIT_NO_W8=1``, through 16 x 16 blocks."""
    cases = [(n, cin, cout, h, w, 1) for (h, w), (n, cin, cout) in zip(MAPS, LAYERS)]
    cases += [(5, 32, 128, 8, 8, 0), (5, 48, 64, 4, 4, 2), (8, 16, 128, 7, 7, 1)]
    four = _run_cases(tmp_path / "w8.pt", cases, {})
    blocks = _run_cases(tmp_path / "w16.pt", cases, {"TIA_DEV": "1", "TIA_WINO_SPLIT_NO_W8": "1"})
    for case, a, b in zip(cases, four, blocks):
        n, _, cout, h, w, pad = case
        assert a.shape == (n, cout, h + 2 * pad - 2, w + 2 * pad - 2) and bool((a != 0).any()), case
        assert torch.equal(a, b), (case, (a - b).abs().max().item())


@gpu
def test_persistent_form_is_bit_identical_to_one_block_per_workgroup(tmp_path):
    """The smallest launches ``wino_grid`` makes persistent at 128 output channels and two slices (pixel blocks x 2 >= 2 x compute
    units, asked of the device), one with a batch that is no multiple of four, against ``TIA_DEV=1 TIA_WINO_NO_PERSIST=1`` in a child."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
    cases = [(4 * cus, 32, 128, 8, 8, 1), (4 * cus + 1, 32, 128, 7, 7, 1)]
    for n, _, cout, _, _, _ in cases:
        assert ((n + 3) // 4) * (cout // 64) >= 2 * cus
    persist = _run_cases(tmp_path / "persist.pt", cases, {})
    blocks = _run_cases(tmp_path / "blocks.pt", cases, {"TIA_DEV": "1", "TIA_WINO_NO_PERSIST": "1"})
    for case, a, b in zip(cases, persist, blocks):
        assert a.shape[0] == case[0] and bool((a != 0).any()), case
        assert torch.equal(a, b), (case, (a - b).abs().max().item())


def _side(pad: int) -> int:
    return 8 if pad < 2 else 6  # (8 x 8 outputs at padding 2 as well)


@gpu
@pytest.mark.parametrize("pad", [0, 1, 2])
def test_exact_isolated_activations_through_all_sixteen_positions(pad):
    x, wt, ref = case_isolated_activations(pad, n=5, h=_side(pad), w=_side(pad))
    got = _wino(x, wt, None, None, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@gpu
@pytest.mark.parametrize("pad", [0, 1, 2])
def test_exact_isolated_powers_of_two_return_the_weights(pad):
    x, wt, ref = case_isolated_powers_of_two(pad, n=5, h=_side(pad), w=_side(pad))
    got = _wino(x, wt, None, None, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@gpu
@pytest.mark.parametrize("pad", [0, 1])
def test_exact_mid_times_mid(pad):
    x, wt, ref = case_mid_mid(pad, n=5, h=8, w=8)
    got = _wino(x, wt, None, None, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@gpu
def test_exact_integer_accumulation():
    x, wt, ref = case_integers(n=5, h=8, w=8)
    got = _wino(x, wt, None, None, pad=1, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@gpu
def test_non_finite_and_overflowing_activations_stay_in_their_image():
    """One NaN, one +inf and one 3.4e38 (bf16 rounds its leading part to infinity) in images 0 and 1 of the first block and in the
    last block's only live image: every output that reads one of them is non-finite, every other output -- the rest of those images
    and ALL of images 2 and 3, which share a block with two of them -- is bit for bit the clean run's."""
    pad = 1
    x, wt, b = _random_layer(5, 48, 128, 8, 8, seed=5)
    clean = _wino(x, wt, b, None, pad=pad, relu=False)
    bad = {(0, 3, 4, 7): float("nan"), (1, 20, 0, 0): float("inf"), (4, 47, 7, 6): 3.4e38}
    xb = x.clone()
    for (bi, c, yy, xx), v in bad.items():
        xb[bi, c, yy, xx] = v
    got = _wino(xb, wt, b, None, pad=pad, relu=False)
    mark = torch.zeros((5, 1, 8, 8), dtype=torch.float64)
    for bi, _, yy, xx in bad:
        mark[bi, 0, yy, xx] = 1
    reads = (F.conv2d(mark, torch.ones((1, 1, 3, 3), dtype=torch.float64), None, 1, pad) > 0).expand_as(got)
    assert reads.any() and not reads.all()
    assert not torch.isfinite(got[reads]).any()
    assert torch.equal(got[~reads], clean[~reads])
    assert torch.equal(got[2:4], clean[2:4]) and bool(torch.isfinite(clean).all())


def test_route_query():
    """``tia_conv3x3_wino_bf16x3_form`` (host only): 2 for layer 4 of 256 x 256 patches at the headline batch (the class is admitted:
    DESIGN 4.40 item 4), 1 for the three classes on 16 x 16 blocks, 0 for the neighbours -- the 7 x 7 maps of 224 x 224 patches among
    them, measured and not admitted -- and under ``TIA_WINO_NO_SPLIT``; the older query answers as before."""
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    form, serves = lib.tia_conv3x3_wino_bf16x3_form, lib.tia_conv3x3_wino_bf16x3_serves
    layer4 = (4096, 8, 8, 512, 512, 1)
    assert form(*layer4) == 2  # noqa: PLR2004
    assert serves(*layer4) == 0
    for hw, c in ((64, 64), (32, 128), (16, 256)):
        assert form(4096, hw, hw, c, c, 1) == 1 and serves(4096, hw, hw, c, c, 1) == 1
    for args in ((4096, 8, 8, 256, 256, 1), (4096, 4, 4, 512, 512, 1), (4096, 8, 16, 512, 512, 1), (4096, 8, 8, 256, 512, 1),
                 (4096, 8, 8, 512, 256, 1), (16, 8, 8, 512, 512, 1), (4096, 7, 7, 512, 512, 1), (4096, 8, 8, 512, 512, 0)):
        assert form(*args) == 0 and serves(*args) == 0, args
    assert form(4096, 8, 8, 500, 512, 1) == serves(4096, 8, 8, 500, 512, 1) < 0
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from tiatoolbox_amd import _lib; l = _lib.load(); "
            "print(l.tia_conv3x3_wino_bf16x3_form(4096, 8, 8, 512, 512, 1), l.tia_conv3x3_wino_bf16x3_form(4096, 64, 64, 64, 64, 1))")
    for env, expect in (({"TIA_DEV": "1", "TIA_WINO_NO_SPLIT": "1"}, "0 0"),
                        ({"TIA_DEV": "1", "TIA_WINO_SPLIT_NO_W8": "1"}, "0 1"),
                        ({"TIA_WINO_NO_SPLIT": "1"}, "2 1")):  # (without TIA_DEV the switch is not read)
        base = {k: v for k, v in os.environ.items() if k != "TIA_DEV"}
        out = subprocess.run([sys.executable, "-c", code, str(ROOT)], env={**base, **env}, check=True, capture_output=True, text=True)
        assert out.stdout.split("\n")[0].strip() == expect, (env, out.stdout)


@gpu
def test_engine_takes_the_four_image_form_under_auto_only():
    """The smallest batch of 256 x 256 patches for which the query takes layer 4 on this geometry (asked, not hard-coded): a
    ``PatchPredictor`` run of that batch launches the W8 split kernel under ``auto`` and not under ``direct``; probabilities within
    1e-5, equal predictions."""
    from torch.profiler import ProfilerActivity, profile

    from tiatoolbox_amd.models.architecture.fused import wino_split_form
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.utils import synth

    batch = next((n for n in range(4, 4097, 4) if wino_split_form(n, 8, 8, 512, 512, 1) == 2), None)  # noqa: PLR2004
    assert batch is not None
    print("batch of 256 x 256 patches:", batch)
    patches = synth.g_he(batch, 256, 256, seed=31)
    eng = PatchPredictor("resnet18-kather100k", batch_size=batch, device="cuda", verbose=False)
    eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(256, 256))  # builds the inference copy
    outs, names = {}, {}
    for algo in ("auto", "direct"):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            outs[algo] = eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(256, 256), conv_algo=algo)
            torch.cuda.synchronize()
        names[algo] = {e.name for e in prof.events()}

    def w8_split(name: str) -> bool:
        return "conv3x3_wino_bf16x3_kernel" in name and "W8" in name

    assert not any(w8_split(k) or "conv3x3_wino42_kernel" in k for k in names["direct"])
    assert any(w8_split(k) for k in names["auto"]), sorted(k for k in names["auto"] if "wino" in k)
    dp = np.abs(np.asarray(outs["auto"]["probabilities"], np.float64) - np.asarray(outs["direct"]["probabilities"], np.float64)).max()
    print(f"max |auto - direct| probability = {dp:.3e}")
    assert dp <= 1e-5, dp
    assert np.array_equal(outs["auto"]["predictions"], outs["direct"]["predictions"])

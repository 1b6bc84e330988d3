"""Host checks of the split-operand Winograd F(2x2, 3x3) form (``tia_conv3x3_wino_bf16x3_nhwc_f32``): the arithmetic
(an emulation of the kernel's order against float64), the size of the dropped terms, the packed layout, the refusal of weights without
a usable split, and the route query.  No GPU."""

from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from _wino_split_cases import (case_integers, case_isolated_activations, case_isolated_powers_of_two, case_mid_mid, dropped_terms_bound,
                               emulate_conv, packed_index)

ROOT = Path(__file__).resolve().parent.parent
TIA_EINVAL, TIA_ESIZE = -1, -3


def _layer(n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn((n, cin, h, w), generator=g)), torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5


@pytest.mark.parametrize(("cin", "n", "hw"), [(16, 2, 12), (64, 2, 12), (512, 1, 8)])
def test_emulated_order_is_within_the_gate_of_float64(cin, n, hw):
    """V in float32, six products per 16-channel step into one float32 accumulator, output transform in float32: against a float64
    convolution, relative to max |y|; the gate of every ``auto`` path is 1e-5.  The float32 Winograd emulation's figure beside it."""
    x, w = _layer(n, cin, 64, hw, hw, seed=cin)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    err = ((emulate_conv(x, w, 1).double() - ref).abs().max() / ref.abs().max()).item()
    e32 = ((emulate_conv(x, w, 1, split=False).double() - ref).abs().max() / ref.abs().max()).item()
    print(f"cin {cin}: split Winograd {err:.2e}, float32 Winograd {e32:.2e}")
    assert err <= 1e-5, err


def test_dropped_terms_are_below_one_float32_ulp_of_the_products():
    """mid lo + lo mid + lo lo <= 2^-23 sum |V| |U|, element by element, at every position."""
    x, w = _layer(2, 64, 64, 10, 10, seed=3)
    for lost, bound in dropped_terms_bound(x, w, 1):
        assert bool((lost <= bound).all())
        assert bool((lost > 0).any())


def test_exact_cases_hold_in_the_emulation():
    """The builders assert their exactness bound themselves; the emulation of the kernel's order returns the float64 result bit for bit."""
    for pad, (x, w, ref) in ((1, case_isolated_activations(1, n=2)), (0, case_isolated_powers_of_two(0, n=2)), (2, case_mid_mid(2, n=1)),
                             (1, case_integers(1, n=1))):
        assert torch.equal(emulate_conv(x, w, pad), ref), pad


def test_packed_layout_is_a_permutation_with_contiguous_stages():
    """Every source element appears once, and a stage -- (slice, column pair of the position grid, 64-column block) -- is 48 KB of
    consecutive elements holding exactly its 8 positions x 3 planes x 16 channels x 64 columns."""
    cout, cin = 128, 48
    idx = packed_index(cout, cin)
    flat = idx.reshape(-1)
    assert flat.numel() == 3 * 16 * cout * cin and torch.equal(flat.sort().values, torch.arange(flat.numel()))
    assert idx[0, 0, 0].numel() * 2 == 48 * 1024
    for cs, jh, cb in ((0, 0, 0), (2, 1, 1), (1, 0, 1)):
        src = idx[cs, jh, cb].reshape(-1)
        j = src % 4
        i = (src // 4) % 4
        ch = (src // 16) % cin
        o = (src // (16 * cin)) % cout
        p = src // (16 * cin * cout)
        assert set(j.tolist()) == {2 * jh, 2 * jh + 1} and set(i.tolist()) == {0, 1, 2, 3} and set(p.tolist()) == {0, 1, 2}
        assert set(ch.tolist()) == set(range(16 * cs, 16 * cs + 16)) and set(o.tolist()) == set(range(64 * cb, 64 * cb + 64))
    # a lane's ds_read_b128: eight consecutive channels of one column
    assert torch.equal(idx[1, 1, 0, 3, 2, 1, 7], idx[1, 1, 0, 3, 2, 1, 7, 0] + 16 * torch.arange(8))


@pytest.mark.parametrize("bad", [1e-36, float("nan"), float("inf")])
def test_weights_without_a_usable_split_are_refused_before_any_device_call(bad):
    """``U`` with a part below the normal range, or non-finite: ``split_stem_weights`` says unusable, so the packer returns ``None``
    (it asks before it allocates on the device: this runs without a GPU)."""
    from tiatoolbox_amd.models.architecture.fused import pack_conv_weights_wino_split, split_stem_weights, wino_weights_f32

    conv = torch.nn.Conv2d(16, 64, 3, padding=1)
    with torch.no_grad():
        conv.weight[3, 5] = 0  # (a corner tap alone: U[0][0] is the weight itself, not a sum that absorbs it)
        conv.weight[3, 5, 0, 0] = bad
    assert not split_stem_weights(wino_weights_f32(conv.weight))[1]
    assert pack_conv_weights_wino_split(conv) is None
    good = torch.nn.Conv2d(16, 64, 3, padding=1)
    parts, usable = split_stem_weights(wino_weights_f32(good.weight))
    assert usable and torch.equal(parts.double().sum(0), wino_weights_f32(good.weight).double())


def test_winograd_weights_follow_the_packers_operation_order():
    """``wino_weights_f32`` against G g G^T in float64 written out as the device packer does (rows, then columns; halves last)."""
    from tiatoolbox_amd.models.architecture.fused import wino_weights_f32

    g = torch.randn((8, 4, 3, 3), generator=torch.Generator().manual_seed(1))
    u = wino_weights_f32(g)
    gd = g.double()
    t = [gd[:, :, 0], 0.5 * (gd[:, :, 0] + gd[:, :, 1] + gd[:, :, 2]), 0.5 * (gd[:, :, 0] - gd[:, :, 1] + gd[:, :, 2]), gd[:, :, 2]]
    for i in range(4):
        uu = [t[i][..., 0], 0.5 * (t[i][..., 0] + t[i][..., 1] + t[i][..., 2]), 0.5 * (t[i][..., 0] - t[i][..., 1] + t[i][..., 2]), t[i][..., 2]]
        for j in range(4):
            assert torch.equal(u[:, :, i, j], uu[j].float())


# the stride-1 layer classes of resnet18 (map side, channels) at 256^2 / 224^2 patches, and what the table at
# tia_conv3x3_wino_bf16x3_serves admits of them at the headline batch
LAYERS_256 = [(64, 64), (32, 128), (16, 256), (8, 512)]
LAYERS_224 = [(56, 64), (28, 128), (14, 256), (7, 512)]
ADMITTED_4096 = [(64, 64), (32, 128), (16, 256)]


def test_route_query():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    serves, form = lib.tia_conv3x3_wino_bf16x3_serves, lib.tia_conv3x3_wino_form
    # the shapes tia_conv3x3_wino_form refuses: the same negative code
    for args in ((0, 64, 64, 64, 64, 1), (8, 64, 64, 64, 64, 3), (8, 64, 64, 24, 64, 1), (8, 64, 64, 64, 96, 1), (8, 0, 64, 64, 64, 1)):
        assert form(*args) < 0 and serves(*args) == form(*args), args
    # exactly the layer classes the committed table admits
    took = [(side, c) for side, c in LAYERS_256 + LAYERS_224 if serves(4096, side, side, c, c, 1) == 1]
    assert took == ADMITTED_4096, took
    # nothing next to the measured classes: 48^2 maps, rectangular maps, other channel counts, cin != cout
    for h, w, cin, cout in ((48, 48, 64, 64), (48, 48, 128, 128), (16, 64, 64, 64), (64, 32, 64, 64), (64, 64, 128, 128), (64, 64, 512, 512),
                            (32, 32, 64, 64), (32, 32, 256, 256), (16, 16, 128, 128), (16, 16, 512, 512), (64, 64, 64, 128), (32, 32, 128, 64),
                            (128, 128, 64, 64), (80, 80, 64, 64)):
        assert form(4096, h, w, cin, cout, 1) >= 0 and serves(4096, h, w, cin, cout, 1) == 0, (h, w, cin, cout)
    # small launches (fewer than two rounds of items over the compute units) stay where they are, whatever the class
    assert all(serves(16, side, side, c, c, 1) == 0 for side, c in LAYERS_256)
    # other paddings are not "same" layers of the table
    assert serves(4096, 64, 64, 64, 64, 0) == 0 and serves(4096, 64, 64, 64, 64, 2) == 0
    # the developer switch, read once per process: a fresh child
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from tiatoolbox_amd import _lib; "
            "print(_lib.load().tia_conv3x3_wino_bf16x3_serves(4096, 64, 64, 64, 64, 1))")
    for env, expect in (({"TIA_DEV": "1", "TIA_WINO_NO_SPLIT": "1"}, "0"), ({"TIA_WINO_NO_SPLIT": "1"}, "1")):
        out = subprocess.run([sys.executable, "-c", code, str(ROOT)], env={**os.environ, **env}, check=True, capture_output=True, text=True)
        assert out.stdout.strip() == expect, (env, out.stdout, out.stderr)

"""The split-operand Winograd F(2x2, 3x3) form on the bf16 matrix cores (``tia_conv3x3_wino_bf16x3_nhwc_f32``) on the GPU.

All kernel cases call ``hip_conv3x3_wino`` with the bf16 planes of ``pack_conv_weights_wino_split`` on small tensors.  The kernel's
units are a block of 16 x 16 outputs of one image, a 64-channel column block, a 16-channel slice (two steps each) and two patch
buffers; the shapes (19 x 13 and 16 x 16 maps: partial and full blocks; 7 x 7 and 8 x 8 maps with five images: the maps the float32
forms pack four to a block, here one block each; 16 / 48 / 64 input channels: one slice, an odd count, layer 1's; 64 / 128 output
channels) are the smallest that cross each of them.  The four-image and window geometries of the float32 form are not built for this
one, so the batch sizes 3 and 5 stand in for them.  The 1e-5 gate cannot see a lost ``lo`` plane (3e-6), so the EXACT
cases -- results without a rounded sum anywhere in the Winograd domain, bit for bit -- are what pins the three planes of both
operands, the mid x mid product and the addressing of all 16 positions.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from _wino_split_cases import case_integers, case_isolated_activations, case_isolated_powers_of_two, case_mid_mid, packed_index

pytestmark = pytest.mark.gpu

MAPS = ((19, 13), (16, 16), (7, 7), (8, 8))


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _conv_of(w: torch.Tensor, pad: int) -> torch.nn.Conv2d:
    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, padding=pad, bias=False)
    conv.weight = torch.nn.Parameter(w.clone(), requires_grad=False)
    return conv.cuda()


def _wino(x, w, bias, residual, *, pad: int, relu: bool, split: bool = True) -> torch.Tensor:
    """``hip_conv3x3_wino`` of CPU NCHW tensors through the split form (or the float32 F(2x2) form); the result back on the CPU."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_wino, pack_conv_weights_wino, pack_conv_weights_wino_split

    u = (pack_conv_weights_wino_split if split else pack_conv_weights_wino)(_conv_of(w, pad))
    assert u is not None and (u.dtype == torch.bfloat16) == split
    y = hip_conv3x3_wino(_nhwc(x), u, None if bias is None else bias.cuda(), None if residual is None else _nhwc(residual), padding=pad,
                         relu=relu)
    torch.cuda.synchronize()
    return y.cpu().contiguous()


def _random_layer(n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((n, cin, h, w), generator=g))
    wt = torch.randn((cout, cin, 3, 3), generator=g) / (9 * cin) ** 0.5
    return x, wt, torch.randn((cout,), generator=g)


@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("hw", MAPS)
def test_error_against_float64_is_within_the_summation_order_gate(hw, pad):
    """max |y - float64| <= 1e-5 max |y| for every channel combination, n = 3 and 5; the float32 Winograd kernel's error on the same
    tensors is printed beside it."""
    h, w = hw
    for n, cin, cout in ((5, 16, 64), (3, 48, 128), (5, 64, 64), (3, 64, 128)):
        x, wt, b = _random_layer(n, cin, cout, h, w, seed=1000 * n + cin + cout + 7 * h + pad)
        ref = F.conv2d(x.double(), wt.double(), b.double(), 1, pad)
        got = _wino(x, wt, b, None, pad=pad, relu=False)
        assert got.shape == ref.shape
        err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
        e32 = ((_wino(x, wt, b, None, pad=pad, relu=False, split=False).double() - ref).abs().max() / ref.abs().max()).item()
        print(f"{h}x{w} pad {pad} n={n} {cin}->{cout}: split {err:.2e}; float32 Winograd {e32:.2e}")
        assert err <= 1e-5, (n, cin, cout, err)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_every_epilogue_combination(with_bias, with_residual, relu):
    x, wt, b = _random_layer(5, 48, 128, 19, 13, seed=77)
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


def test_whole_batch_and_persistent_form_are_bit_identical_to_chunks():
    """A batch large enough for the persistent form (two rounds of items over the compute units, asked of the route query's rule through
    the item count) must equal the same batch in small chunks -- one block per workgroup -- bit for bit: 32 x 32 maps of 64 channels
    (four slices), 16 x 16 maps of 128 channels (two column blocks), and a 19 x 13 map (partial blocks)."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_wino, pack_conv_weights_wino_split

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device="cuda").manual_seed(11)
    for c, h, w, chunk in ((64, 32, 32, 7), (128, 16, 16, 5), (64, 19, 13, 3)):
        blocks = ((h + 15) // 16) * ((w + 15) // 16) * (c // 64)
        n = 2 * cus // blocks + 9
        conv = torch.nn.Conv2d(c, c, 3, padding=1).cuda()
        us = pack_conv_weights_wino_split(conv)
        x = torch.randn((n, c, h, w), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
        res = torch.randn_like(x)
        whole = hip_conv3x3_wino(x, us, conv.bias, res, padding=1, relu=True)
        parts = torch.cat([hip_conv3x3_wino(x[i:i + chunk], us, conv.bias, res[i:i + chunk], padding=1, relu=True)
                           for i in range(0, n, chunk)])
        assert torch.equal(whole, parts), (n, c, h, w)


_ONE_BLOCK_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import torch
from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_wino, pack_conv_weights_wino_split
torch.manual_seed(5)
conv = torch.nn.Conv2d(64, 64, 3, padding=1).cuda()
x = torch.randn((int(sys.argv[2]), 64, 32, 32), generator=torch.Generator().manual_seed(6)).cuda().contiguous(memory_format=torch.channels_last)
y = hip_conv3x3_wino(x, pack_conv_weights_wino_split(conv), conv.bias, x, padding=1, relu=True)
torch.save(y.cpu(), sys.argv[3])
"""


def test_persistent_form_is_bit_identical_to_one_block_per_workgroup(tmp_path):
    """The SAME batch through the persistent form (this process) and with ``TIA_DEV=1 TIA_WINO_NO_PERSIST=1`` (a fresh child: the
    switch is read once per process), which makes the library launch one block per workgroup whatever its own rule says."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count // 4 + 9
    outs = []
    for name, env in (("persist.pt", {}), ("blocks.pt", {"TIA_DEV": "1", "TIA_WINO_NO_PERSIST": "1"})):
        subprocess.run([sys.executable, "-c", _ONE_BLOCK_CHILD, str(root), str(n), str(tmp_path / name)], env={**os.environ, **env}, check=True)
        outs.append(torch.load(tmp_path / name))
    assert outs[0].shape == (n, 64, 32, 32) and bool((outs[0] != 0).any())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("pad", [0, 1, 2])
def test_exact_isolated_activations_through_all_sixteen_positions(pad):
    """(i) all three activation planes."""
    x, wt, ref = case_isolated_activations(pad)
    got = _wino(x, wt, None, None, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@pytest.mark.parametrize("pad", [0, 1, 2])
def test_exact_isolated_powers_of_two_return_the_weights(pad):
    """(ii) all three weight planes."""
    x, wt, ref = case_isolated_powers_of_two(pad)
    got = _wino(x, wt, None, None, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@pytest.mark.parametrize("pad", [0, 1])
def test_exact_mid_times_mid(pad):
    """(iii) (1 + 2^-10)^2 = 1 + 2^-9 + 2^-20 on the centre tap."""
    x, wt, ref = case_mid_mid(pad)
    got = _wino(x, wt, None, None, pad=pad, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


def test_exact_integer_accumulation():
    """(iv) dense small integers, every partial sum below 2^24 quanta in the Winograd domain: slices, positions, padding."""
    x, wt, ref = case_integers()
    got = _wino(x, wt, None, None, pad=1, relu=False)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


def _reads(shape, pad, positions) -> torch.Tensor:
    """Boolean [n, 1, ho, wo]: the outputs whose 3 x 3 window contains one of the input ``positions`` (image, row, column)."""
    mark = torch.zeros((shape[0], 1, shape[2], shape[3]), dtype=torch.float64)
    for b, yy, xx in positions:
        mark[b, 0, yy, xx] = 1
    return F.conv2d(mark, torch.ones((1, 1, 3, 3), dtype=torch.float64), None, 1, pad) > 0


def test_non_finite_and_overflowing_activations_never_give_a_finite_wrong_value():
    """One NaN, one +inf and one activation whose leading part overflows (3.4e38: bf16 rounds it to infinity), at a corner, an edge and
    an interior position of their 4 x 4 windows: every output that reads one of them is non-finite, every other output is bit for bit
    the clean run's.  (B^T d B carries a pixel to exactly the positions, and A^T M A those to exactly the outputs, whose taps reach it:
    the other outputs of the same TILE do not see it at all, so they are held to the stricter bit-equality, not to being non-finite.)
    3.39e38 has a finite leading part and an exact split: its outputs are the correct (finite or overflowed) float32 values."""
    pad = 1
    x, wt, b = _random_layer(5, 48, 128, 19, 13, seed=5)
    clean = _wino(x, wt, b, None, pad=pad, relu=False)
    bad = {(0, 3, 4, 7): float("nan"), (1, 20, 0, 0): float("inf"), (4, 47, 18, 12): 3.4e38, (3, 17, 9, 6): float("-inf")}
    xb = x.clone()
    for (bi, c, yy, xx), v in bad.items():
        xb[bi, c, yy, xx] = v
    got = _wino(xb, wt, b, None, pad=pad, relu=False)
    reads = _reads(x.shape, pad, [(bi, yy, xx) for bi, _, yy, xx in bad]).expand_as(got)
    assert reads.any() and not reads.all()
    assert not torch.isfinite(got[reads]).any()
    assert torch.equal(got[~reads], clean[~reads])
    # 3.39e38
    xh = x.clone()
    xh[2, 9, 6, 6] = 3.39e38
    got = _wino(xh, wt, b, None, pad=pad, relu=False)
    reads = _reads(x.shape, pad, [(2, 6, 6)]).expand_as(got)
    ref = F.conv2d(xh.double(), wt.double(), b.double(), 1, pad)
    assert torch.equal(got[~reads], clean[~reads])
    over = ref.abs() > torch.finfo(torch.float32).max
    assert not torch.isfinite(got[reads & over]).any()
    sel = reads & ~over & torch.isfinite(got)  # (a Winograd-domain sum may overflow where the convolution's does not: never finite and wrong)
    assert sel.any() and bool(((got[sel].double() - ref[sel]).abs() <= 1e-5 * ref[sel].abs().max()).all())


def test_packed_layout_matches_the_restatement_and_the_float32_packing():
    """The bf16 planes are the restated permutation of the split of ``U``, and that ``U`` is bit for bit the one the float32 form
    multiplies by (unpacked from ``pack_conv_weights_wino``)."""
    from tiatoolbox_amd.models.architecture.fused import (pack_conv_weights_wino, pack_conv_weights_wino_split, split_stem_weights,
                                                          wino_weights_f32)

    conv = torch.nn.Conv2d(48, 128, 3, padding=1).cuda()
    packed = pack_conv_weights_wino_split(conv)
    u = wino_weights_f32(conv.weight.detach().cpu())
    parts = split_stem_weights(u)[0]
    expect = parts.reshape(-1)[packed_index(128, 48).reshape(-1)].reshape(packed.shape)
    assert packed.dtype == torch.bfloat16 and torch.equal(packed.cpu().float(), expect)
    # [16 pos, cin/16 cs, 2 h8, cout/64 cb, 2 hi, 64 col, 4 c4] -> [cout, cin, 4, 4]
    uf = pack_conv_weights_wino(conv).cpu().permute(3, 5, 1, 2, 4, 6, 0).reshape(128, 48, 4, 4)
    assert torch.equal(uf, u)


def test_argument_checks_return_the_float32_forms_codes_and_leave_the_output_untouched():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    stream = _lib.current_stream()
    x = torch.randn((2, 16, 16, 64), device="cuda")
    u3 = torch.zeros((48 * 64 * 64,), dtype=torch.bfloat16, device="cuda")
    uf = torch.zeros((16 * 64 * 64,), device="cuda")
    y = torch.full((2 * 16 * 16 * 64,), 7.0, device="cuda")

    def split(xp, up, yp, cin, cout, pad=1, ho=16):
        return lib.tia_conv3x3_wino_bf16x3_nhwc_f32(xp, up, 0, 0, yp, 2, 16, 16, cin, cout, pad, pad, ho, ho, 0, stream)

    def plain(xp, up, yp, cin, cout, pad=1, ho=16):
        return lib.tia_conv3x3_wino_nhwc_f32(xp, up, 0, 0, yp, 2, 16, 16, cin, cout, pad, pad, ho, ho, 0, stream)

    for cin, cout, pad, ho in ((24, 64, 1, 16), (64, 96, 1, 16), (64, 64, 3, 16), (64, 64, 1, 0), (64, 64, 0, 19)):
        rc = split(x.data_ptr(), u3.data_ptr(), y.data_ptr(), cin, cout, pad, ho)
        assert rc < 0 and rc == plain(x.data_ptr(), uf.data_ptr(), y.data_ptr(), cin, cout, pad, ho), (cin, cout, pad, ho)
    for args in ((0, u3.data_ptr(), y.data_ptr()), (x.data_ptr(), 0, y.data_ptr()), (x.data_ptr(), u3.data_ptr(), 0),
                 (x.data_ptr() + 4, u3.data_ptr(), y.data_ptr())):
        assert split(*args, 64, 64) == -1, args
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert split(x.data_ptr(), u3.data_ptr(), y.data_ptr(), 64, 64) == 0  # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())
    assert lib.tia_conv_pack_weights_wino_bf16x3(x.data_ptr(), 64, 24, u3.data_ptr(), stream) == -3
    assert lib.tia_conv_pack_weights_wino_bf16x3(0, 64, 64, u3.data_ptr(), stream) == -1


def test_engine_takes_the_split_form_under_auto_only():
    """The smallest batch of 256 x 256 patches for which the query takes layer 1 (asked, not hard-coded): a ``PatchPredictor`` run of that
    batch launches ``conv3x3_wino_bf16x3_kernel`` under ``auto`` and not under ``direct``; probabilities within 1e-5, equal predictions."""
    from torch.profiler import ProfilerActivity, profile

    from tiatoolbox_amd.models.architecture.fused import wino_split_serves
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.utils import synth

    batch = next((n for n in range(4, 4097, 4) if wino_split_serves(n, 64, 64, 64, 64, 1)), None)
    assert batch is not None
    print("smallest batch of 256 x 256 patches on the split Winograd form:", batch)
    patches = synth.g_he(batch, 256, 256, seed=31)
    eng = PatchPredictor("resnet18-kather100k", batch_size=batch, device="cuda", verbose=False)
    eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(256, 256))  # builds the inference copy
    outs, seen = {}, {}
    for algo in ("auto", "direct"):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            outs[algo] = eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(256, 256), conv_algo=algo)
            torch.cuda.synchronize()
        seen[algo] = any("conv3x3_wino_bf16x3_kernel" in e.name for e in prof.events())
    assert seen == {"auto": True, "direct": False}, seen
    dp = np.abs(np.asarray(outs["auto"]["probabilities"], np.float64) - np.asarray(outs["direct"]["probabilities"], np.float64)).max()
    print(f"max |auto - direct| probability = {dp:.3e}")
    assert dp <= 1e-5, dp
    assert np.array_equal(outs["auto"]["predictions"], outs["direct"]["predictions"])

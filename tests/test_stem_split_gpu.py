"""The uint8 stem on the bf16 matrix cores with exactly split weights (``tia_stem_conv7x7_pool_nhwc_u8x3``).

(a) against the unfused float32 torch ops on the CPU at the float32 kernel's own gate, (b) the division by 255 bit for bit,
(c) known answers that do not depend on the summation order, bit for bit -- the check on how the bf16 MFMA accumulates in
float32, (d) which stem the engines launch.
"""

from __future__ import annotations

import copy
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from test_stem_gpu import SHAPES, _reference, _stem_parts


def _split_stem(conv, x_u8: torch.Tensor) -> torch.Tensor:
    from tiatoolbox_amd.models.architecture.fused import hip_stem_conv_pool_split, pack_stem_weights_split

    conv_d = copy.deepcopy(conv).cuda()
    wp = pack_stem_weights_split(conv_d)
    assert wp is not None and wp.shape == (3, 22, 64, 8) and wp.dtype == torch.bfloat16
    assert float(wp[:, 21].float().abs().max()) == 0.0  # k >= 168: zero padding
    return hip_stem_conv_pool_split(x_u8.cuda(), wp, conv_d.bias.detach().float().contiguous())


def _expected_from_sum(s: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``fl(S / 255) + bias``, ReLU, pool in float32 on the CPU (IEEE division and addition, element-wise)."""
    return F.max_pool2d(F.relu(s.float() / 255 + bias.float().view(1, -1, 1, 1)), 3, 2, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_split_stem_matches_unfused_torch_ops(shape):
    """(a) the gate of the float32 kernel (``test_stem_gpu.py``: 1e-5 absolute, float32 summation order only), same weights and
    inputs; batch views whose base address is 1, 2, 3 bytes off a dword give the same numbers."""
    n, h, w = shape
    conv = _stem_parts(seed=h * 1000 + w)
    g = torch.Generator().manual_seed(n + h + w)
    x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    ref = _reference(conv, x.float().div(255))
    got = _split_stem(conv, x)
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_contiguous(memory_format=torch.channels_last)
    err = (got.cpu() - ref).abs().max().item()
    print(f"(a) shape {shape}: max |split stem - float32 reference| = {err:.3e}")
    assert err <= 1e-5, err
    flat = torch.zeros(x.numel() + 8, dtype=torch.uint8)
    for off in (1, 2, 3):
        flat[off:off + x.numel()] = x.view(-1)
        view = flat.cuda()[off:off + x.numel()].view(n, h, w, 3)
        assert view.data_ptr() % 4 == off
        assert torch.equal(_split_stem(conv, view), got), off


@pytest.mark.gpu
def test_split_stem_unaligned_batch_slices():
    conv = _stem_parts(seed=3)
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (4, 37, 53, 3), generator=g, dtype=torch.uint8)  # 5883 bytes per image: slices are 3, 2, 1 off a dword
    full = _split_stem(conv, x)
    xd = x.cuda()
    for first in (1, 2, 3):
        assert xd[first:].data_ptr() % 4 != 0
        assert torch.equal(_split_stem(conv, xd[first:]), full[first:]), first


@pytest.mark.gpu
def test_split_stem_divides_every_byte_value_like_torch():
    """(b) one unit tap (centre, channel 0), no bias: the pooled value over a block of equal bytes is ``fl(v / 255)`` bit for bit."""
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=True)
    with torch.no_grad():
        conv.weight.zero_()
        conv.bias.zero_()
        conv.weight[:, 0, 3, 3] = 1.0
    x = torch.zeros((1, 8, 8 * 256, 3), dtype=torch.uint8)
    x[0, :, :, 0] = torch.arange(256, dtype=torch.uint8).repeat_interleave(8)[None, :]
    got = _split_stem(conv, x).cpu()  # [1, 64, 2, 512]: pooled column 2 b + 1 sees input columns 8 b + 2 .. 8 b + 6 only
    want = torch.arange(256).float().div(255)
    for ch in (0, 31, 32, 63):
        for row in (0, 1):
            assert torch.equal(got[0, ch, row, 1::2], want), (ch, row, (got[0, ch, row, 1::2] - want).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 256, 256), (3, 224, 224), (2, 37, 53), (1, 70, 600), (1, 131, 258)])
def test_split_stem_integer_weights_bit_for_bit(shape):
    """(c) integer weights in [-400, 400] (nine bits: planes hi and mid) and random bytes: every partial sum is an integer below
    2^24 in magnitude, so the sum is exact in ANY order; expected ``fl(S / 255) + bias``, ReLU, pool from integer arithmetic."""
    n, h, w = shape
    g = torch.Generator().manual_seed(h + 7 * w)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-400, 401, conv.weight.shape, generator=g).float())
        conv.bias.copy_(torch.randn(64, generator=g) * 50)
    assert 147 * 255 * int(conv.weight.abs().max()) < 1 << 24
    x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    with torch.inference_mode():
        s = F.conv2d(x.double().permute(0, 3, 1, 2), conv.weight.double(), None, 2, 3)  # integers: exact in float64
        assert float(s.abs().max()) < 1 << 24 and torch.equal(s, s.round())
        want = _expected_from_sum(s, conv.bias.detach())
    got = _split_stem(conv, x).cpu()
    bad = int((got != want).sum())
    print(f"(c) integer weights {shape}: {bad} of {want.numel()} values differ, max |diff| {(got - want).abs().max().item():.3e}")
    assert torch.equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 256, 256), (3, 224, 224), (2, 37, 53), (1, 70, 600)])
def test_split_stem_single_tap_full_mantissa_bit_for_bit(shape):
    """(c) ONE non-zero tap per output channel with a random 24-bit mantissa (all three planes) and inputs that are zero or a power
    of two: ``x * w`` is exact and is the whole sum, so the low plane must survive the accumulation bit for bit."""
    from tiatoolbox_amd.models.architecture.fused import split_stem_weights

    n, h, w = shape
    g = torch.Generator().manual_seed(3 * h + w)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=True)
    mant = torch.randint(0, 1 << 23, (64,), generator=g, dtype=torch.int32) | 1  # odd: the last mantissa bit is set
    sign = torch.randint(0, 2, (64,), generator=g, dtype=torch.int32) * -(1 << 31)
    expo = torch.randint(118, 124, (64,), generator=g, dtype=torch.int32) << 23  # |w| in [2^-9, 2^-3)
    vals = (mant | expo | sign).view(torch.float32)
    with torch.no_grad():
        conv.weight.zero_()
        conv.bias.copy_(torch.randn(64, generator=g) * 0.01)
        for o in range(64):
            c, ky, kx = (int(v) for v in torch.randint(0, 7, (3,), generator=g))
            conv.weight[o, c % 3, ky, kx] = vals[o]
    parts, usable = split_stem_weights(conv.weight.detach())
    assert usable and int((parts[2] != 0).sum()) >= 48  # the low plane carries bits for most channels
    x = (1 << torch.randint(0, 8, (n, h, w, 3), generator=g)).to(torch.uint8) * torch.randint(0, 2, (n, h, w, 3), generator=g, dtype=torch.uint8)
    with torch.inference_mode():
        s = F.conv2d(x.double().permute(0, 3, 1, 2), conv.weight.double(), None, 2, 3)  # one product per output: exact
        assert torch.equal(s.float().double(), s)  # ... and a float32 number
        want = _expected_from_sum(s, conv.bias.detach())
    got = _split_stem(conv, x).cpu()
    bad = int((got != want).sum())
    print(f"(c) single tap {shape}: {bad} of {want.numel()} values differ, max |diff| {(got - want).abs().max().item():.3e}")
    assert torch.equal(got, want)


def _stem_kernels(prof) -> set[str]:
    names = {e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()}
    return {n.replace(" ", "").replace("(bool)", "") for n in names if "stem7x7_pool_kernel" in n}


def _is_variant(name: str, mma: int) -> bool:
    return f"stem7x7_pool_kernel<true,{mma}>" in name or f"stem7x7_pool_kernel<1,{mma}>" in name or f"stem7x7_pool_kernelILb1ELi{mma}E" in name


@pytest.mark.gpu
def test_engine_takes_the_split_stem_under_auto_and_the_float32_stem_under_direct(caplog):
    """(d) ``PatchPredictor`` on uint8 patches: ``conv_algo="auto"`` launches ``stem7x7_pool_kernel<true, 3>``, ``"direct"`` the
    float32 variant and reproduces ``hip_stem_conv_pool`` + the blocks run by hand bit for bit; weights without an exact split
    keep the float32 stem."""
    from torch.profiler import ProfilerActivity, profile

    from tiatoolbox_amd.models.architecture.fused import MfmaResNet, hip_stem_conv_pool, pack_stem_weights
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.utils import synth

    patches = synth.g_he(16, 224, 224, seed=21)
    eng = PatchPredictor("resnet18-kather100k", batch_size=16, device="cuda", verbose=False)
    eng.run(patches, patch_mode=True, return_probabilities=True)  # builds the inference copy
    outs, kernels = {}, {}
    for algo in ("auto", "direct"):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            outs[algo] = eng.run(patches, patch_mode=True, return_probabilities=True, conv_algo=algo)
            torch.cuda.synchronize()
        kernels[algo] = _stem_kernels(prof)
    print("(d) stem kernels:", kernels)
    assert kernels["auto"] and all(_is_variant(k, 3) for k in kernels["auto"]), kernels
    assert kernels["direct"] and all(_is_variant(k, 0) for k in kernels["direct"]), kernels
    dp = np.abs(np.asarray(outs["auto"]["probabilities"], np.float64) - np.asarray(outs["direct"]["probabilities"], np.float64)).max()
    print(f"(d) max |auto - direct| probability = {dp:.3e}")
    assert dp <= 1e-5, dp
    assert np.array_equal(outs["auto"]["predictions"], outs["direct"]["predictions"])

    # direct by hand: the float32 stem entry point, the blocks, the head of CNNModel.forward
    model = eng._fast_model  # noqa: SLF001  (the inference copy of the last run: conv_algo="direct")
    trunk = model.feat_extract
    assert isinstance(trunk, MfmaResNet) and trunk.conv_algo == "direct"
    xd = torch.from_numpy(patches).cuda()
    with torch.inference_mode():
        stem = hip_stem_conv_pool(xd, pack_stem_weights(trunk.stem.weight.detach().float()), trunk.stem.bias.detach().float().contiguous())
        feat = trunk.blocks(stem)
        prob = torch.softmax(model.classifier(torch.flatten(model.pool(feat), 1)).float(), -1).cpu().numpy()
    assert np.array_equal(prob, np.asarray(outs["direct"]["probabilities"], prob.dtype))

    # weights without an exact split: one info line, and the float32 stem's numbers under "winograd" too
    broken = copy.deepcopy(trunk)
    with torch.no_grad():
        broken.stem.weight[7, 1, 2, 3] = 1e-36
    broken.set_conv_algo("winograd")
    with caplog.at_level(logging.INFO, logger="tiatoolbox_amd"):
        broken.prepare_stem(torch.float32)
    assert sum("no exact three-part bf16 split" in r.getMessage() for r in caplog.records) == 1
    with torch.inference_mode(), profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        got = broken.stem_forward(xd)
        torch.cuda.synchronize()
    ks = _stem_kernels(prof)
    assert ks and all(_is_variant(k, 0) for k in ks), ks
    want = hip_stem_conv_pool(xd, pack_stem_weights(broken.stem.weight.detach().float()), broken.stem.bias.detach().float().contiguous())
    assert torch.equal(got, want)
    # the intact trunk in the same mode takes the split kernel
    trunk.set_conv_algo("winograd")
    try:
        with torch.inference_mode(), profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            trunk.stem_forward(xd)
            torch.cuda.synchronize()
        ks = _stem_kernels(prof)
        assert ks and all(_is_variant(k, 3) for k in ks), ks
    finally:
        trunk.set_conv_algo("direct")

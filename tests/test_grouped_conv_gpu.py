"""The grouped 3x3 convolution of ResNeXt (``tia_conv3x3_grouped_nhwc_f32``) and the five new kather100k classifiers on the GPU:
kernel against CPU ``F.conv2d(groups=32)``, engine runs against the CPU run, no library convolution in float32, and the
half-precision route (BN-folded torch module, one warning)."""

from __future__ import annotations

import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
from tiatoolbox_amd.utils import synth

NEW = ("resnet101-kather100k", "resnext50_32x4d-kather100k", "resnext101_32x8d-kather100k", "wide_resnet50_2-kather100k",
       "wide_resnet101_2-kather100k")

# every conv2 of resnext50_32x4d (cg 4 .. 32) and resnext101_32x8d (cg 8 .. 64) at 224^2: (channels, map, stride); the stride-2
# ones are the first block of a stage; then odd maps for the stride-2 borders
SHAPES = [
    (128, 56, 56, 1), (256, 56, 56, 2), (256, 28, 28, 1), (512, 28, 28, 2), (512, 14, 14, 1), (1024, 14, 14, 2), (1024, 7, 7, 1),
    (512, 56, 56, 2), (1024, 28, 28, 2), (2048, 14, 14, 2), (2048, 7, 7, 1),
    (128, 11, 9, 2), (256, 15, 13, 2), (512, 9, 7, 2), (1024, 5, 3, 2), (2048, 7, 9, 2), (128, 3, 5, 1), (2048, 1, 1, 1),
]


@pytest.fixture(scope="module")
def patches():
    return synth.g_he(4, 224, 224, seed=41)


@pytest.mark.gpu
@pytest.mark.parametrize(("c", "h", "w", "stride"), SHAPES)
def test_grouped_kernel_matches_cpu_conv2d(c, h, w, stride):
    """``relu(conv2d(x, w, groups=32, stride, padding=1) + bias)``: max |delta| <= 1e-5 of the largest output magnitude."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_grouped, pack_grouped_conv_weights

    torch.manual_seed(c + h + w + stride)
    n = 2
    conv = torch.nn.Conv2d(c, c, 3, stride, 1, groups=32, bias=True)
    x = torch.randn(n, c, h, w)
    ref = F.relu(F.conv2d(x, conv.weight, conv.bias, stride=stride, padding=1, groups=32))
    conv = conv.cuda()
    xd = x.cuda().contiguous(memory_format=torch.channels_last)
    got = hip_conv3x3_grouped(xd, pack_grouped_conv_weights(conv), conv.bias.detach(), stride=stride, relu=True).cpu()
    assert got.shape == ref.shape
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, (c, h, w, stride, err)
    # without bias and ReLU
    raw = F.conv2d(x, conv.weight.cpu(), None, stride=stride, padding=1, groups=32)
    got = hip_conv3x3_grouped(xd, pack_grouped_conv_weights(conv), None, stride=stride, relu=False).cpu()
    assert float((got - raw).abs().max() / raw.abs().max()) <= 1e-5


@pytest.mark.gpu
def test_grouped_kernel_refuses_what_it_cannot_take():
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_grouped, pack_grouped_conv_weights

    conv = torch.nn.Conv2d(128, 128, 3, 1, 1, groups=32).cuda()
    wp = pack_grouped_conv_weights(conv)
    with pytest.raises(ValueError, match="float32 channels-last"):
        hip_conv3x3_grouped(torch.zeros((1, 128, 8, 8)), wp, None, stride=1, relu=True)  # host tensor
    with pytest.raises(ValueError, match="do not match"):
        hip_conv3x3_grouped(torch.zeros((1, 256, 8, 8), device="cuda").contiguous(memory_format=torch.channels_last), wp, None,
                            stride=1, relu=True)
    with pytest.raises(ValueError, match="4 to 64 channels per group"):
        pack_grouped_conv_weights(torch.nn.Conv2d(96, 96, 3, 1, 1, groups=32))
    x = torch.zeros((1, 8, 8, 128), device="cuda")
    y = torch.zeros((1, 8, 8, 128), device="cuda")
    lib = _lib.load()
    assert lib.tia_conv3x3_grouped_nhwc_f32(x.data_ptr(), wp.data_ptr(), 0, y.data_ptr(), 1, 8, 8, 32, 4, 3, 1, None) == _lib.TIA_EINVAL
    assert lib.tia_conv3x3_grouped_nhwc_f32(x.data_ptr(), wp.data_ptr(), 0, y.data_ptr(), 1, 8, 8, 32, 4, 1, 1, None) == 0
    assert lib.tia_conv3x3_grouped_nhwc_f32(x.data_ptr(), wp.data_ptr(), 0, y.data_ptr(), 1, 8, 8, 32, 12, 1, 1, None) == _lib.TIA_ESIZE
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NEW)
def test_engine_matches_cpu_run(patches, name, conv_algo):
    """``PatchPredictor(name)`` on the GPU (hand-written trunk: ``MfmaResNet``) against the CPU float32 run of the same seeded
    weights: identical predictions, probabilities within 1e-4, under both ``conv_algo`` values."""
    cpu = PatchPredictor(name, batch_size=4).run(patches, patch_mode=True, return_probabilities=True)
    eng = PatchPredictor(name, batch_size=4, device="cuda")
    gpu = eng.run(patches, patch_mode=True, return_probabilities=True, conv_algo=conv_algo)
    fast = eng._inference_model(torch.float32)  # noqa: SLF001
    assert type(fast.feat_extract).__name__ == "MfmaResNet"
    err = float(np.abs(gpu["probabilities"] - cpu["probabilities"]).max())
    assert err <= 1e-4, err
    assert np.array_equal(gpu["predictions"], cpu["predictions"])


@pytest.mark.gpu
def test_float32_resnext_run_launches_only_handwritten_convolutions(patches):
    from torch.profiler import ProfilerActivity, profile

    x = torch.from_numpy(patches).cuda()
    eng = PatchPredictor("resnext50_32x4d-kather100k", batch_size=4, device="cuda", verbose=False)
    eng.run(x, patch_mode=True, return_probabilities=True)  # builds the inference copy
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out = eng.run(x, patch_mode=True, return_probabilities=True)
        torch.cuda.synchronize()
    assert np.isfinite(out["probabilities"]).all()
    names = {e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()}
    kernels = {n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()}
    assert any("conv3x3_grouped_kernel" in k for k in kernels), kernels
    assert any("conv_mfma_f32_kernel" in k for k in kernels), kernels
    assert any("stem7x7_pool_kernel" in k for k in kernels), kernels
    banned = ("igemm", "naive_conv", "SubTensorOp", "ck::", "miopen", "MIOpen", "Im2Col", "gemm_conv", "grouped_conv_fwd")
    offenders = {k for k in kernels if any(b in k for b in banned)}
    assert not offenders, offenders


@pytest.mark.gpu
def test_half_precision_resnext_runs_the_folded_torch_module(patches, caplog):
    """fp16 has no grouped kernel: the inference copy is the BN-folded torch module (not ``MfmaResNet``), with one warning
    saying so; probabilities within the half-precision tolerance of the float32 run."""
    eng = PatchPredictor("resnext50_32x4d-kather100k", batch_size=4, device="cuda")
    ref = eng.run(patches, patch_mode=True, return_probabilities=True)
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = eng.run(patches, patch_mode=True, return_probabilities=True, compute_dtype="float16")
    warned = [r for r in caplog.records if "grouped convolutions" in r.getMessage()]
    assert len(warned) == 1, [r.getMessage() for r in caplog.records]
    fast = eng._inference_model(torch.float16)  # noqa: SLF001
    assert not any(type(m).__name__ == "MfmaResNet" for m in fast.modules())
    err = float(np.abs(got["probabilities"] - ref["probabilities"]).max())
    assert err <= 1e-3, err

"""Winograd F(4x2, 3x3) (``conv3x3_wino42_kernel``, csrc/conv3x3_wino42.hip): packed weights, accuracy against a CPU float32
convolution at the 1e-5 gate of the F(2x2) kernel, the persistent form against one block per workgroup, the route query, and the
resnet18 patch predictor at 256^2 patches."""

from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

G4 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                   [0, 0, 1]], dtype=torch.float64)
G2 = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)


def _lib_or_skip():
    from tiatoolbox_amd import _lib, build

    if not build.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib.load()


def test_route_query_takes_f42_for_the_256_maps():
    """``tia_conv3x3_wino_form`` (host only): F(4x2) for "same"-padded 32^2 / 16^2 maps and maps of at most 8 x 8, F(2x2) for
    everything else (the 64^2 map of 256^2 patches, a tie; the 56 / 28 / 14 maps of 224^2 patches; other paddings), an error for
    shapes no form serves."""
    lib = _lib_or_skip()
    for hw, c in ((32, 128), (16, 256), (8, 512), (7, 512), (32, 64)):
        assert lib.tia_conv3x3_wino_form(1024, hw, hw, c, c, 1) == 1, hw
    for hw, c in ((64, 64), (128, 64), (56, 64), (28, 128), (14, 256), (20, 64), (33, 64)):
        assert lib.tia_conv3x3_wino_form(1024, hw, hw, c, c, 1) == 0, hw
    assert lib.tia_conv3x3_wino_form(16, 64, 64, 64, 64, 0) == 0
    assert lib.tia_conv3x3_wino_form(16, 64, 64, 64, 64, 2) == 0
    assert lib.tia_conv3x3_wino_form(16, 64, 64, 24, 64, 1) < 0
    assert lib.tia_conv3x3_wino_form(16, 64, 64, 64, 96, 1) < 0
    assert lib.tia_conv3x3_wino_form(0, 64, 64, 64, 64, 1) < 0


@pytest.mark.gpu
def test_f42_packed_weights_are_g4_g_g2t():
    """``pack_conv_weights_wino42`` = ``G4 g G2^T`` computed in float64 and rounded once, in the [pos 24][cin/16][2][cout/64][2][64][4]
    stage layout."""
    from tiatoolbox_amd.models.architecture.fused import pack_conv_weights_wino42

    g = torch.Generator().manual_seed(3)
    for cin, cout in ((16, 64), (64, 128), (48, 192)):
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        up = pack_conv_weights_wino42(conv.cuda())
        assert up.shape == (24, cin // 16, 2, cout // 64, 2, 64, 4)
        u = up.cpu().permute(0, 3, 5, 1, 2, 4, 6).reshape(6, 4, cout, cin).permute(2, 3, 0, 1)  # [cout][cin][i][j]
        ref = (G4 @ conv.weight.detach().cpu().double() @ G2.T).float()
        # one rounding of a float64 transform: within one float32 step of the reference everywhere (the two float64 evaluations
        # differ in the last bits, which moves a rounding by one step now and then; near-zero results by cancellation only)
        step = torch.from_numpy(np.spacing(ref.abs().numpy()))
        assert bool(((u - ref).abs() <= torch.maximum(step, torch.tensor(1e-12 * ref.abs().max().item()))).all())
        assert (u == ref).double().mean().item() > 0.95
    with pytest.raises(ValueError, match="Winograd"):
        pack_conv_weights_wino42(torch.nn.Conv2d(24, 64, 3).cuda())


@pytest.mark.gpu
def test_f42_conv_matches_torch_cpu_fp32():
    """Every 3x3 / stride-1 shape of resnet18 at 256^2 patches, blocks whole and clipped, four-image blocks incl. a partial one,
    every epilogue variant: max |delta| <= 1e-5 of the largest output magnitude against CPU float32 conv2d."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_wino, pack_conv_weights_wino42

    g = torch.Generator().manual_seed(7)
    cases = [(3, 64, 64, 64), (2, 128, 128, 32), (2, 256, 256, 16), (9, 512, 512, 8),  # 256^2 patches' maps
             (6, 512, 512, 7), (5, 64, 64, 8), (1, 32, 64, 20), (2, 16, 128, 13), (1, 64, 64, 48), (3, 48, 192, 5)]
    for n, cin, cout, hw in cases:
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=True)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (cin * 9)) ** 0.5)
            conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
        x = torch.randn((n, cin, hw, hw), generator=g)
        w_cpu, b_cpu = conv.weight.detach().clone(), conv.bias.detach().clone()
        ref_lin = F.conv2d(x, w_cpu, b_cpu, padding=1)
        res = torch.randn(ref_lin.shape, generator=g)
        dev_conv = conv.cuda()
        up = pack_conv_weights_wino42(dev_conv)
        xd = x.cuda().contiguous(memory_format=torch.channels_last)
        rd = res.cuda().contiguous(memory_format=torch.channels_last)
        scale = ref_lin.abs().max().item()
        for use_bias, use_res, relu in ((True, False, False), (True, False, True), (True, True, True), (False, True, False)):
            exp = F.conv2d(x, w_cpu, b_cpu if use_bias else None, padding=1) + (res if use_res else 0)
            exp = torch.relu(exp) if relu else exp
            got = hip_conv3x3_wino(xd, up, dev_conv.bias if use_bias else None, rd if use_res else None, padding=1, relu=relu)
            assert got.shape == exp.shape and got.is_contiguous(memory_format=torch.channels_last)
            err = (got.cpu() - exp).abs().max().item() / scale
            assert 0.0 < err <= 1e-5, (n, cin, cout, hw, use_bias, use_res, relu, err)


@pytest.mark.gpu
def test_f42_persistent_form_is_bit_identical_to_one_block_per_workgroup():
    """Launches with at least two rounds of (pixel block, channel tile) items per CU take the persistent form; a batch computed whole
    must equal the same batch computed in small chunks (one block per workgroup) bit for bit, 16 x 16 and four-image blocks."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_wino, pack_conv_weights_wino42

    g = torch.Generator(device="cuda").manual_seed(11)
    for n, c, hw, chunk in ((40, 64, 64, 2), (30, 128, 40, 3), (264, 512, 8, 4), (130, 256, 16, 2)):
        conv = torch.nn.Conv2d(c, c, 3, padding=1).cuda()
        up = pack_conv_weights_wino42(conv)
        x = torch.randn((n, c, hw, hw), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
        res = torch.randn_like(x)
        whole = hip_conv3x3_wino(x, up, conv.bias, res, padding=1, relu=True)
        parts = torch.cat([hip_conv3x3_wino(x[i:i + chunk], up, conv.bias, res[i:i + chunk], padding=1, relu=True)
                           for i in range(0, n, chunk)])
        assert torch.equal(whole, parts), (n, c, hw)


@pytest.mark.gpu
def test_patch_predictor_256_takes_f42_within_tolerance_of_direct():
    """resnet18 ``PatchPredictor`` on 256^2 patches: ``conv_algo="auto"`` runs the 9 stride-1 3x3 layers of layer2..4 on F(4x2) and
    the 4 of layer1 (64^2) on F(2x2), as the route query says; probabilities within 1e-5 of ``"direct"``, identical predictions,
    ``"winograd"`` bit-equal to ``"auto"``."""
    from tiatoolbox_amd.models.architecture.fused import wino_form
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.utils import synth

    assert wino_form(16, 64, 64, 64, 64, 1) == 0
    for hw, c in ((32, 128), (16, 256), (8, 512)):
        assert wino_form(16, hw, hw, c, c, 1) == 1
    patches = synth.g_he(24, 256, 256, seed=4)
    eng = PatchPredictor("resnet18-kather100k", batch_size=16, device="cuda", verbose=False)
    auto = eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(256, 256))
    direct = eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(256, 256), conv_algo="direct")
    wino = eng.run(patches, patch_mode=True, return_probabilities=True, patch_input_shape=(256, 256), conv_algo="winograd")
    assert np.array_equal(wino["probabilities"], auto["probabilities"])
    dp = np.abs(np.asarray(auto["probabilities"], np.float64) - np.asarray(direct["probabilities"], np.float64)).max()
    assert 0.0 < dp <= 1e-5, dp
    assert np.array_equal(auto["predictions"], direct["predictions"])
    # the trunk of the last run ("winograd") holds F(4x2) weights for the 9 layers the route gives it: the kernel ran
    packed = [k for m in eng._fast_model.modules() for k in getattr(m, "_packed", {}) if k[1] == "wino42"]
    assert len(packed) == 9, packed

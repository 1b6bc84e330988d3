"""Host-side checks of the plain-encoder and concat-skip UNet graphs (``FusedPlainUNet``, ``FusedUNet`` with
``skip_type="concat"``) WITHOUT a GPU, by the method of ``test_fused_graphs.py``: the HIP wrappers are replaced by their plain-torch
definitions, so what is tested is the graph surgery -- which BN folds into which convolution, where the pooling and the
concatenation sit, which affine the concat pass of the ResNet-50 decoder carries.  The two new definitions are

* ``hip_avgpool2x2(x)``                     = ``F.avg_pool2d(x, 2, 2)``;
* ``hip_upsample2x_concat(x, y, sc, sh)``   = ``torch.cat([x.repeat_interleave(2, 2).repeat_interleave(2, 3), y], 1)``, followed by
  ``relu(. * sc + sh)`` when an affine is given.

The kernels themselves are compared with these definitions in ``test_unet_plain_gpu.py`` (``-m gpu``).  ``avgpool_ref`` of
``_unet_plain_ref.py`` is the arithmetic the pooling kernel is held to, written out with slices; it is shown here to BE torch's
``avg_pool2d`` bit for bit, and the pairwise order to be another function.
"""

from __future__ import annotations

import copy
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F  # noqa: N812

sys.path.insert(0, str(Path(__file__).resolve().parent))
from _unet_plain_ref import (CONFIGS, DTYPES, POOL_SHAPES, avgpool_ref, build, concat_hand_example, concat_ref,  # noqa: E402
                             fused_class)
from test_fused_graphs import torch_kernels  # noqa: E402, F401  (the fixture that replaces the convolution wrappers)

from tiatoolbox_amd.models.architecture.unet import UNetModel  # noqa: E402
from tiatoolbox_amd.models.architecture.unet_fused import FusedPlainUNet, FusedUNet  # noqa: E402


@pytest.fixture
def plain_kernels(torch_kernels, monkeypatch):  # noqa: F811
    _, uf = torch_kernels
    calls = {"pool": 0, "concat": 0, "affine": 0}

    def pool(x):
        calls["pool"] += 1
        return F.avg_pool2d(x, 2, 2)

    def concat(x, y, scale=None, shift=None):
        calls["concat"] += 1
        calls["affine"] += scale is not None
        assert (scale is None) == (shift is None) and (scale is None or scale.shape == shift.shape == (x.shape[1] + y.shape[1],))
        return concat_ref(x, y, scale, shift)

    monkeypatch.setattr(uf, "hip_avgpool2x2", pool)
    monkeypatch.setattr(uf, "hip_upsample2x_concat", concat)
    return calls


@pytest.mark.parametrize("name", list(CONFIGS))
def test_graph_equals_forward(plain_kernels, name):
    model, x = build(name)
    with torch.inference_mode():
        ref = model(x)
        fused = fused_class(name)(copy.deepcopy(model))
        got = fused(x)
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert float((got - ref).abs().max()) <= 2e-6, float((got - ref).abs().max())
    routes = [m.route for m in fused.modules() if hasattr(m, "route")]
    assert "torch" not in routes and routes.count("thin") == 1 and routes.count("head") == 1
    if name == "plain-add":
        assert plain_kernels == {"pool": 2, "concat": 0, "affine": 0} and not fused.accepts_uint8
    elif name == "plain-concat":
        assert plain_kernels == {"pool": 2, "concat": 2, "affine": 0} and not fused.accepts_uint8
    else:  # four decoder stages, each with its 2 ch-channel BN + ReLU inside the concat pass
        assert plain_kernels == {"pool": 0, "concat": 4, "affine": 4} and fused.accepts_uint8
        assert [stage[0].scale.numel() for stage in fused.up] == [2048, 1024, 512, 128]


def test_plain_graph_takes_the_same_bytes_as_floats_of_any_dtype(plain_kernels):  # noqa: ARG001
    """``x / 255`` is computed through float64: the batch as bytes, as float32 and as float64 gives the same logits."""
    model, x = build("plain-add")
    fused = FusedPlainUNet(copy.deepcopy(model))
    with torch.inference_mode():
        got = fused(x)
        assert torch.equal(fused(x.to(torch.uint8)), got) and torch.equal(fused(x.double()), got)


def test_refusals_name_the_layer():
    with pytest.raises(TypeError, match=r"no hand-written kernel for layer `backbone\.blocks\.0\.0\.0`"):
        FusedPlainUNet(UNetModel(3, 2, "unet", encoder_levels=[4, 8, 16]))
    with pytest.raises(TypeError, match="layer `clf`"):  # a 128 -> 2 class head: the head kernel reads 64 channels
        FusedPlainUNet(UNetModel(3, 2, "unet", encoder_levels=[128, 128]))
    with pytest.raises(TypeError, match=r"layer `backbone\.blocks\.0\.0\.0`"):  # 11 channels x 3 taps > 32
        FusedPlainUNet(UNetModel(11, 2, "unet", encoder_levels=[64, 64]))
    with pytest.raises(TypeError, match="plain conv-BN-ReLU"):
        FusedPlainUNet(UNetModel(3, 2, "resnet50"))
    with pytest.raises(TypeError, match="ResNet-50 encoder"):
        FusedUNet(UNetModel(3, 2, "unet"))
    # every refusal is the constructors' own exception (what the engine falls back on; any other error propagates there)
    from tiatoolbox_amd.models.architecture.unet_fused import UnsupportedLayerError

    for make in (lambda: FusedPlainUNet(UNetModel(3, 2, "unet", encoder_levels=[4, 8, 16])), lambda: FusedUNet(UNetModel(3, 2, "unet"))):
        with pytest.raises(UnsupportedLayerError):
            make()
    odd = UNetModel(3, 2, "unet", encoder_levels=[64, 64])
    odd.backbone.blocks[0][1] = torch.nn.AvgPool2d(2, stride=2, ceil_mode=True)  # the kernel divides odd maps with floor
    with pytest.raises(UnsupportedLayerError, match="ceil_mode"):
        FusedPlainUNet(odd)


def test_library_convolutions_lists_what_a_fused_unet_builds_around():
    """``FusedUNet`` accepts a decoder convolution off the MFMA tile (64 -> 48: the library runs it in float32); the list the engine
    warns with names it, and is empty for the graphs of this file."""
    from tiatoolbox_amd.models.architecture.unet_fused import library_convolutions

    model, _ = build("resnet50-concat")
    assert library_convolutions(FusedUNet(copy.deepcopy(model))) == []
    assert library_convolutions(FusedPlainUNet(build("plain-add")[0])) == []
    narrow = copy.deepcopy(model)
    narrow.uplist[3][5] = torch.nn.Conv2d(64, 48, 3, padding=1, bias=False)
    narrow.clf = torch.nn.Conv2d(48, 5, 1)
    assert library_convolutions(FusedUNet(narrow)) == ["up.3.2", "clf"]


def _pack_h(conv, dtype):  # what `pack_conv_weights_h` holds: [kh, kw, cin / 8, cout, 8] halves of the float32 weights
    w = conv.weight.detach()
    assert w.dtype == torch.float32  # packed from the float32, BN-folded weights: one rounding
    cout, cin, kh, kw = w.shape
    return w.to(dtype).reshape(cout, cin // 8, 8, kh, kw).permute(3, 4, 1, 0, 2).contiguous()


@pytest.mark.parametrize("name", ["plain-concat", "resnet50-concat"])
def test_prepare_keeps_float32_operands_through_the_cast(monkeypatch, name):
    import tiatoolbox_amd.models.architecture.hovernet_fused as hf
    import tiatoolbox_amd.models.architecture.unet_fused as uf
    from tiatoolbox_amd.models.architecture.hovernet_fused import _BnAct, _Conv

    monkeypatch.setattr(hf, "pack_conv_weights_h", _pack_h)
    monkeypatch.setattr(uf, "pack_stem_weights", lambda weight: torch.cat([weight.detach().permute(2, 3, 1, 0).reshape(147, 64),
                                                                           torch.zeros(1, 64)]))
    model, _ = build(name)
    fused = fused_class(name)(copy.deepcopy(model))
    want_bias = {n: m.bias.detach().clone() for n, m in fused.named_modules() if isinstance(m, _Conv) and m.bias is not None}
    want_affine = {n: (m.scale.clone(), m.shift.clone()) for n, m in fused.named_modules() if isinstance(m, _BnAct)}
    thin = fused.enc[0][0] if name == "plain-concat" else None
    want_thin = hf.pack_thin_conv_weights(thin.weight) if thin is not None else None
    fused.prepare(torch.float16)
    fused = fused.to(torch.float16)
    assert fused.half_dtype == torch.float16 and next(fused.parameters()).dtype == torch.float16  # the cast happened ...
    stem = getattr(fused, "stem", None)  # (FusedUNet's stem runs on the stem kernel and keeps its own float32 copies)
    for n, mod in fused.named_modules():  # ... and left the float32 operands alone, bit for bit
        if isinstance(mod, _Conv) and mod is not stem:
            assert mod.half_dtype == torch.float16 and (mod.bias is None) == (mod._bias32 is None)  # noqa: SLF001
            if mod.bias is not None:
                assert mod.bias.dtype == torch.float16 and mod._bias32.dtype == torch.float32  # noqa: SLF001
                assert torch.equal(mod._bias32, want_bias[n])  # noqa: SLF001
            if mod.route == "mfma":
                assert mod._packed_h.dtype == torch.float16  # noqa: SLF001
        if isinstance(mod, _BnAct):
            sc, sh = mod.affine32()
            assert sc.dtype == sh.dtype == torch.float32 and mod.scale.dtype == torch.float16
            assert torch.equal(sc, want_affine[n][0]) and torch.equal(sh, want_affine[n][1])
    assert fused.clf._weight32.dtype == torch.float32  # noqa: SLF001
    if thin is not None:
        assert thin.route == "thin" and thin._packed.dtype == torch.float32 and torch.equal(thin._packed, want_thin)  # noqa: SLF001
        assert not want_affine  # post-activation blocks: every BN is folded
    else:
        assert len(want_affine) == 4
        assert fused._stem_packed.dtype == torch.float32 and torch.equal(fused._stem_bias32, want_bias["stem"])  # noqa: SLF001


def test_prepare_refuses_a_cast_module_and_other_dtypes():
    model, _ = build("plain-add")
    fused = FusedPlainUNet(copy.deepcopy(model))
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        fused.prepare(torch.float64)
    with pytest.raises(ValueError, match="before the cast"):
        fused.half().prepare(torch.float16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pooling_reference_is_avg_pool2d_bit_for_bit(dtype):
    """The order the kernel is held to, on the GPU test's shapes (contiguous and channels-last alike)."""
    g = torch.Generator().manual_seed(21)
    differ = total = 0
    for n, h, w, c in POOL_SHAPES:
        x = (torch.randn((n, c, h, w), generator=g) * 3).to(dtype)
        want = F.avg_pool2d(x, 2, 2)
        assert torch.equal(F.avg_pool2d(x.contiguous(memory_format=torch.channels_last), 2, 2), want)
        assert torch.equal(avgpool_ref(x), want), (n, h, w, c)
        differ += int((avgpool_ref(x, "pairwise") != want).sum())
        total += want.numel()
    if dtype == torch.float32:  # the pairwise sum is another function: the equality test on the device separates the two
        assert differ > total // 10, (differ, total)


@pytest.mark.parametrize("dtype", DTYPES)
def test_concat_reference_on_a_hand_worked_pixel(dtype):
    """The reference gives the hand-worked numbers, and a fused multiply-add is another function ON THESE INPUTS (channels 0 and 8)."""
    x, y, scale, shift, want_act, want_plain = concat_hand_example(dtype)
    assert torch.equal(concat_ref(x, y, scale, shift).double(), want_act)
    assert torch.equal(concat_ref(x, y).double(), want_plain)
    fma = concat_ref(x, y, scale, shift, variant="fma").double()
    assert (fma[0, :, 0, 0] != want_act[0, :, 0, 0]).nonzero().flatten().tolist() == [0, 8]
    assert float(fma[0, 0, 0, 0]) > float(want_act[0, 0, 0, 0])


def test_wrappers_refuse_host_tensors():
    from tiatoolbox_amd.models.architecture import fused

    x = torch.zeros((1, 8, 2, 2)).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="CUDA"):
        fused.hip_avgpool2x2(x)
    with pytest.raises(ValueError, match="CUDA"):
        fused.hip_upsample2x_concat(x, torch.zeros((1, 8, 4, 4)))

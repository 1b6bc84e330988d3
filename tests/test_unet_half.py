"""Host-side checks of the half-precision ``FusedUNet`` (no GPU): the new C entry points are declared, the references of
``_unet_half_ref.py`` say what they claim (a hand-worked example, and the wrong variants are told apart), and ``prepare(dtype)``
keeps what the half kernels take in float32 through ``module.to(dtype)`` -- with the HIP calls replaced by their plain-torch
definitions, like ``test_fused_graphs.py``, the half graph is then run on the CPU against the plain module."""

from __future__ import annotations

import copy
import re
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F  # noqa: N812

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _unet_half_ref as R  # noqa: E402, N812

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("tia_upsample2x_add_act_nhwc_h", "tia_stem_conv7x7_pool_conv_nhwc", "tia_conv1x1_head_nhwc_h")


def test_new_entry_points_are_declared_in_header_and_binding():
    from tiatoolbox_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tiatoolbox_amd.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"^\s*int\s+{name}\s*\(", header, flags=re.M), name
        assert name in _lib._SIGNATURES, name  # noqa: SLF001
    # the dtype travels as an int32 in front of the stream / the output
    assert len(_lib._SIGNATURES["tia_upsample2x_add_act_nhwc_h"][0]) == len(_lib._SIGNATURES["tia_upsample2x_add_act_nhwc_f32"][0]) + 1  # noqa: SLF001
    assert len(_lib._SIGNATURES["tia_conv1x1_head_nhwc_h"][0]) == len(_lib._SIGNATURES["tia_conv1x1_head_nhwc_f32"][0]) + 1  # noqa: SLF001
    assert _lib._SIGNATURES["tia_stem_conv7x7_pool_conv_nhwc"] == _lib._SIGNATURES["tia_stem_conv7x7_pool_nhwc"]  # noqa: SLF001


@pytest.mark.parametrize("dtype", R.HALVES)
def test_upsample_add_reference_on_a_hand_worked_pixel(dtype):
    x, y, scale, shift, want_act, want_plain = R.hand_example(dtype)
    got = R.upsample_add_ref(x, y, scale, shift)
    assert got.dtype == dtype and got.shape == (1, 8, 2, 2)
    assert torch.equal(got.double(), want_act)
    assert torch.equal(R.upsample_add_ref(x, y).double(), want_plain)
    # the near misses are other functions ON THESE INPUTS: channel 0 tells a fused multiply-add, channel 1 an early rounding of s
    fma = R.upsample_add_ref(x, y, scale, shift, variant="fma").double()
    early = R.upsample_add_ref(x, y, scale, shift, variant="round_s").double()
    m = R.MANTISSA[dtype]
    assert not torch.equal(fma, want_act) and float(fma[0, 0, 0, 0]) == 2.0 ** -(24 - m) * (1 + 2.0 ** -m)
    assert torch.equal(fma[:, 1:], want_act[:, 1:])
    assert not torch.equal(early, want_act) and float(early[0, 1, 0, 0]) == 0.0
    assert torch.equal(early[:, 2:], want_act[:, 2:])


@pytest.mark.parametrize("dtype", R.HALVES)
def test_early_rounding_differs_on_random_data_too(dtype):
    """The random inputs of the GPU test separate the contract from the early rounding of ``s`` as well (a fused multiply-add differs
    from it in the last float32 bit only, which reaches the half result too rarely to count on: the hand-worked pixel covers it)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 64, 8, 8), generator=g).to(dtype)
    y = torch.randn((2, 64, 16, 16), generator=g).to(dtype)
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    ref = R.upsample_add_ref(x, y, sc, sh)
    assert (ref == 0).any() and (ref > 0).any()  # the ReLU cuts
    assert not torch.equal(ref, R.upsample_add_ref(x, y, sc, sh, variant="round_s"))


def test_head_reference_bound_is_far_below_the_output_range():
    g = torch.Generator().manual_seed(4)
    x = torch.randn((63, 64), generator=g).to(torch.float16)
    w, b = torch.randn((5, 64), generator=g) * 0.2, torch.randn(5, generator=g)
    ref, bound = R.head_ref(x, w, b)
    assert torch.allclose(ref, x.double() @ w.double().T + b.double())
    assert float(bound.max()) * 100 <= float(ref.max() - ref.min())
    ref_pre, _ = R.head_ref(x, w, b, torch.full((64,), 2.0), torch.full((64,), -1.0))
    assert torch.allclose(ref_pre, torch.clamp_min(x.double() * 2 - 1, 0) @ w.double().T + b.double())


# ---- the half graph on the CPU: HIP calls replaced by what the header says they compute --------------------------------------------
def _unpack_h(wp):  # [kh, kw, cin/8, cout, 8] -> OIHW
    kh, kw, c8, cout, _ = wp.shape
    return wp.permute(3, 2, 4, 0, 1).reshape(cout, c8 * 8, kh, kw)


@pytest.fixture
def torch_half_kernels(monkeypatch):
    import tiatoolbox_amd.models.architecture.hovernet_fused as hf
    import tiatoolbox_amd.models.architecture.unet_fused as uf

    calls = {"conv_h": 0, "up": 0, "head": 0, "stem": 0}

    def pack_h(conv, dtype):
        w = conv.weight.detach()
        assert w.dtype == torch.float32  # packed from the float32, BN-folded weights: one rounding
        cout, cin, kh, kw = w.shape
        return w.to(dtype).reshape(cout, cin // 8, 8, kh, kw).permute(3, 4, 1, 0, 2).contiguous()

    def conv_h(x, wp, bias, res, *, cout, kernel, stride, padding, relu):
        calls["conv_h"] += 1
        assert x.dtype == wp.dtype and x.dtype in R.HALVES and (bias is None or bias.dtype == torch.float32)
        assert res is None or res.dtype == x.dtype
        y = F.conv2d(x.float(), _unpack_h(wp).float(), bias, stride, padding)
        assert y.shape[1] == cout and wp.shape[0] == kernel
        y = y + res.float() if res is not None else y
        return (F.relu(y) if relu else y).to(x.dtype)

    def up(x, y, scale=None, shift=None):
        calls["up"] += 1
        assert x.dtype == y.dtype and x.dtype in R.HALVES and (scale is None or scale.dtype == shift.dtype == torch.float32)
        return R.upsample_add_ref(x, y, scale, shift)

    def stem(x_nhwc, wp, bias, *, out_dtype=torch.float32, return_conv=False):
        calls["stem"] += 1
        assert wp.dtype == bias.dtype == torch.float32
        w = wp[:147].view(7, 7, 3, 64).permute(3, 2, 0, 1)
        xf = x_nhwc.float().div(255) if x_nhwc.dtype == torch.uint8 else x_nhwc
        conv = F.relu(F.conv2d(xf.permute(0, 3, 1, 2), w, bias, 2, 3))
        pooled = F.max_pool2d(conv, 3, 2, 1)
        return (pooled.to(out_dtype), conv.to(out_dtype)) if return_conv else pooled.to(out_dtype)

    def head(x, weight, bias, *, pre_scale=None, pre_shift=None):
        calls["head"] += 1
        assert x.dtype in R.HALVES and weight.dtype == torch.float32 and bias.dtype == torch.float32 and pre_scale is None
        return F.conv2d(x.float(), weight.reshape(weight.shape[0], 64, 1, 1), bias)

    monkeypatch.setattr(hf, "pack_conv_weights_h", pack_h)
    monkeypatch.setattr(hf, "hip_conv2d_h", conv_h)
    monkeypatch.setattr(hf, "hip_conv1x1_head", head)
    monkeypatch.setattr(uf, "hip_upsample2x_add", up)
    monkeypatch.setattr(uf, "hip_stem_conv_pool", stem)
    monkeypatch.setattr(uf, "pack_stem_weights",
                        lambda weight: torch.cat([weight.detach().permute(2, 3, 1, 0).reshape(147, 64), torch.zeros(1, 64)]))
    return uf, calls


@pytest.mark.parametrize("dtype", R.HALVES)
def test_prepare_keeps_float32_operands_through_the_cast_and_runs_the_same_graph(torch_half_kernels, dtype):
    from tiatoolbox_amd.models.architecture.hovernet_fused import _BnAct, _Conv
    from tiatoolbox_amd.models.architecture.unet import UNetModel

    uf, calls = torch_half_kernels
    torch.manual_seed(2)
    unet = UNetModel(3, 5, "resnet50", decoder_block=[3, 3]).eval()
    g = R.randomise_bn(unet, 9)
    x = torch.randint(0, 256, (1, 3, 96, 128), generator=g).float()
    with torch.inference_mode():
        ref = unet(x)
        fused = uf.FusedUNet(copy.deepcopy(unet))
        want_bias = {n: m.bias.detach().clone() for n, m in fused.named_modules() if isinstance(m, _Conv) and m.bias is not None}
        want_affine = {n: (m.scale.clone(), m.shift.clone()) for n, m in fused.named_modules() if isinstance(m, _BnAct)}
        fused.prepare(dtype)
        fused = fused.to(dtype)
        assert fused.half_dtype == dtype and fused.accepts_uint8
        assert next(fused.parameters()).dtype == dtype  # the cast happened ...
        n_conv = 0
        for name, mod in fused.named_modules():  # ... and left the float32 operands alone, bit for bit
            if isinstance(mod, _Conv) and mod is not fused.stem:
                n_conv += 1
                assert mod.half_dtype == dtype and (mod.bias is None) == (mod._bias32 is None)  # noqa: SLF001
                if mod.bias is not None:
                    assert mod.bias.dtype == dtype and mod._bias32.dtype == torch.float32  # noqa: SLF001
                    assert torch.equal(mod._bias32, want_bias[name])  # noqa: SLF001
                assert (mod._packed_h is not None and mod._packed_h.dtype == dtype) != (mod._weight32 is not None)  # noqa: SLF001
            if isinstance(mod, _BnAct):
                sc, sh = mod.affine32()
                assert sc.dtype == sh.dtype == torch.float32 and mod.scale.dtype == dtype
                assert torch.equal(sc, want_affine[name][0]) and torch.equal(sh, want_affine[name][1])
        assert n_conv == 62  # 61 MFMA convolutions + the head
        assert fused._stem_packed.dtype == torch.float32 and fused._stem_bias32.dtype == torch.float32  # noqa: SLF001
        assert torch.equal(fused._stem_bias32, want_bias["stem"])  # noqa: SLF001
        assert fused.clf._weight32.dtype == torch.float32 and fused.clf._weight32.shape == (5, 64)  # noqa: SLF001
        got = fused(x)
        got_u8 = fused(x.to(torch.uint8))
    assert calls == {"conv_h": 2 * 61, "up": 2 * 4, "head": 2, "stem": 2}
    assert got.dtype == torch.float32 and got.shape == ref.shape == (1, 5, 48, 64)
    assert torch.equal(got, got_u8)
    # every activation rounded to half once per layer: ~2^-(m+1) per layer over ~60 layers, far above any wiring mistake's reach
    assert R.rel_err(got, ref) <= (0.02 if dtype == torch.float16 else 0.15), R.rel_err(got, ref)


def test_prepare_refuses_layers_without_a_half_kernel_and_cast_modules():
    from tiatoolbox_amd.models.architecture.hovernet_fused import _Conv

    thin = _Conv(torch.nn.Conv2d(3, 64, 7, 2, 3))
    with pytest.raises(TypeError, match="no torch.float16 kernel"):
        thin.prepare(torch.float16)
    grouped = _Conv(torch.nn.Conv2d(128, 32, 3, groups=2, bias=False))  # (32 -> 8 channels per group has a half kernel)
    with pytest.raises(TypeError, match="no torch.bfloat16 kernel"):
        grouped.prepare(torch.bfloat16)
    ok = _Conv(torch.nn.Conv2d(64, 5, 1))
    with pytest.raises(ValueError, match="float32 parameters"):
        ok.half().prepare(torch.float16)  # packing after the cast would start from rounded weights
    with pytest.raises(ValueError, match="fp16 / bf16"):
        _Conv(torch.nn.Conv2d(64, 5, 1)).prepare(torch.float64)


def test_wrappers_refuse_mixed_dtypes_on_the_host():
    """Argument checks that need no device: the CUDA check comes first (no silent torch fall-back)."""
    from tiatoolbox_amd.models.architecture import fused

    x = torch.zeros((1, 64, 2, 2), dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="CUDA"):
        fused.hip_upsample2x_add(x, torch.zeros((1, 64, 4, 4), dtype=torch.float16))
    with pytest.raises(ValueError, match="channels-last CUDA"):
        fused.hip_conv1x1_head(x, torch.zeros((5, 64)), None)
    with pytest.raises(ValueError, match="CUDA"):
        fused.pack_conv_weights_h(torch.nn.Conv2d(32, 64, 1), torch.float16)

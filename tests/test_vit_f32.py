"""``compute_dtype="bfloat16x3"`` without a GPU: the exported symbols and their signatures, the exact weight split of a Linear and its
routing, the SwiGLU padding, what ``FusedViT.prepare`` and the engines refuse, and the wiring of the float32 graph on torch stand-ins
of every wrapper -- held to the float32 module (exact up to float32 summation order), with a list of wiring faults that each have to
fail the same criterion."""

from __future__ import annotations

import ctypes
import logging

import numpy as np
import pytest
import torch

from _vit_f32_ref import NEW_WRAPPERS, split_graph, torch_f32_wrappers
from _vit_ref import tiny_vit
from _vit_resid32_ref import FORMS, rel_error, torch_resid32_wrappers

ORDER_GATE = 1e-5  # float32 against the same arithmetic in another summation order: the bound test_vit_virchow.py uses against float64
P, I64, I32, F32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float


# ----------------------------------------------------------------------------------------------------------------------- symbols
def test_library_exports_the_entry_points_with_their_signatures():
    from tiatoolbox_amd import _lib, build

    want = {"tia_mha_fwd_f32": [P, P, I64, I64, I64, I64, F32, I32, P],
            "tia_gelu_rows_f32": [P, I64, P],
            "tia_swiglu_rows_f32": [P, P, I64, I64, P],
            "tia_vit_patchify_f32": [P, P, I64, I64, I64, I64, I64, P],
            "tia_vit_assemble_f32": [P, P, P, P, I32, P, I64, I64, I64, I64, P]}
    for name, args in want.items():
        assert name in _lib._SIGNATURES, name  # noqa: SLF001
        got_args, got_res = _lib._SIGNATURES[name]  # noqa: SLF001
        assert list(got_args) == args and got_res is ctypes.c_int, name
    assert build.LIB_PATH.exists(), "library not built (run __graft_entry__.build()): the new exports cannot be checked"
    lib = ctypes.CDLL(str(build.LIB_PATH))
    for name in want:
        assert hasattr(lib, name), name
    # host-side refusals need no device: nothing is dereferenced or launched
    bound = _lib.load()
    x, y = 0x10000, 0x20000  # non-null, 16-byte aligned, never read
    assert bound.tia_mha_fwd_f32(x, y, 1, 4, 2, 32, 0.125, 0, None) == _lib.TIA_ESIZE       # head_dim 32
    assert bound.tia_mha_fwd_f32(x, y, 1, 4, 2, 64, 0.125, 2, None) == _lib.TIA_EINVAL      # a half dtype code
    assert bound.tia_mha_fwd_f32(x + 4, y, 1, 4, 2, 64, 0.125, 0, None) == _lib.TIA_EINVAL  # misaligned
    assert bound.tia_mha_fwd_f32(x, y, 1, 0, 2, 64, 0.125, 0, None) == _lib.TIA_EINVAL
    assert bound.tia_gelu_rows_f32(x, 6, None) == _lib.TIA_ESIZE and bound.tia_gelu_rows_f32(None, 8, None) == _lib.TIA_EINVAL
    assert bound.tia_swiglu_rows_f32(x, y, 1, 6, None) == _lib.TIA_ESIZE
    assert bound.tia_vit_patchify_f32(x, y, 1, 28, 28, 14, 588, None) == _lib.TIA_ESIZE
    assert bound.tia_vit_assemble_f32(x, x, None, x, 1, y, 1, 4, 2, 64, None) == _lib.TIA_EINVAL  # register rows without their pointer


# --------------------------------------------------------------------------------------------------- the split, routing, padding
def test_weight_split_of_a_linear_is_exact_bit_for_bit(stand_ins, monkeypatch):
    """What the prepared graph hands the split: every ``_LinearF32`` passes ``pack_linear_weights_split`` the folded float32 weight itself
    (no rounding in front of the split), and the three planes of that weight are bf16 numbers whose float32 sum is the weight, bit
    for bit."""
    from tiatoolbox_amd.models.architecture.fused import split_stem_weights
    from tiatoolbox_amd.models.architecture.vit_fused import fold_layer_scale

    vit_fused, _ = stand_ins
    handed: list[torch.Tensor] = []
    inner = vit_fused.pack_linear_weights_split

    def recording(weight):
        handed.append(weight.clone())
        return inner(weight)

    monkeypatch.setattr(vit_fused, "pack_linear_weights_split", recording)
    vit = tiny_vit()
    fused = split_graph(vit, "cpu")
    blk = vit.blocks[0]
    own = [fold_layer_scale(linear, scale)[0] for linear, scale in ((blk.attn.qkv, None), (blk.attn.proj, blk.ls1), (blk.mlp.fc1, None),
                                                                     (blk.mlp.fc2, blk.ls2))]
    assert len(handed) == 1 + 4 * len(vit.blocks)  # the patch embedding, then qkv, proj, fc1, fc2 of every block
    for w, got, name in zip(own, handed[1:5], ("qkv", "proj", "fc1", "fc2")):
        assert torch.equal(got.view(torch.int32), w.view(torch.int32)), name
        lin = fused.layers[0][name]
        assert type(lin).__name__ == "_LinearF32" and lin.split and lin.weight32 is None and lin.packed.dtype == torch.bfloat16
        parts, usable = split_stem_weights(got)
        assert usable and parts.shape == (3, *w.shape)
        assert torch.equal(parts.to(torch.bfloat16).float(), parts)  # every plane holds bf16 numbers
        total = (parts[0] + parts[1]) + parts[2]  # float32 adds: both are exact
        assert torch.equal(total.view(torch.int32), w.view(torch.int32))
        assert bool((parts[2] != 0).any())  # (the third plane is not idle: 24 significant bits need all three)
        assert torch.equal(lin.packed.float(), parts)  # (what the stand-in keeps for the GEMM: the same three planes)


@pytest.fixture
def stand_ins(monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    calls: dict = {}
    for name, fn in {**torch_resid32_wrappers(calls), **torch_f32_wrappers(calls)}.items():
        monkeypatch.setattr(vit_fused, name, fn)
    return vit_fused, calls


def test_an_unsplittable_weight_routes_its_layer_to_the_float32_kernel(stand_ins, caplog):
    """1e-36 has no split into NORMAL bf16 numbers (its third part is below 2^-126): that layer, and only that one, takes the float32
    GEMM, and one ``info`` line names it."""
    vit = tiny_vit()
    with torch.no_grad():
        vit.blocks[1].mlp.fc1.weight[3, 5] = 1e-36
    with caplog.at_level(logging.INFO, logger="tiatoolbox_amd"):
        fused = split_graph(vit, "cpu")
    kinds = {lin.name: lin.split for layer in fused.layers for lin in (layer["qkv"], layer["proj"], layer["fc1"], layer["fc2"])}
    kinds[fused.patch.name] = fused.patch.split
    assert [name for name, split in kinds.items() if not split] == ["blocks.1.mlp.fc1"] and len(kinds) == 9
    said = [r.getMessage() for r in caplog.records if "split-bf16 GEMM" in r.getMessage()]
    assert len(said) == 1 and "blocks.1.mlp.fc1 (128 -> 512)" in said[0] and "tia_conv2d_nhwc_f32" in said[0] and "1 layer(s)" in said[0]
    assert fused.layers[1]["fc1"].packed.dtype == torch.float32 and fused.layers[0]["fc1"].packed.dtype == torch.bfloat16
    assert fused.linear_dtype == "bfloat16x3" and fused.half_dtype is None and fused.residual_dtype is None
    x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert rel_error(fused(x), vit(x)) <= ORDER_GATE


def test_swiglu_padding_to_the_split_kernels_multiple_is_exact_zeros(stand_ins):
    """Virchow's shape in small: H = 520 is padded to 544 by the constructor (the half GEMM's 32) and ``fc1`` = 1088 is off the split
    kernel's 128: each half goes to 576, ``fc1`` to 1152, with zero rows, zero bias and zero ``fc2`` columns -- and the real lanes
    keep their bits."""
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT, fold_layer_scale

    build, _ = FORMS["tiny-v2"]
    vit = build()
    fused = FusedViT(vit)
    before = [(layer["fc1"].weight32.clone(), layer["fc1"].bias32.clone(), layer["fc2"].weight32.clone()) for layer in fused.layers]
    assert before[0][0].shape == (1088, 320)
    fused.prepare(torch.float32, linear_dtype="bfloat16x3")
    for i, layer in enumerate(fused.layers):
        fc1, fc2 = layer["fc1"], layer["fc2"]
        assert (fc1.cout, fc1.cin, fc2.cout, fc2.cin) == (1152, 320, 320, 576) and fc1.split and not fc2.split  # (320 % 128 != 0)
        w1 = fc1.packed.double().sum(0).float()  # (the stand-in keeps the three planes)
        w2 = fc2.packed.reshape(576, 320).T
        own1, own_b1 = fold_layer_scale(vit.blocks[i].mlp.fc1, None)
        own2, _ = fold_layer_scale(vit.blocks[i].mlp.fc2, vit.blocks[i].ls2)
        for lo, src_w, src_b in ((0, own1[:520], own_b1[:520]), (576, own1[520:], own_b1[520:])):
            assert torch.equal(w1[lo:lo + 520], src_w) and torch.equal(fc1.bias32[lo:lo + 520], src_b)
        for lo, hi in ((520, 576), (1096, 1152)):
            assert bool((w1[lo:hi] == 0).all()) and bool((fc1.bias32[lo:hi] == 0).all())
        assert torch.equal(w2[:, :520], own2) and bool((w2[:, 520:] == 0).all())
    # a half below the pad floor is left alone (and then keeps the float32 kernel if it is off the multiple)
    small = FusedViT(FORMS["tiny-reg-swiglu"][0]())
    small.prepare(torch.float32, linear_dtype="bfloat16x3")
    assert small.layers[0]["fc1"].cout == 512 and small.layers[0]["fc2"].cin == 256


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_prepare_refusals_stay_and_the_new_ones_come_before_any_device_work():
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    with pytest.raises(ValueError, match="float16 or bfloat16"):
        FusedViT(tiny_vit()).prepare(torch.float32)
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        FusedViT(tiny_vit()).prepare(torch.float32, linear_dtype="float8_e4m3")
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        FusedViT(tiny_vit()).prepare(torch.float32, residual_dtype="float32")
    with pytest.raises(ValueError, match="float16 or bfloat16"):  # the stream of the float32 route is float32 already
        FusedViT(tiny_vit()).prepare(torch.float32, linear_dtype="bfloat16x3", residual_dtype="float32")
    for half in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="bfloat16x3.*float32 route"):
            FusedViT(tiny_vit()).prepare(half, linear_dtype="bfloat16x3")
    fused = FusedViT(tiny_vit())
    assert fused.linear_dtype is None and fused.half_dtype is None
    with pytest.raises(RuntimeError, match="prepare"):
        fused(torch.zeros((1, 3, 32, 32)))


def test_prepare_packs_once(stand_ins):
    fused = split_graph(tiny_vit(), "cpu")
    with pytest.raises(ValueError, match="packs once"):
        fused.prepare(torch.float32, linear_dtype="bfloat16x3")
    with pytest.raises(ValueError, match="packs once"):
        fused.prepare(torch.bfloat16)
    with pytest.raises(RuntimeError, match="uint8"):
        fused.forward_uint8(torch.zeros((1, 32, 32, 3), dtype=torch.uint8), torch.zeros((256, 3)))


def _patches(n: int = 2) -> np.ndarray:
    return np.random.default_rng(0).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def _vit_engine():
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone("vit_small_patch16_224")
    model.feat_extract = tiny_vit(img_size=224, dynamic=False)
    return DeepFeatureExtractor(model, batch_size=2)  # device="cpu"


def test_engine_refuses_the_option_on_the_cpu_and_forgets_it():
    eng = _vit_engine()
    with pytest.raises(ValueError, match="bfloat16x3.*Vision Transformer.*CUDA"):
        eng.run(_patches(), patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16x3")
    assert eng.compute_dtype == "float32"  # the refused value is not left behind for the next run
    assert eng.run(_patches(), patch_mode=True, ioconfig=_cfg())["probabilities"].shape == (2, 128)


def test_engine_refuses_the_option_for_a_cnn():
    from tiatoolbox_amd.models import PatchPredictor

    eng = PatchPredictor("resnet18-kather100k", batch_size=2)
    with pytest.raises(ValueError, match="bfloat16x3.*Vision Transformer"):
        eng.run(_patches(), patch_mode=True, compute_dtype="bfloat16x3")
    assert eng.compute_dtype == "float32"


def test_engine_refuses_residual_dtype_beside_the_option_and_keys_its_copy(monkeypatch):
    """On an engine that believes it is on a CUDA device (no device is touched: the refusal comes first, and a new copy starts with
    ``deepcopy``, which stops the call)."""
    from tiatoolbox_amd.models.engine import engine_abc

    assert engine_abc._carrier_dtype("bfloat16x3") == torch.float32  # noqa: SLF001  (a float32 carrier, as FP8's is bfloat16)
    eng = _vit_engine()
    eng.device = "cuda"
    eng.compute_dtype, eng.residual_dtype = "bfloat16x3", "float32"
    with pytest.raises(ValueError, match="bfloat16x3.*without residual_dtype"):
        eng._inference_model(torch.float32)  # noqa: SLF001
    assert eng.compute_dtype == "float32" and eng.residual_dtype is None

    class Stop(Exception):
        pass

    def deepcopy(_):
        raise Stop

    monkeypatch.setattr("copy.deepcopy", deepcopy)
    cached = object()
    eng._fast_model = cached  # noqa: SLF001
    eng._fast_key = (torch.float32, "cuda", id(eng.model), eng.fold_batchnorm, engine_abc._weights_version(eng.model),  # noqa: SLF001
                     "winograd", False, None)  # the key of a compute_dtype="float32" run
    assert eng._inference_model(torch.float32) is cached  # noqa: SLF001
    eng.compute_dtype = "bfloat16x3"
    with pytest.raises(Stop):  # the option never shares the float32 module's copy
        eng._inference_model(torch.float32)  # noqa: SLF001


# ------------------------------------------------------------------------------------------------------------------- the wiring
def _case(form: str):
    build, side = FORMS[form]
    vit = build()
    x = torch.randn((2, 3, side, side), generator=torch.Generator().manual_seed(side))
    return vit, x


@pytest.mark.parametrize("form", list(FORMS))
def test_stand_in_graph_matches_the_float32_module(form, stand_ins):
    _, calls = stand_ins
    vit, x = _case(form)
    with torch.no_grad():
        got, ref = split_graph(vit, "cpu")(x), vit(x)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    e = rel_error(got, ref)
    print(f"stand-ins {form}: e against the float32 module {e:.3e}")
    assert e <= ORDER_GATE
    depth, pooled = len(vit.blocks), vit.global_pool == "token_mean"
    assert calls["hip_vit_patchify_f32"] == 1 and calls["hip_vit_assemble_f32"] == 1 and calls["hip_mha_fwd_f32"] == depth
    assert calls["hip_linear_f32"] == 1 + 4 * depth and calls["hip_add_layernorm_rows_f32"] == 2 * depth + (0 if pooled else 1)
    assert calls.get("hip_vit_cls_mean_pool_f32", 0) == int(pooled)
    assert calls.get("hip_swiglu_rows_f32", 0) + calls.get("hip_gelu_rows_f32_", 0) == depth
    assert "hip_vit_assemble_rows_f32" not in calls  # (the half-token form belongs to residual_dtype="float32")


def test_classifier_works_unchanged_on_the_route(stand_ins):
    from _vit_classifier_ref import timm_model

    from tiatoolbox_amd.models.architecture import vit_fused

    model = timm_model()
    fused = vit_fused.FusedViTClassifier(model)
    fused.feat_extract.prepare(torch.float32, linear_dtype="bfloat16x3")
    monkey_head = lambda x, w, b: torch.softmax(torch.nn.functional.linear(x, w, b), -1)  # noqa: E731
    vit_fused.hip_linear_softmax_rows_f32, keep = monkey_head, vit_fused.hip_linear_softmax_rows_f32
    try:
        x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(3))
        with torch.no_grad():
            got, ref = fused(x), model(x)
    finally:
        vit_fused.hip_linear_softmax_rows_f32 = keep
    assert fused.half_dtype is None and float((got - ref).abs().max()) <= ORDER_GATE


# each fault changes the prepared graph or wraps the installed stand-ins
def _wrap(vit_fused, monkeypatch, name, make):
    monkeypatch.setattr(vit_fused, name, make(getattr(vit_fused, name)))


def _missing_residual(which: int):
    """The GEMM's calls in order: patch (0), then qkv, proj, fc1, fc2 of block 0 (1 .. 4): call ``which`` loses its residual."""
    def fault(fused, vit_fused, monkeypatch):  # noqa: ARG001
        state = {"calls": 0}

        def make(fn):
            def wrapper(x, w, bias, residual=None, *, cout):
                i, state["calls"] = state["calls"], state["calls"] + 1
                return fn(x, w, bias, None if i == which else residual, cout=cout)
            return wrapper
        _wrap(vit_fused, monkeypatch, "hip_linear_f32", make)
    return fault


def _swapped_gate(fused, vit_fused, monkeypatch):  # noqa: ARG001
    _wrap(vit_fused, monkeypatch, "hip_swiglu_rows_f32", lambda fn: lambda x: fn(torch.cat([x[..., x.shape[-1] // 2:], x[..., :x.shape[-1] // 2]], -1)))


def _wrong_skip(fused, vit_fused, monkeypatch):  # noqa: ARG001
    _wrap(vit_fused, monkeypatch, "hip_vit_cls_mean_pool_f32",
          lambda fn: lambda x, branch, gamma, beta, **kw: fn(x, branch, gamma, beta, **{**kw, "skip": 1}))


def _wrong_scale(fused, vit_fused, monkeypatch):  # noqa: ARG001
    _wrap(vit_fused, monkeypatch, "hip_mha_fwd_f32", lambda fn: lambda qkv, heads, scale: fn(qkv, heads, scale * scale))  # 1 / hd


def _norms_swapped(fused, vit_fused, monkeypatch):  # noqa: ARG001
    layer = fused.layers[0]
    layer["norm1"], layer["norm2"] = layer["norm2"], layer["norm1"]


def _last_block_left_out(fused, vit_fused, monkeypatch):  # noqa: ARG001
    fused.layers = fused.layers[:-1]  # the final norm (or pool) reads the stream before the last block


FAULTS = {"proj-without-its-residual": (_missing_residual(2), None), "fc2-without-its-residual": (_missing_residual(4), None),
          "swapped-gate-half": (_swapped_gate, "swiglu"), "wrong-prefix-skip": (_wrong_skip, "registers+pool"),
          "wrong-scale": (_wrong_scale, None), "norm1-norm2-swapped": (_norms_swapped, None),
          "last-block-left-out": (_last_block_left_out, None)}
FAULT_CASES = [(fault, form) for fault, (_, needs) in FAULTS.items() for form in FORMS
               if needs is None or (needs == "swiglu" and form != "tiny") or (needs == "registers+pool" and form == "tiny-v2")]


@pytest.mark.parametrize(("fault", "form"), FAULT_CASES)
def test_each_wiring_fault_fails_the_criterion(fault, form, stand_ins, monkeypatch):
    vit_fused, _ = stand_ins
    vit, x = _case(form)
    fused = split_graph(vit, "cpu")
    FAULTS[fault][0](fused, vit_fused, monkeypatch)
    with torch.no_grad():
        e = rel_error(fused(x), vit(x))
    print(f"fault {fault} {form}: e {e:.3e} ({e / ORDER_GATE:.0f} x the gate)")
    assert e > ORDER_GATE


def test_the_half_routes_call_none_of_the_new_wrappers(monkeypatch):
    """Every existing route returns what it returned: ``prepare(torch.bfloat16)`` reaches none of the float32 route's wrappers -- they
    are replaced by functions that fail."""
    from _vit_classifier_ref import torch_vit_wrappers

    from tiatoolbox_amd.models.architecture import vit_fused

    def fail(*_a, **_k):
        raise AssertionError("a wrapper of the float32 route was called on a half route")

    for name, fn in torch_vit_wrappers({}).items():
        monkeypatch.setattr(vit_fused, name, fn)
    for name in NEW_WRAPPERS:
        monkeypatch.setattr(vit_fused, name, fail)
    vit = tiny_vit()
    fused = vit_fused.FusedViT(vit)
    fused.prepare(torch.bfloat16)
    assert fused.linear_dtype is None and all(type(layer[n]).__name__ == "_Linear" for layer in fused.layers for n in ("qkv", "proj", "fc1", "fc2"))
    x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(0))
    with torch.inference_mode():
        assert fused(x).dtype == torch.float32

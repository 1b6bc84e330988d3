"""``residual_dtype="float32"`` without a GPU: the exported symbols, what ``FusedViT.prepare`` and the engines refuse, and the wiring of
the new graph on torch stand-ins of every wrapper -- held to the float32 module under ``torch.autocast`` (the arithmetic the option
restates), with a list of wiring faults that each have to fail the same criterion."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from _vit_classifier_ref import torch_vit_wrappers
from _vit_ref import tiny_vit
from _vit_resid32_ref import (FORMS, NEW_WRAPPERS, autocast_features, fused_graph, ref64, rel_error, torch_resid32_wrappers)

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


# --------------------------------------------------------------------------------------------------------------- symbols, refusals
def test_library_exports_the_three_entry_points():
    from tiatoolbox_amd import _lib, build

    if not build.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(str(build.LIB_PATH))
    for name in ("tia_add_layernorm_rows_f32", "tia_vit_assemble_rows_f32", "tia_vit_cls_mean_pool_f32"):
        assert hasattr(lib, name) and name in _lib._SIGNATURES, name  # noqa: SLF001


def test_prepare_takes_the_keyword_and_refuses_before_any_device_work():
    """On a CPU-built ``FusedViT``: every refusal is a ``ValueError`` although no device (and no packing) is within reach."""
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    for bad in ("float16", "bfloat16", "fp32", torch.float32):
        with pytest.raises(ValueError, match="residual_dtype"):
            FusedViT(tiny_vit()).prepare(torch.bfloat16, residual_dtype=bad)
    with pytest.raises(ValueError, match="float32-input quantising LayerNorm"):
        FusedViT(tiny_vit()).prepare(torch.bfloat16, linear_dtype="float8_e4m3", residual_dtype="float32")
    with pytest.raises(ValueError, match="float16 or bfloat16"):  # the pinned refusal comes first, with or without the argument
        FusedViT(tiny_vit()).prepare(torch.float32, residual_dtype="float32")
    fused = FusedViT(tiny_vit())
    assert fused.residual_dtype is None and fused.half_dtype is None  # nothing was prepared by the refused calls' kin


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


@pytest.mark.parametrize("compute", [None, "bfloat16", "float32", "float8_e4m3"])
def test_engine_refuses_the_option_on_the_cpu_and_forgets_it(compute):
    eng = _vit_engine()
    assert eng.residual_dtype is None
    kw = {} if compute is None else {"compute_dtype": compute}
    with pytest.raises(ValueError, match="residual_dtype.*Vision Transformer.*CUDA"):
        eng.run(_patches(), patch_mode=True, ioconfig=_cfg(), residual_dtype="float32", **kw)
    assert eng.residual_dtype is None  # the refused value is not left behind for the next run
    if compute in (None, "float32"):
        assert eng.run(_patches(), patch_mode=True, ioconfig=_cfg())["probabilities"].shape == (2, 128)


def test_engine_refuses_the_option_for_a_cnn_and_unknown_values():
    from tiatoolbox_amd.models import PatchPredictor

    eng = PatchPredictor("resnet18-kather100k", batch_size=2)
    with pytest.raises(ValueError, match="residual_dtype.*Vision Transformer"):
        eng.run(_patches(), patch_mode=True, compute_dtype="bfloat16", residual_dtype="float32")
    assert eng.residual_dtype is None
    eng = _vit_engine()
    with pytest.raises(ValueError, match="residual_dtype='bfloat16'"):
        eng.run(_patches(), patch_mode=True, ioconfig=_cfg(), residual_dtype="bfloat16")
    assert eng.residual_dtype is None


def test_the_option_is_part_of_the_inference_copy_key(monkeypatch):
    """Two values of the option never share an inference copy: the key that ``_inference_model`` compares carries it."""
    from tiatoolbox_amd.models.engine import engine_abc

    eng = _vit_engine()
    eng.device = "cuda"  # (no device is touched: a new copy starts with `deepcopy`, which stops the call)

    class Stop(Exception):
        pass

    def deepcopy(_):
        raise Stop

    monkeypatch.setattr("copy.deepcopy", deepcopy)
    cached = object()
    eng._fast_model = cached  # noqa: SLF001
    eng._fast_key = (torch.bfloat16, "cuda", id(eng.model), eng.fold_batchnorm, engine_abc._weights_version(eng.model),  # noqa: SLF001
                     "winograd", False, None)  # the default run's key
    assert eng._inference_model(torch.bfloat16) is cached  # noqa: SLF001  (the default: the cached copy)
    eng.residual_dtype = "float32"
    with pytest.raises(Stop):  # another value: a copy of its own is built
        eng._inference_model(torch.bfloat16)  # noqa: SLF001


# ------------------------------------------------------------------------------------------------------------------- the wiring
def _stand_ins(monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    calls: dict = {}
    for name, fn in {**torch_vit_wrappers(calls), **torch_resid32_wrappers(calls)}.items():
        monkeypatch.setattr(vit_fused, name, fn)
    return vit_fused, calls


def _case(form: str):
    build, side = FORMS[form]
    vit = build()
    x = torch.randn((2, 3, side, side), generator=torch.Generator().manual_seed(side))
    return vit, x


def _errors(vit, x, dtype, **prepare) -> tuple[float, float]:
    """``(e of the stand-in graph, e of the autocast module)`` against the form's float64 reference."""
    ref = ref64(vit, x)
    with torch.no_grad():
        got = fused_graph(vit, dtype, "cpu", **prepare)(x)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    return rel_error(got, ref), rel_error(autocast_features(vit, x, dtype, "cpu"), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["tiny", "tiny-reg-swiglu", "tiny-v2"])
def test_stand_in_graph_matches_autocast(form, dtype, monkeypatch):
    _, calls = _stand_ins(monkeypatch)
    vit, x = _case(form)
    e_new, e_yard = _errors(vit, x, dtype, residual_dtype="float32")
    print(f"stand-ins {form} {dtype}: e_new {e_new:.3e}  e_autocast {e_yard:.3e}")
    assert e_new <= 2.0 * e_yard
    depth = len(vit.blocks)
    pooled = vit.global_pool == "token_mean"
    assert calls["hip_vit_assemble_rows_f32"] == 1 and calls["hip_add_layernorm_rows_f32"] == 2 * depth + (0 if pooled else 1)
    assert calls.get("hip_vit_cls_mean_pool_f32", 0) == int(pooled)


# each fault wraps the installed stand-ins; `state` is shared between the wrappers of one fault
def _wrap(monkeypatch, vit_fused, name, make):
    monkeypatch.setattr(vit_fused, name, make(getattr(vit_fused, name)))


def _branch_twice(monkeypatch, vit_fused):
    def make(fn):
        def wrapper(x, branch, gamma, beta, **kw):
            if branch is not None:
                fn(x, branch, None, None, **{**kw, "out_dtype": None})  # the add alone, once more
            return fn(x, branch, gamma, beta, **kw)
        return wrapper
    _wrap(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32", make)


def _not_written_back(monkeypatch, vit_fused):
    _wrap(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32",
          lambda fn: lambda x, branch, gamma, beta, **kw: fn(x.clone(), branch, gamma, beta, **kw))


def _norm_before_add(monkeypatch, vit_fused):
    def make(fn):
        def wrapper(x, branch, gamma, beta, **kw):
            if branch is None:
                return fn(x, None, gamma, beta, **kw)
            y = fn(x, None, gamma, beta, **kw)
            fn(x, branch, None, None, **{**kw, "out_dtype": None})
            return y
        return wrapper
    _wrap(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32", make)


def _last_branch_left_out(monkeypatch, vit_fused):
    def make(fn):
        def wrapper(x, branch, gamma, beta, **kw):
            final = kw.get("out_dtype") == torch.float32
            return fn(x, None if final else branch, gamma, beta, **kw)
        return wrapper
    _wrap(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32", make)
    _wrap(monkeypatch, vit_fused, "hip_vit_cls_mean_pool_f32", lambda fn: lambda x, branch, gamma, beta, **kw: fn(x, None, gamma, beta, **kw))  # noqa: ARG005


def _residual_kept(which: int):
    """The half GEMM's calls in order: patch (0), then qkv, proj, fc1, fc2 of block 0 (1 .. 4): call ``which`` is still handed the
    stream (rounded to the half type) as its residual."""
    def fault(monkeypatch, vit_fused):
        state = {"calls": 0}

        def make_norm(fn):
            def wrapper(x, branch, gamma, beta, **kw):
                state["x"] = x
                return fn(x, branch, gamma, beta, **kw)
            return wrapper

        def make_linear(fn):
            def wrapper(a, w, bias, residual=None, *, cout):
                i, state["calls"] = state["calls"], state["calls"] + 1
                if i == which:
                    residual = state["x"].to(a.dtype)
                return fn(a, w, bias, residual, cout=cout)
            return wrapper

        _wrap(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32", make_norm)
        _wrap(monkeypatch, vit_fused, "hip_linear_h", make_linear)
    return fault


FAULTS = {"branch-added-twice": _branch_twice, "x32-not-written-back": _not_written_back, "layernorm-before-the-add": _norm_before_add,
          "last-branch-left-out": _last_branch_left_out, "proj-keeps-its-residual": _residual_kept(2),
          "fc2-keeps-its-residual": _residual_kept(4)}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["tiny", "tiny-v2"])  # (the class-row end and the pooled end of the graph)
@pytest.mark.parametrize("fault", list(FAULTS))
def test_each_wiring_fault_fails_the_criterion(fault, form, dtype, monkeypatch):
    vit_fused, _ = _stand_ins(monkeypatch)
    FAULTS[fault](monkeypatch, vit_fused)
    vit, x = _case(form)
    e_fault, e_yard = _errors(vit, x, dtype, residual_dtype="float32")
    print(f"fault {fault} {form} {dtype}: e_fault {e_fault:.3e}  e_autocast {e_yard:.3e}  ratio {e_fault / e_yard:.1f}")
    assert e_fault > 2.0 * e_yard


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["tiny", "tiny-v2"])
def test_none_is_the_graph_built_without_the_keyword(form, dtype, monkeypatch):
    _, calls = _stand_ins(monkeypatch)
    vit, x = _case(form)
    with torch.no_grad():
        plain = fused_graph(vit, dtype, "cpu")(x)
        given = fused_graph(vit, dtype, "cpu", residual_dtype=None)(x)
    assert torch.equal(plain, given)
    assert not any(name in calls for name in NEW_WRAPPERS)

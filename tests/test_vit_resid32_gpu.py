"""``FusedViT`` with ``residual_dtype="float32"`` on the GPU: parity with the float32 module on the CPU, the float32 module under
``torch.autocast`` on the same device as the yardstick (the module with a float32 residual stream); what the option buys at a small
LayerScale; the default graph unchanged; the input forms, the engines' route to it and what it launches."""

from __future__ import annotations

import copy
import functools
import logging

import numpy as np
import pytest
import torch

from _vit_classifier_ref import timm_model
from _vit_foundation_ref import TINY_REG, tiny_foundation
from _vit_ref import forward64, randomise, tiny_vit
from _vit_resid32_ref import autocast_features, cast_features, fused_graph, rel_error, scale_layer_scale
from _vit_virchow_ref import TINY_V1, TINY_V2, tiny_virchow
from test_vit_gpu import _mha_head_dims

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
NAME = "vit_small_patch16_224"
NEW_KERNELS = ("add_layernorm_rows_f32_kernel", "vit_assemble_rows_f32_kernel", "vit_cls_mean_pool_f32_kernel")
REPLACED = ("layernorm_rows_h_kernel", "vit_assemble_tokens_h_kernel", "vit_assemble_prefix_h_kernel", "vit_cls_mean_pool_h_kernel")

BUILDERS = {
    "tiny": lambda: tiny_vit(layer_scale=False),
    "tiny-ls": lambda: tiny_vit(layer_scale=True),
    "tiny-reg-swiglu": lambda: tiny_foundation(TINY_REG),  # register tokens, no class entry, p = 14, packed SwiGLU
    "tiny-v1": lambda: tiny_virchow(TINY_V1),              # token_mean, padded SwiGLU
    "tiny-v2": lambda: tiny_virchow(TINY_V2),              # and prefix_pos_embed
    "uni-width": lambda: tiny_vit(layer_scale=True, embed_dim=1024, num_heads=16, mlp_dim=4096, img_size=224),
    "virchow2-width": lambda: tiny_virchow(TINY_V2, embed_dim=1280, num_heads=16, mlp_dim=6832, reg_tokens=4, img_size=224, depth=1),
}


@functools.lru_cache(maxsize=None)
def _case(form: str, n: int, h: int, w: int):
    """(the module, the batch, the float32 module's features on the CPU): computed once, shared by both half types, left unchanged."""
    vit = BUILDERS[form]()
    x = torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(h + w + n))
    with torch.inference_mode():
        ref = vit(x).double()
    return vit, x, ref


def _run(fused, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    with torch.inference_mode():
        return fused(x.cuda().to(dtype).contiguous(memory_format=torch.channels_last))  # what `infer_batch` hands over


def _parity(form: str, n: int, h: int, w: int, dtype: torch.dtype) -> None:
    """``e = max |feat - ref| / max(max |ref|, 1)``: the option's graph at most twice the error of the autocast module."""
    vit, x, ref = _case(form, n, h, w)
    got = _run(fused_graph(vit, dtype, "cuda", residual_dtype="float32"), x, dtype)
    assert got.shape == ref.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    e_new, e_yard = rel_error(got, ref), rel_error(autocast_features(vit, x, dtype, "cuda"), ref)
    print(f"resid32 {form} n={n} {h}x{w} {dtype}: e_new {e_new:.3e}  e_autocast {e_yard:.3e}")
    assert e_new <= 2.0 * e_yard


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["tiny", "tiny-ls"])
@pytest.mark.parametrize("size", [32, 64, 224])
@pytest.mark.parametrize("n", [1, 3])
def test_graph_matches_module(n, size, form, dtype):
    _parity(form, n, size, size, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize(("form", "n", "h", "w"), [("tiny-ls", 2, 48, 64), ("tiny-reg-swiglu", 2, 28, 28), ("tiny-reg-swiglu", 1, 42, 28),
                                                    ("tiny-v1", 3, 28, 28), ("tiny-v2", 3, 28, 28), ("tiny-v2", 1, 42, 56),
                                                    ("uni-width", 2, 224, 224), ("virchow2-width", 1, 224, 224)])
def test_graph_matches_module_in_every_form(form, n, h, w, dtype):
    _parity(form, n, h, w, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_float32_stream_keeps_small_layer_scale_updates(dtype):
    """What the option is for.  Depth 8 with every LayerScale gamma at 0.01 x U(0.5, 1.5): a branch update of that size beside an ``x``
    of order 1 is near or below half a unit of the half type, and a half residual stream rounds most of it away.  ``r_new = e_f32 /
    e_half`` of the two ``FusedViT`` graphs from the same weights, beside ``r_yard = e_autocast / e_cast`` of the two torch modules on
    the same device, all four against ``forward64``: ``r_new <= 4 r_yard`` (the usual factor 2 on each term of the ratio) and
    ``r_new <= 0.25`` (a condition: on the CPU the yardstick pair alone gives 0.014 in bf16 and 0.024 in fp16)."""
    vit = scale_layer_scale(tiny_vit(layer_scale=True, depth=8), 0.01)
    x = torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(64))
    ref = forward64(vit.state_dict(), x, heads=vit.num_heads, patch=vit.patch_size, native_grid=vit.native_grid)
    e_half = rel_error(_run(fused_graph(vit, dtype, "cuda"), x, dtype), ref)
    e_f32 = rel_error(_run(fused_graph(vit, dtype, "cuda", residual_dtype="float32"), x, dtype), ref)
    e_cast, e_auto = rel_error(cast_features(vit, x, dtype, "cuda"), ref), rel_error(autocast_features(vit, x, dtype, "cuda"), ref)
    r_new, r_yard = e_f32 / e_half, e_auto / e_cast
    print(f"resid32 benefit {dtype}: e_half {e_half:.3e}  e_f32 {e_f32:.3e}  e_cast {e_cast:.3e}  e_autocast {e_auto:.3e}  "
          f"r_new {r_new:.4f}  r_yard {r_yard:.4f}")
    assert r_new <= 4.0 * r_yard and r_new <= 0.25  # noqa: PLR2004


def _device_kernels(fn) -> set:
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()}
    return {n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()}


def _banned(name: str) -> bool:
    low = name.lower()
    return any(b in low for b in ("cijk_", "rocblas", "hipblaslt", "gemm", "fmha", "miopen")) or ("attention" in low and "ck" in low)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["tiny-ls", "tiny-v2"])
def test_none_is_the_default_graph(form, dtype):
    """``prepare(dtype)`` and ``prepare(dtype, residual_dtype=None)``: the same bits from the same kernels, none of them new."""
    side = 32 if form == "tiny-ls" else 28
    vit, x, _ = _case(form, 3, side, side)
    plain, given = fused_graph(vit, dtype, "cuda"), fused_graph(vit, dtype, "cuda", residual_dtype=None)
    assert given.residual_dtype is None and torch.equal(_run(plain, x, dtype), _run(given, x, dtype))
    k_plain, k_given = _device_kernels(lambda: _run(plain, x, dtype)), _device_kernels(lambda: _run(given, x, dtype))
    assert k_plain == k_given and not [k for k in k_given if any(new in k for new in NEW_KERNELS)], k_given
    wanted = (["vit_patchify_h_kernel", "vit_assemble_tokens_h_kernel", "gelu_rows_h_kernel", "mha_fwd_h_kernel"] if form == "tiny-ls" else
              ["vit_patchify_pad_h_kernel", "vit_assemble_prefix_h_kernel", "swiglu_rows_h_kernel", "vit_cls_mean_pool_h_kernel",
               "mha_fwd_h_kernel"])
    for name in [*wanted, "layernorm_rows_h_kernel", "conv_mfma_h"]:
        assert any(name in k for k in k_given), (name, k_given)
    assert _mha_head_dims(k_given) == ({64} if form == "tiny-ls" else {80}), k_given  # (80 dimensions per head: the attention kernel's other instantiation)


@pytest.mark.parametrize("form", ["tiny-ls", "tiny-v2"])
def test_forward_launches_the_new_kernels_and_none_they_replace(form):
    side = 32 if form == "tiny-ls" else 28
    vit, x, _ = _case(form, 3, side, side)
    fused = fused_graph(vit, torch.bfloat16, "cuda", residual_dtype="float32")
    _run(fused, x, torch.bfloat16)
    kernels = _device_kernels(lambda: _run(fused, x, torch.bfloat16))
    for wanted in NEW_KERNELS[:2] if form == "tiny-ls" else NEW_KERNELS:
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert not [k for k in kernels if any(old in k for old in REPLACED)], kernels
    assert not {k for k in kernels if _banned(k)}, kernels
    for wanted in ("mha_fwd_h_kernel", "conv_mfma_h"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert _mha_head_dims(kernels) == ({64} if form == "tiny-ls" else {80}), kernels


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["tiny-ls", "tiny-v2"])
def test_forward_uint8_is_forward_of_the_hooks_batch(form, dtype):
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    side = 32 if form == "tiny-ls" else 28
    vit, _, _ = _case(form, 3, side, side)
    hook = timm_preproc_func("Virchow2" if form == "tiny-v2" else NAME)
    fused = fused_graph(vit, dtype, "cuda", residual_dtype="float32")
    x = torch.from_numpy(np.random.default_rng(side).integers(0, 256, (3, side, side, 3), dtype=np.uint8)).cuda()
    with torch.inference_mode():
        got = fused.forward_uint8(x, hook.device_table("cuda", dtype))
        assert got.dtype == torch.float32 and torch.equal(got, fused(hook.device_batch(x, dtype).permute(0, 3, 1, 2)))


# ------------------------------------------------------------------------------------------------------------------------- engines
def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def _rule(got: np.ndarray, yard: np.ndarray, ref: np.ndarray, what: str) -> None:
    scale = max(float(np.abs(ref).max()), 1.0)
    e_new, e_yard = float(np.abs(got - ref).max()) / scale, float(np.abs(yard - ref).max()) / scale
    print(f"{what}: e_new {e_new:.3e}  e_autocast {e_yard:.3e}")
    assert got.shape == ref.shape and got.dtype == np.float32 and bool(np.isfinite(got).all()) and e_new <= 2.0 * e_yard


def test_feature_extractor_runs_the_option_and_keys_its_copy_on_it():
    from tiatoolbox_amd.models import DeepFeatureExtractor

    patches = np.random.default_rng(0).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    cpu = DeepFeatureExtractor(NAME, batch_size=2)
    randomise(cpu.model.feat_extract)
    ref = cpu.run(patches, patch_mode=True, ioconfig=_cfg())["probabilities"]
    eng = DeepFeatureExtractor(copy.deepcopy(cpu.model), batch_size=2, device="cuda")
    got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16", residual_dtype="float32")["probabilities"]
    fast = eng._inference_model(torch.bfloat16)  # noqa: SLF001  (the cached copy the run used)
    assert eng.residual_dtype == "float32" and [m.residual_dtype for m in fast.modules() if type(m).__name__ == "FusedViT"] == ["float32"]
    x = torch.from_numpy(patches).float().permute(0, 3, 1, 2)
    with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):
        yard = copy.deepcopy(cpu.model).cuda()(x.cuda()).float().cpu().numpy()
    assert got.shape == (3, 384)
    _rule(got, yard, ref, "DeepFeatureExtractor vit_small bf16 residual float32")
    # run kwargs persist: the option is switched off by name, and the copy of the default graph is another one
    back = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16", residual_dtype=None)["probabilities"]
    plain = DeepFeatureExtractor(copy.deepcopy(cpu.model), batch_size=2, device="cuda").run(
        patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")["probabilities"]
    assert np.array_equal(back, plain) and not np.array_equal(back, got)


@pytest.mark.parametrize(("name", "dtype"), [("float16", torch.float16), ("bfloat16", torch.bfloat16)], ids=IDS)
def test_patch_predictor_runs_the_option_from_bytes_to_probabilities(name, dtype):
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViTClassifier
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    model = timm_model(tiny_vit(img_size=224, dynamic=False), num_classes=9)
    model.preproc_func = hook = timm_preproc_func(NAME)
    patches = np.random.default_rng(8).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    ref = PatchPredictor(copy.deepcopy(model), batch_size=2).run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True)
    eng = PatchPredictor(copy.deepcopy(model), batch_size=2, device="cuda")
    out = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype=name, residual_dtype="float32")
    fast = eng._inference_model(dtype)  # noqa: SLF001
    assert type(fast) is FusedViTClassifier and fast.feat_extract.residual_dtype == "float32" and eng._defer_norm is True  # noqa: SLF001
    with torch.inference_mode(), torch.autocast("cuda", dtype=dtype):
        x = hook.device_batch(torch.from_numpy(patches).cuda(), torch.float32).permute(0, 3, 1, 2)
        yard = copy.deepcopy(model).cuda()(x).float().cpu().numpy()
    assert out["probabilities"].shape == (3, 9)
    _rule(out["probabilities"], yard, ref["probabilities"], f"PatchPredictor tiny TimmModel {name} residual float32")
    assert float(np.abs(out["probabilities"].sum(-1) - 1).max()) <= 1e-6  # noqa: PLR2004
    kernels = _device_kernels(lambda: eng.infer_patches(eng.dataloader))
    for wanted in ("vit_patchify_norm_u8_h_kernel", "linear_softmax_rows_f32_kernel", *NEW_KERNELS[:2]):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert not [k for k in kernels if _banned(k) or any(old in k for old in REPLACED)], kernels


def test_engine_refuses_the_option_for_head_dim_32(caplog):
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone(NAME)
    model.feat_extract = tiny_vit(num_heads=4, img_size=224, dynamic=False)  # 128 / 4 = 32 per head
    patches = np.random.default_rng(1).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    eng = DeepFeatureExtractor(model, batch_size=2, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"), pytest.raises(ValueError, match="residual_dtype.*head_dim 64"):
        eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16", residual_dtype="float32")
    assert eng.residual_dtype is None
    assert not [r for r in caplog.records if "torch module" in r.getMessage()]  # refused, not run in another form
    for compute in ("float32", "float8_e4m3"):
        with pytest.raises(ValueError, match="residual_dtype"):
            eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=compute, residual_dtype="float32")
        assert eng.residual_dtype is None

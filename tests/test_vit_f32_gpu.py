"""``FusedViT`` on the float32 route (``prepare(torch.float32, linear_dtype="bfloat16x3")``, the engines'
``compute_dtype="bfloat16x3"``) on the GPU: parity with the float64 restatement of the module on the CPU, with the float32 torch
module on the same device as the yardstick; the engines' route to it, and what it launches.  Every figure is printed (collected in
``profiles/vit_f32_tests.txt``)."""

from __future__ import annotations

import copy
import functools
import logging

import numpy as np
import pytest
import torch

from _vit_classifier_ref import timm_model
from _vit_f32_ref import split_graph
from _vit_foundation_ref import TINY_REG, tiny_foundation
from _vit_ref import randomise, tiny_vit
from _vit_resid32_ref import fused_graph, ref64, rel_error
from _vit_virchow_ref import TINY_V2, tiny_virchow

pytestmark = pytest.mark.gpu

NAME = "vit_small_patch16_224"
FLOOR = 8.0 * 2.0 ** -24  # eight float32 units: a yardstick that happens to land nearly exact does not fail a correct graph
# D 128, 2 heads, M 512, depth 2 -- except the head_dim 80 form: 160 / 2 gives a qkv of 480 output channels, which is off every GEMM's
# multiple of 64 (the constructor's UnsupportedLayerError), so it is the Virchow tests' own 320 / 4 with its padded SwiGLU (M 1040)
BUILDERS = {
    "tiny": lambda: tiny_vit(layer_scale=False),
    "tiny-ls": lambda: tiny_vit(layer_scale=True),
    "tiny-reg-swiglu": lambda: tiny_foundation(TINY_REG),  # register tokens, no class entry, p = 14, packed SwiGLU
    "tiny-v2": lambda: tiny_virchow(TINY_V2),              # prefix_pos_embed + token_mean at 80 per head, p = 14
    # the same at 640 / 8 with M 1280: every Linear (qkv 1920, proj 640, fc1 1280, fc2 640, patch 640) is on the split kernel's multiple
    "v2-all-split": lambda: tiny_virchow(TINY_V2, embed_dim=640, num_heads=8, mlp_dim=1280),
}


@functools.lru_cache(maxsize=None)
def _case(form: str, n: int, h: int, w: int):
    """(the module, the float32 batch, its float64 reference on the CPU): computed once, left unchanged."""
    vit = BUILDERS[form]()
    x = torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(h + w + n))
    return vit, x, ref64(vit, x)


def _run(fused, x: torch.Tensor) -> torch.Tensor:
    with torch.inference_mode():
        return fused(x.cuda().contiguous(memory_format=torch.channels_last))  # what `infer_batch` hands over


def _module(vit, x: torch.Tensor) -> torch.Tensor:
    with torch.inference_mode():
        return copy.deepcopy(vit).cuda()(x.cuda()).float().cpu()


def _parity(form: str, n: int, h: int, w: int) -> None:
    """``e = max |feat - ref64| / max(max |ref64|, 1)``: ``e_new <= 2 e_lib + 8 * 2^-24`` with ``e_lib`` the float32 torch module on the same
    device.  The fp16 graph with ``residual_dtype="float32"`` on the same input is recorded beside it, not gated."""
    vit, x, ref = _case(form, n, h, w)
    got = _run(split_graph(vit, "cuda"), x)
    assert got.shape == ref.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    e_new, e_lib = rel_error(got, ref), rel_error(_module(vit, x), ref)
    with torch.inference_mode():
        half = fused_graph(vit, torch.float16, "cuda", residual_dtype="float32")(x.cuda().half().contiguous(memory_format=torch.channels_last))
    e_half = rel_error(half, ref)
    print(f"f32 route {form} n={n} {h}x{w}: e_new {e_new:.3e}  e_lib {e_lib:.3e}  {e_new / (2.0 * e_lib + FLOOR):.3f} of the gate;  "
          f"fp16 graph with a float32 stream {e_half:.3e} = {e_half / max(e_new, 1e-30):.0f} x")
    assert e_new <= 2.0 * e_lib + FLOOR


@pytest.mark.parametrize("form", ["tiny", "tiny-ls"])
@pytest.mark.parametrize("size", [32, 64, 224])
@pytest.mark.parametrize("n", [1, 3])
def test_graph_matches_float64(n, size, form):
    _parity(form, n, size, size)


@pytest.mark.parametrize("form", ["tiny-reg-swiglu", "tiny-v2"])
@pytest.mark.parametrize("size", [28, 56, 224])  # (patch 14: the multiples next to 32 and 64)
@pytest.mark.parametrize("n", [1, 3])
def test_graph_matches_float64_at_patch_14(n, size, form):
    _parity(form, n, size, size)


def test_graph_matches_float64_on_a_resampled_grid():
    _parity("tiny-ls", 2, 48, 64)


@pytest.mark.parametrize(("n", "size"), [(3, 28), (1, 56)])
def test_head_dim_80_beside_the_split_gemm_in_every_layer(n, size):
    """In ``tiny-v2`` only ``fc1`` is on the split kernel's multiple of 128 output channels; here every layer is, so attention at 80 per
    head reads a ``qkv`` and feeds a ``proj`` that the split GEMM wrote and reads."""
    vit, _, _ = _case("v2-all-split", n, size, size)
    fused = split_graph(vit, "cuda")
    assert fused.patch.split and all(layer[name].split for layer in fused.layers for name in ("qkv", "proj", "fc1", "fc2"))
    assert fused.scale == 80 ** -0.5 and fused.layers[0]["qkv"].cout == 1920
    _parity("v2-all-split", n, size, size)


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


@pytest.mark.parametrize("form", ["tiny-ls", "tiny-v2"])
def test_forward_launches_the_new_kernels_and_no_library_gemm(form, caplog):
    side = 32 if form == "tiny-ls" else 28
    vit, x, _ = _case(form, 3, side, side)
    with caplog.at_level(logging.INFO, logger="tiatoolbox_amd"):
        fused = split_graph(vit, "cuda")
    said = [r.getMessage() for r in caplog.records if "split-bf16 GEMM" in r.getMessage()]
    _run(fused, x)
    kernels = _device_kernels(lambda: _run(fused, x))
    wanted = ["mha_fwd_f32_kernel", "conv_ring_bf16x3_kernel", "vit_patchify_f32_kernel", "vit_assemble_f32_kernel", "add_layernorm_rows_f32_kernel"]
    if form == "tiny-ls":  # every layer has an exact split and a shape on the split kernel: no line
        wanted += ["gelu_rows_f32_kernel"]
        assert not said and all(layer[n].split for layer in fused.layers for n in ("qkv", "proj", "fc1", "fc2")) and fused.patch.split
    else:  # 320 -> 960 / 320 are off the multiple of 128: those layers take the float32 GEMM, and one line names them
        wanted += ["swiglu_rows_f32_kernel", "vit_cls_mean_pool_f32_kernel"]
        assert len(said) == 1 and "blocks.0.attn.qkv (320 -> 960)" in said[0] and "blocks.1.mlp.fc2 (576 -> 320)" in said[0]
        assert fused.layers[0]["fc1"].split and fused.layers[0]["fc1"].cout == 1152
    for name in wanted:
        assert any(name in k for k in kernels), (name, kernels)
    assert any(("<80>" in k or "Li80" in k) == (form == "tiny-v2") for k in kernels if "mha_fwd_f32_kernel" in k), kernels
    assert not {k for k in kernels if _banned(k)}, kernels
    assert not [k for k in kernels if "_h_kernel" in k or "conv_mfma_h" in k], kernels  # nothing of the half graphs


# ------------------------------------------------------------------------------------------------------------------------- engines
def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def _rule(got: np.ndarray, lib: np.ndarray, ref: np.ndarray, what: str) -> None:
    scale = max(float(np.abs(ref).max()), 1.0)
    e_new, e_lib = float(np.abs(got - ref).max()) / scale, float(np.abs(lib - ref).max()) / scale
    print(f"{what}: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
    assert got.shape == ref.shape and got.dtype == np.float32 and bool(np.isfinite(got).all()) and e_new <= 2.0 * e_lib + FLOOR


def test_feature_extractor_runs_the_option_and_float32_stays_the_torch_module(caplog):
    from tiatoolbox_amd.models import DeepFeatureExtractor

    patches = np.random.default_rng(0).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    cpu = DeepFeatureExtractor(NAME, batch_size=2)
    randomise(cpu.model.feat_extract)
    vit = cpu.model.feat_extract
    x = torch.from_numpy(patches).float().permute(0, 3, 1, 2)  # (this backbone's hook is the identity on float values)
    ref = ref64(vit, x).numpy()
    eng = DeepFeatureExtractor(copy.deepcopy(cpu.model), batch_size=2, device="cuda")
    got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16x3")["probabilities"]
    fast = eng._inference_model(torch.float32)  # noqa: SLF001  (the cached copy the run used)
    graphs = [m for m in fast.modules() if type(m).__name__ == "FusedViT"]
    assert eng.compute_dtype == "bfloat16x3" and [m.linear_dtype for m in graphs] == ["bfloat16x3"] and graphs[0].half_dtype is None
    assert eng._defer_norm is False  # noqa: SLF001  (the batch reaches the graph as a normalised float32 tensor)
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        lib = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="float32")["probabilities"]
    again = eng._inference_model(torch.float32)  # noqa: SLF001
    assert "FusedViT" not in {type(m).__name__ for m in again.modules()}  # compute_dtype="float32" is the torch module again
    assert len([r for r in caplog.records if "library" in r.getMessage() and "Vision Transformer" in r.getMessage()]) == 1
    assert got.shape == (3, 384) and not np.array_equal(got, lib)
    _rule(got, lib, ref, "DeepFeatureExtractor vit_small bfloat16x3")


def test_patch_predictor_runs_the_option_from_bytes_to_probabilities():
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViTClassifier
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    model = timm_model(tiny_vit(img_size=224, dynamic=False), num_classes=9)
    model.preproc_func = hook = timm_preproc_func(NAME)
    patches = np.random.default_rng(8).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    x = hook.device_batch(torch.from_numpy(patches).cuda(), torch.float32).permute(0, 3, 1, 2).cpu()  # the hook's batched form
    feat = ref64(model.feat_extract, x)
    ref = torch.softmax(feat @ model.classifier.weight.detach().double().T + model.classifier.bias.detach().double(), -1).numpy()
    eng = PatchPredictor(copy.deepcopy(model), batch_size=2, device="cuda")
    out = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype="bfloat16x3")
    fast = eng._inference_model(torch.float32)  # noqa: SLF001
    assert type(fast) is FusedViTClassifier and fast.feat_extract.linear_dtype == "bfloat16x3" and eng._defer_norm is False  # noqa: SLF001
    kernels = _device_kernels(lambda: eng.infer_patches(eng.dataloader))
    for wanted in ("mha_fwd_f32_kernel", "conv_ring_bf16x3_kernel", "linear_softmax_rows_f32_kernel"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert not {k for k in kernels if _banned(k)}, kernels
    lib = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype="float32")
    assert type(eng._inference_model(torch.float32)) is not FusedViTClassifier  # noqa: SLF001
    assert out["probabilities"].shape == (3, 9) and float(np.abs(out["probabilities"].sum(-1) - 1).max()) <= 1e-6  # noqa: PLR2004
    _rule(out["probabilities"], lib["probabilities"], ref, "PatchPredictor tiny TimmModel bfloat16x3")
    assert np.array_equal(out["predictions"], lib["predictions"])


def test_engine_refuses_the_option_for_head_dim_32_and_beside_residual_dtype(caplog):
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone(NAME)
    model.feat_extract = tiny_vit(num_heads=4, img_size=224, dynamic=False)  # 128 / 4 = 32 per head
    patches = np.random.default_rng(1).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    eng = DeepFeatureExtractor(model, batch_size=2, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"), pytest.raises(ValueError, match="bfloat16x3.*head_dim 64"):
        eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16x3")
    assert eng.compute_dtype == "float32"
    assert not [r for r in caplog.records if "torch module" in r.getMessage()]  # refused, not run in another form
    with pytest.raises(ValueError, match="bfloat16x3.*without residual_dtype"):
        eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16x3", residual_dtype="float32")
    assert eng.compute_dtype == "float32" and eng.residual_dtype is None

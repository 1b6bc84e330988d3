"""``return_attention`` on the device: the maps of ``FusedViT`` (``tia_mha_probs_h`` / ``tia_rollout_step_f32`` on the graph's own qkv
tensors) and of the engines against the float64 restatement, with the cast torch module's ``forward_with_attention`` on the same device
as the yardstick; every half route keeps its features bit for bit; the uint8 path; no library kernel appears."""

from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch
from _vit_attention_ref import map_error, maps64_of
from _vit_foundation_ref import TINY_REG, tiny_foundation
from _vit_ref import tiny_vit
from _vit_virchow_ref import TINY_V2, tiny_virchow
from test_vit_gpu import _banned, _device_kernels, _mha_head_dims

from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
KINDS = ("class", "rollout")
BF16 = torch.bfloat16
# Every model runs on a resampled non-square grid of 6 x 5 patches, 16 images at a time.  The criterion below compares two draws of the
# same half-precision rounding noise through the maximum over all map entries; a maximum over a few dozen entries (5 images of 4 x 3)
# is itself too noisy a statistic for a factor of two, so the batch is sized to give it some hundreds of entries (16 x 30 per kind,
# times the heads for "class").
GRID, BATCH = (6, 5), 16
MODELS = {"vit": lambda: tiny_vit(), "registers": lambda: tiny_foundation(TINY_REG), "virchow2": lambda: tiny_virchow(TINY_V2)}  # noqa: PLW0108


def _device_input(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return x.cuda().to(dtype).contiguous(memory_format=torch.channels_last)  # what `infer_batch` hands over


def _fused(vit, dtype: torch.dtype, **prepare):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(copy.deepcopy(vit).cuda())
    fused.prepare(dtype, **prepare)
    return fused.to(dtype)


@functools.lru_cache(maxsize=None)
def _case(name: str):
    """(model, batch, {kind: float64 maps}) -- computed once and left unchanged."""
    vit = MODELS[name]()
    p = vit.patch_size
    x = torch.randn((BATCH, 3, GRID[0] * p, GRID[1] * p), generator=torch.Generator().manual_seed(11))
    return vit, x, {kind: maps64_of(vit, x, kind)[0] for kind in KINDS}


def _lib_maps(vit, x: torch.Tensor, dtype: torch.dtype, kind: str) -> torch.Tensor:
    with torch.inference_mode():
        return copy.deepcopy(vit).cuda().to(dtype).forward_with_attention(x.cuda().to(dtype), kind)[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_fused_maps_match_the_float64_restatement(name, dtype):
    """``e = max |m - m64| / max m64``: the hand-written graph at most twice the error of the torch module cast to ``dtype`` on the
    same device (the project's criterion, ``tests/test_vit_gpu.py``), both kinds; the features are those of a run without maps."""
    vit, x, refs = _case(name)
    fused = _fused(vit, dtype)
    xin = _device_input(x, dtype)
    with torch.inference_mode():
        plain = fused(xin)
        assert fused.attention_maps is None
        for kind in KINDS:
            fused.return_attention = kind
            feats = fused(xin)
            maps = fused.attention_maps
            assert torch.equal(feats, plain)
            assert maps.dtype == torch.float32 and tuple(maps.shape) == tuple(refs[kind].shape) and bool(torch.isfinite(maps).all())
            e_new, e_lib = map_error(maps, refs[kind]), map_error(_lib_maps(vit, x, dtype, kind), refs[kind])
            print(f"fused maps {name} {kind} {dtype}: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
            assert e_new <= 2.0 * e_lib
        fused.return_attention = None
        assert torch.equal(fused(xin), plain) and fused.attention_maps is None


def _backbone(vit):
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    with torch.device("meta"):
        model = TimmBackbone("vit_small_patch16_224")  # (the named trunk's shapes only: it is replaced)
    model.feat_extract = copy.deepcopy(vit)
    model.preproc_func = timm_preproc_func("vit_small_patch16_224")
    return model.eval()


def _cfg(h: int, w: int):
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(h, w), stride_shape=(h, w))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_maps_match_the_float64_restatement(name, dtype):
    """The same criterion through ``DeepFeatureExtractor`` on uint8 patches (sixteen of them in batches of 6, 6 and 4: the uint8 im2col
    path of the graph, the concatenation); the features are bit for bit those of the run without the kwarg, and the next run has no maps."""
    from tiatoolbox_amd.models import DeepFeatureExtractor

    vit = MODELS[name]()
    p = vit.patch_size
    patches = np.random.default_rng(2).integers(0, 256, (BATCH, GRID[0] * p, GRID[1] * p, 3), dtype=np.uint8)
    model = _backbone(vit)
    x = model.preproc_func.device_batch(torch.from_numpy(patches), torch.float32).permute(0, 3, 1, 2).contiguous()
    eng = DeepFeatureExtractor(model, batch_size=6, device="cuda")
    kw = {"patch_mode": True, "ioconfig": _cfg(GRID[0] * p, GRID[1] * p), "compute_dtype": str(dtype).replace("torch.", "")}
    plain = eng.run(patches, **kw)
    assert "attention" not in plain
    for kind in KINDS:
        out = eng.run(patches, return_attention=kind, **kw)
        assert [type(m).__name__ for m in eng._inference_model(dtype).modules()].count("FusedViT") == 1  # noqa: SLF001
        ref = maps64_of(vit, x, kind)[0]
        assert out["attention"].dtype == np.float32 and out["attention"].shape == tuple(ref.shape)
        assert np.array_equal(out["probabilities"], plain["probabilities"])
        e_new, e_lib = map_error(out["attention"], ref), map_error(_lib_maps(vit, x, dtype, kind), ref)
        print(f"engine maps {name} {kind} {dtype}: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
        assert e_new <= 2.0 * e_lib
    assert "attention" not in eng.run(patches, **kw) and eng.return_attention is None


def _route_cases():
    from tiatoolbox_amd.models.architecture.vit_fused import calibrate_int8_smoothing

    def smoothed(vit, x):
        return {"linear_dtype": "int8", "smoothing": calibrate_int8_smoothing(copy.deepcopy(vit).cuda(), [x.cuda()], alpha=0.5)}

    return {
        "float8_e4m3": (lambda: tiny_vit(), (64, 64), lambda vit, x: {"linear_dtype": "float8_e4m3"}),  # noqa: ARG005, PLW0108
        "int8": (lambda: tiny_foundation({**TINY_REG, "reg_tokens": 4}), (42, 56), lambda vit, x: {"linear_dtype": "int8"}),  # noqa: ARG005
        "int8-smoothed": (lambda: tiny_virchow(TINY_V2), (28, 28), smoothed),
        "residual-float32": (lambda: tiny_vit(), (48, 64), lambda vit, x: {"residual_dtype": "float32"}),  # noqa: ARG005, PLW0108
    }


@pytest.mark.parametrize("route", ["float8_e4m3", "int8", "int8-smoothed", "residual-float32"])
def test_every_half_route_returns_maps_and_keeps_its_features(route):
    """The map kernels read the qkv tensor the route's own ``qkv`` layer wrote and write nothing the graph reads: finite maps of the
    right shape, features bit for bit those of the same route without maps."""
    make, (h, w), prepare = _route_cases()[route]
    vit = make()
    x = torch.randn((3, 3, h, w), generator=torch.Generator().manual_seed(h + w))
    fused = _fused(vit, BF16, **prepare(vit, x))
    xin = _device_input(x, BF16)
    gh, gw = h // vit.patch_size, w // vit.patch_size
    with torch.inference_mode():
        plain = fused(xin)
        for kind in KINDS:
            fused.return_attention = kind
            assert torch.equal(fused(xin), plain)
            maps = fused.attention_maps
            assert tuple(maps.shape) == ((3, vit.num_heads, gh, gw) if kind == "class" else (3, gh, gw))
            assert maps.dtype == torch.float32 and bool(torch.isfinite(maps).all()) and float(maps.min()) >= 0
            ref = maps64_of(vit, x, kind)[0]
            print(f"route {route} {kind}: e {map_error(maps, ref):.3e} against the float64 module (not gated: a quantised graph)")
            assert float(maps.sum((-2, -1)).max()) <= 1 + 1e-5


def test_uint8_path_returns_the_maps_of_the_float_path_bit_for_bit():
    """``forward_uint8`` (the hook's table looked up inside the im2col) and ``forward`` on the hook's output are the same graph from the
    token GEMM on: the same features and the same maps, for a backbone and for a classifier's graph."""
    from _vit_classifier_ref import timm_model

    from tiatoolbox_amd.models.architecture.vit_fused import FusedViTClassifier

    hook = timm_preproc_func("vit_small_patch16_224")
    vit = tiny_foundation(TINY_REG)
    p = vit.patch_size
    x_u8 = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (3, 3 * p, 2 * p, 3), dtype=np.uint8)).cuda()
    model = timm_model(vit).cuda()
    graph = FusedViTClassifier(model)
    graph.prepare(BF16)
    graph = graph.to(BF16)
    table = hook.device_table(x_u8.device, BF16)
    x = hook.device_batch(x_u8, BF16).permute(0, 3, 1, 2)
    with torch.inference_mode():
        for kind in KINDS:
            graph.return_attention = kind
            a = graph.forward_uint8(x_u8, table)
            maps_u8 = graph.attention_maps
            b = graph(x)
            assert torch.equal(a, b) and torch.equal(maps_u8, graph.attention_maps) and maps_u8 is not graph.attention_maps
            assert tuple(maps_u8.shape) == ((3, vit.num_heads, 3, 2) if kind == "class" else (3, 3, 2))


def test_bf16_forward_with_rollout_launches_only_handwritten_kernels():
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(tiny_vit(layer_scale=True, dynamic=True).cuda())
    fused.prepare(BF16)
    fused = fused.to(BF16)
    fused.return_attention = "rollout"
    x = torch.randn((2, 3, 64, 64), device="cuda").to(BF16).contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        fused(x)
        kernels = _device_kernels(lambda: fused(x))
    for wanted in ("mha_fwd_h_kernel", "mha_probs_kernel", "rollout_step_kernel", "layernorm_rows_h_kernel", "conv_mfma_h"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert _mha_head_dims(kernels) == {64}, kernels  # (the head_dim-64 instantiation of the one attention kernel, and no other)
    assert not {k for k in kernels if _banned(k) or "softmax" in k.lower()}, kernels

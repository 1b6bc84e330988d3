"""``FusedViT`` with ``linear_dtype="int8"`` and the engines' ``compute_dtype="int8"`` against the float32 module on the CPU.  The
yardstick is the torch module in bfloat16 on the same device with the inputs and weights of ``qkv`` / ``fc1`` / ``fc2`` fake-quantised
by the recipe (``_vit_int8_ref.fake_quantised_module``); the INT8 graph may have at most twice its error.  Every case also prints --
and does not gate -- the FP8 graph's and the bf16 graph's error and cosine on the same model and input: the evidence of the
accuracy claim.  And: the kernels an INT8 forward launches, a layer off the INT8 GEMM's shapes, and run-to-run determinism."""

from __future__ import annotations

import copy
import logging

import numpy as np
import pytest
import torch

from _vit_classifier_ref import redraw_classifier
from _vit_foundation_ref import TINY_REG, tiny_foundation
from _vit_int8_ref import fake_quantised_module, rel_error
from _vit_ref import randomise, tiny_vit
from _vit_virchow_ref import TINY_V2, tiny_virchow
from test_vit_gpu import _banned, _device_kernels, _mha_head_dims

pytestmark = pytest.mark.gpu

INT8 = "int8"
FP8 = "float8_e4m3"
BF16 = torch.bfloat16


def _graph(vit, linear_dtype=INT8):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(copy.deepcopy(vit).cuda())
    fused.prepare(BF16, linear_dtype=linear_dtype)
    return fused.to(BF16)


def _cos(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float(torch.nn.functional.cosine_similarity(got.cpu().double(), ref.double(), dim=-1).min())


def _parity_int8(vit, x: torch.Tensor, what: str, layers=("qkv", "fc1", "fc2")) -> None:
    """``e = max |feat - ref| / max(max |ref|, 1)`` against the float32 module on the CPU: ``e_int8_graph <= 2 e_yardstick``.  The FP8
    and bf16 graphs' figures are printed beside it, not asserted."""
    with torch.inference_mode():
        ref = vit(x)
        xd = x.cuda().to(BF16).contiguous(memory_format=torch.channels_last)
        yard = fake_quantised_module(copy.deepcopy(vit).cuda(), layers=layers)(x.cuda().to(BF16)).float()
        fused = _graph(vit)
        assert fused.linear_dtype == INT8 and fused.half_dtype == BF16
        got = fused(xd)
        fp8, bf16 = _graph(vit, FP8)(xd), _graph(vit, None)(xd)
    assert got.shape == ref.shape and got.dtype == torch.float32
    e_new, e_yard = rel_error(got, ref), rel_error(yard, ref)
    print(f"{what}: e_int8_graph {e_new:.3e}  e_yardstick {e_yard:.3e}  min cosine {_cos(got, ref):.5f}  |  not gated: fp8 graph e "
          f"{rel_error(fp8, ref):.3e} cos {_cos(fp8, ref):.5f}, bf16 graph e {rel_error(bf16, ref):.3e} cos {_cos(bf16, ref):.5f}")
    assert bool(torch.isfinite(got).all()) and e_new <= 2.0 * e_yard


@pytest.mark.parametrize("size", [32, 64, 224])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("layer_scale", [True, False], ids=["ls", "no-ls"])
def test_int8_graph_matches_module(layer_scale, n, size):
    vit = tiny_vit(layer_scale=layer_scale, embed_dim=128, num_heads=2, mlp_dim=512)
    x = torch.randn((n, 3, size, size), generator=torch.Generator().manual_seed(size + n))
    _parity_int8(vit, x, f"tiny layer_scale={layer_scale} n={n} {size}x{size}")


@pytest.mark.parametrize("n", [1, 3])
def test_int8_graph_matches_module_at_vit_small_shape(n):
    vit = tiny_vit(layer_scale=True, embed_dim=384, num_heads=6, mlp_dim=1536, img_size=224)
    x = torch.randn((n, 3, 224, 224), generator=torch.Generator().manual_seed(9 + n))
    _parity_int8(vit, x, f"vit_small shape with LayerScale, depth 2, n={n} 224x224")


@pytest.mark.parametrize("n", [1, 3])
def test_int8_graph_matches_module_with_registers_and_swiglu(n):
    vit = tiny_foundation({**TINY_REG, "reg_tokens": 4})
    x = torch.randn((n, 3, 42, 56), generator=torch.Generator().manual_seed(5 + n))
    _parity_int8(vit, x, f"tiny patch 14, R=4, SwiGLU n={n} 42x56")


@pytest.mark.parametrize("n", [1, 3])
def test_int8_graph_matches_module_with_token_mean_pooling(n):
    """320 / 4 = 80 per head: ``qkv`` and ``fc1`` (K = 320) are off ``K % 128`` and stay half; H = 520 -> 544 -> 640 for the INT8 ``fc2``,
    which is what the yardstick quantises."""
    vit = tiny_virchow(TINY_V2)
    x = torch.randn((n, 3, 28, 28), generator=torch.Generator().manual_seed(6 + n))
    _parity_int8(vit, x, f"tiny token_mean (Virchow2 form) D=320 n={n} 28x28", layers=("fc2",))


def test_two_forwards_are_bit_identical():
    """The int32 accumulator is exact and every other kernel of the graph is deterministic: the same batch twice gives the same bits,
    from a second graph built from the same weights as well."""
    vit = tiny_vit(layer_scale=True, embed_dim=384, num_heads=6, mlp_dim=1536, img_size=224)
    x = torch.randn((3, 3, 224, 224), generator=torch.Generator().manual_seed(3)).cuda().to(BF16).contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        fused = _graph(vit)
        first, second, other = fused(x), fused(x), _graph(vit)(x)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)) and torch.equal(first.view(torch.int32), other.view(torch.int32))


def test_int8_forward_launches_the_int8_kernels_and_no_library():
    fused = _graph(tiny_vit(layer_scale=True, dynamic=True))
    swiglu = _graph(tiny_foundation({**TINY_REG, "reg_tokens": 4}))
    x = torch.randn((2, 3, 64, 64), device="cuda").to(BF16).contiguous(memory_format=torch.channels_last)
    x14 = torch.randn((2, 3, 56, 56), device="cuda").to(BF16).contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        fused(x)
        swiglu(x14)
        kernels = _device_kernels(lambda: fused(x))
        kernels_swiglu = _device_kernels(lambda: swiglu(x14))
    for wanted in ("linear_rows_kernel<tia::q8::Int8", "layernorm_rows_kernel<tia::q8::Int8", "act_rows_kernel<tia::q8::Int8", "mha_fwd_h_kernel", "conv_mfma_h"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
        assert any(wanted in k for k in kernels_swiglu), (wanted, kernels_swiglu)
    assert _mha_head_dims(kernels) == _mha_head_dims(kernels_swiglu) == {64}, (kernels, kernels_swiglu)  # (head_dim 64: that instantiation and no other)
    assert {k for k in kernels if "act_rows_kernel<tia::q8::Int8" in k} != {k for k in kernels_swiglu if "act_rows_kernel<tia::q8::Int8" in k}
    for ks in (kernels, kernels_swiglu):  # every INT8 layer's producer is the quantising one; nothing of the FP8 route runs
        assert not {k for k in ks if "gelu_rows_h_kernel" in k or "swiglu_rows_h_kernel" in k or "fp8" in k or "tia::q8::E4m3" in k}, ks
        assert not {k for k in ks if _banned(k)}, ks


def test_a_layer_off_the_int8_shapes_stays_on_the_half_kernel(caplog):
    """``mlp_dim = 576``: ``fc2`` (576 -> 128) is off the INT8 GEMM's ``K % 128`` and on the half GEMM's ``cin % 32``; ``qkv`` and
    ``fc1`` (128 -> 576) go to INT8.  One ``info`` line names the layers that stay."""
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    vit = tiny_vit(mlp_dim=576)
    with caplog.at_level(logging.INFO, logger="tiatoolbox_amd"):
        fused = _graph(vit)
    said = [r.getMessage() for r in caplog.records if "half kernel" in r.getMessage()]
    assert len(said) == 1 and "INT8" in said[0] and "blocks.0.mlp.fc2" in said[0] and "blocks.1.mlp.fc2" in said[0] and "fc1" not in said[0], said
    kinds = {name: {type(layer[name]).__name__ for layer in fused.layers} for name in ("qkv", "proj", "fc1", "fc2")}
    assert kinds == {"qkv": {"_LinearInt8"}, "proj": {"_Linear"}, "fc1": {"_LinearInt8"}, "fc2": {"_Linear"}}
    assert isinstance(fused, FusedViT)
    x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        kernels = _device_kernels(lambda: fused(x.cuda().to(BF16)))
    assert any("gelu_rows_h_kernel" in k for k in kernels) and not any("act_rows_kernel<tia::q8::Int8" in k for k in kernels), kernels
    assert any("linear_rows_kernel<tia::q8::Int8" in k for k in kernels) and any("layernorm_rows_kernel<tia::q8::Int8" in k for k in kernels), kernels
    _parity_int8(vit, x, "mlp_dim 576 (fc2 on the half kernel)", layers=("qkv", "fc1"))  # the yardstick quantises what the graph does


# ------------------------------------------------------------------------------------------------------------------- the engines
NAME = "vit_small_patch16_224"


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def _rule(got: np.ndarray, yard: np.ndarray, ref: np.ndarray, what: str) -> None:
    scale = max(float(np.abs(ref).max()), 1.0)
    e_new, e_yard = float(np.abs(got - ref).max()) / scale, float(np.abs(yard - ref).max()) / scale
    print(f"{what}: e_int8 {e_new:.3e}  e_yardstick {e_yard:.3e}")
    assert got.shape == ref.shape and got.dtype == np.float32 and bool(np.isfinite(got).all()) and e_new <= 2.0 * e_yard


def _no_warning(caplog) -> None:
    assert not [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and r.name.startswith("tiatoolbox_amd")]


def test_feature_extractor_runs_int8_from_uint8_patches(caplog):
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    patches = np.random.default_rng(0).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    cpu = DeepFeatureExtractor(NAME, batch_size=2)
    randomise(cpu.model.feat_extract)
    cpu.model.preproc_func = timm_preproc_func(NAME)  # ToTensor + Normalize: on the GPU the graph's im2col makes it from the uint8 batch
    ref = cpu.run(patches, patch_mode=True, ioconfig=_cfg())["probabilities"]
    eng = DeepFeatureExtractor(NAME, batch_size=2, device="cuda")
    eng.model.feat_extract.load_state_dict(cpu.model.feat_extract.state_dict(), strict=True)
    eng.model.preproc_func = timm_preproc_func(NAME)
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=INT8)["probabilities"]
    _no_warning(caplog)
    assert eng.compute_dtype == INT8 and eng._defer_norm is True  # noqa: SLF001
    fast = eng._inference_model(BF16)  # noqa: SLF001  (the cached copy the run used)
    graphs = [m for m in fast.modules() if type(m).__name__ == "FusedViT"]
    assert len(graphs) == 1 and graphs[0].linear_dtype == INT8 and next(fast.parameters()).dtype == BF16
    with torch.inference_mode():
        x = cpu.model.preproc_func.device_batch(torch.from_numpy(patches).cuda(), BF16).permute(0, 3, 1, 2)
        yard = fake_quantised_module(copy.deepcopy(cpu.model).cuda())(x).float().cpu().numpy()
    _rule(got, yard, ref, "DeepFeatureExtractor vit_small int8")
    kernels = _device_kernels(lambda: eng.infer_patches(eng.dataloader))
    for wanted in ("vit_patchify_norm_u8_h_kernel", "linear_rows_kernel<tia::q8::Int8", "layernorm_rows_kernel<tia::q8::Int8", "act_rows_kernel<tia::q8::Int8"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert not {k for k in kernels if _banned(k)}, kernels
    # the cache tells the option from FP8 and from plain bfloat16: other copies, and back again to the same bits
    fp8 = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=FP8)["probabilities"]
    assert [m.linear_dtype for m in eng._inference_model(BF16).modules() if type(m).__name__ == "FusedViT"] == [FP8]  # noqa: SLF001
    plain = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")["probabilities"]
    assert [m.linear_dtype for m in eng._inference_model(BF16).modules() if type(m).__name__ == "FusedViT"] == [None]  # noqa: SLF001
    assert not np.array_equal(plain, got) and not np.array_equal(fp8, got)
    again = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=INT8)["probabilities"]
    assert np.array_equal(again, got)
    scale = max(float(np.abs(ref).max()), 1.0)
    print(f"not gated: fp8 e {float(np.abs(fp8 - ref).max()) / scale:.3e}, bf16 e {float(np.abs(plain - ref).max()) / scale:.3e}")


def test_patch_predictor_runs_a_timm_model_in_int8(caplog):
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture.vanilla import TimmModel
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViTClassifier
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    torch.manual_seed(0)
    model = TimmModel(NAME, 9)
    randomise(model.feat_extract)
    redraw_classifier(model.classifier)
    model.preproc_func = timm_preproc_func(NAME)
    model = model.eval()
    # 16 patches, as in the FP8 test: e is a maximum over patches x 9 probabilities, for the graph and for the yardstick alike; over few
    # values the ratio of two such maxima scatters by more than the rule's factor of 2
    patches = np.random.default_rng(8).integers(0, 256, (16, 224, 224, 3), dtype=np.uint8)
    ref = PatchPredictor(copy.deepcopy(model), batch_size=8).run(patches, patch_mode=True, ioconfig=_cfg(),
                                                                 return_probabilities=True)["probabilities"]
    eng = PatchPredictor(copy.deepcopy(model), batch_size=8, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        out = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype=INT8)
    _no_warning(caplog)
    fast = eng._inference_model(BF16)  # noqa: SLF001
    assert type(fast) is FusedViTClassifier and fast.feat_extract.linear_dtype == INT8 and eng._defer_norm is True  # noqa: SLF001
    assert [type(m).__name__ for m in fast.modules()].count("FusedViT") == 1
    with torch.inference_mode():
        x = model.preproc_func.device_batch(torch.from_numpy(patches).cuda(), BF16).permute(0, 3, 1, 2)
        yard = fake_quantised_module(copy.deepcopy(model).cuda())(x).float().cpu().numpy()
    _rule(out["probabilities"], yard, ref, "PatchPredictor TimmModel vit_small int8")
    assert float(np.abs(out["probabilities"].sum(-1) - 1).max()) <= 1e-6
    kernels = _device_kernels(lambda: eng.infer_patches(eng.dataloader))
    for wanted in ("vit_patchify_norm_u8_h_kernel", "linear_rows_kernel<tia::q8::Int8", "layernorm_rows_kernel<tia::q8::Int8", "act_rows_kernel<tia::q8::Int8",
                   "linear_softmax_rows_f32_kernel"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert not {k for k in kernels if _banned(k)}, kernels


def test_engine_refuses_int8_for_a_vit_the_graph_does_not_take():
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone(NAME)
    model.feat_extract = tiny_vit(num_heads=4, img_size=224, dynamic=False)  # 128 / 4 = 32 per head: FusedViT refuses it
    patches = np.random.default_rng(1).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    eng = DeepFeatureExtractor(model, batch_size=2, device="cuda")
    with pytest.raises(ValueError, match="int8.*head_dim 64"):
        eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=INT8)
    assert eng.compute_dtype == "float32" and eng.residual_dtype is None
    with pytest.raises(ValueError, match="int8.*residual_dtype"):
        eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=INT8, residual_dtype="float32")
    assert eng.compute_dtype == "float32" and eng.residual_dtype is None

"""``FusedViT`` with ``linear_dtype="float8_e4m3"`` and the engines' ``compute_dtype="float8_e4m3"`` against the float32 module on the
CPU.  The yardstick is the analogue of ``test_vit_gpu._parity``'s: the torch module in bfloat16 on the same device with the inputs
and weights of ``qkv`` / ``fc1`` / ``fc2`` fake-quantised by the recipe (``_vit_fp8_ref.fake_quantised_module``); the FP8 graph may
have at most twice its error.  And: the kernels an FP8 forward launches, and a layer off the FP8 GEMM's shapes."""

from __future__ import annotations

import copy
import logging

import numpy as np
import pytest
import torch

from _vit_classifier_ref import redraw_classifier
from _vit_foundation_ref import TINY_REG, tiny_foundation
from _vit_fp8_ref import fake_quantised_module, rel_error
from _vit_ref import randomise, tiny_vit
from _vit_virchow_ref import TINY_V2, tiny_virchow
from test_vit_gpu import _banned, _device_kernels, _mha_head_dims

pytestmark = pytest.mark.gpu

FP8 = "float8_e4m3"
BF16 = torch.bfloat16


def _fp8_graph(vit):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(copy.deepcopy(vit).cuda())
    fused.prepare(BF16, linear_dtype=FP8)
    return fused.to(BF16)


def _parity_fp8(vit, x: torch.Tensor, what: str) -> None:
    """``e = max |feat - ref| / max(max |ref|, 1)`` against the float32 module on the CPU: ``e_fp8_graph <= 2 e_yardstick``."""
    with torch.inference_mode():
        ref = vit(x)
        yard = fake_quantised_module(copy.deepcopy(vit).cuda())(x.cuda().to(BF16)).float()
        bf16 = copy.deepcopy(vit).cuda().to(BF16)(x.cuda().to(BF16)).float()
        fused = _fp8_graph(vit)
        assert fused.linear_dtype == FP8 and fused.half_dtype == BF16
        got = fused(x.cuda().to(BF16).contiguous(memory_format=torch.channels_last))
    assert got.shape == ref.shape and got.dtype == torch.float32
    e_new, e_yard, e_bf16 = rel_error(got, ref), rel_error(yard, ref), rel_error(bf16, ref)
    cos = float(torch.nn.functional.cosine_similarity(got.cpu().double(), ref.double(), dim=-1).min())
    print(f"{what}: e_fp8_graph {e_new:.3e}  e_yardstick {e_yard:.3e}  (bf16 module {e_bf16:.3e})  min cosine {cos:.5f}")
    assert bool(torch.isfinite(got).all()) and e_new <= 2.0 * e_yard


@pytest.mark.parametrize("size", [(32, 32), (64, 64), (48, 64)], ids=["32", "64", "48x64"])
@pytest.mark.parametrize("n", [1, 3])
def test_fp8_graph_matches_module(n, size):
    vit = tiny_vit(embed_dim=128, num_heads=2, mlp_dim=512)
    x = torch.randn((n, 3, *size), generator=torch.Generator().manual_seed(size[0] + size[1] + n))
    _parity_fp8(vit, x, f"tiny n={n} {size[0]}x{size[1]}")


def test_fp8_graph_matches_module_at_vit_small_shape():
    vit = tiny_vit(layer_scale=True, embed_dim=384, num_heads=6, mlp_dim=1536, img_size=224)
    x = torch.randn((2, 3, 224, 224), generator=torch.Generator().manual_seed(9))
    _parity_fp8(vit, x, "vit_small shape with LayerScale, depth 2, n=2")


def test_fp8_graph_matches_module_with_registers_and_swiglu():
    vit = tiny_foundation({**TINY_REG, "reg_tokens": 4})
    x = torch.randn((3, 3, 42, 56), generator=torch.Generator().manual_seed(5))
    _parity_fp8(vit, x, "tiny patch 14, R=4, SwiGLU n=3 42x56")


def test_fp8_graph_matches_module_with_token_mean_pooling():
    vit = tiny_virchow(TINY_V2)  # 320 / 4 = 80 per head: qkv 320 -> 960 is off K % 128 and stays half; H = 520 -> 544 -> 640 for FP8
    x = torch.randn((2, 3, 28, 28), generator=torch.Generator().manual_seed(6))
    _parity_fp8(vit, x, "tiny token_mean (Virchow2 form) n=2 28x28")


def test_fp8_forward_launches_the_fp8_kernels_and_no_library():
    fused = _fp8_graph(tiny_vit(layer_scale=True, dynamic=True))
    swiglu = _fp8_graph(tiny_foundation({**TINY_REG, "reg_tokens": 4}))
    x = torch.randn((2, 3, 64, 64), device="cuda").to(BF16).contiguous(memory_format=torch.channels_last)
    x14 = torch.randn((2, 3, 56, 56), device="cuda").to(BF16).contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        fused(x)
        swiglu(x14)
        kernels = _device_kernels(lambda: fused(x))
        kernels_swiglu = _device_kernels(lambda: swiglu(x14))
    for wanted in ("linear_rows_kernel<tia::q8::E4m3", "layernorm_rows_kernel<tia::q8::E4m3", "act_rows_kernel<tia::q8::E4m3", "mha_fwd_h_kernel", "conv_mfma_h"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
        assert any(wanted in k for k in kernels_swiglu), (wanted, kernels_swiglu)
    assert _mha_head_dims(kernels) == _mha_head_dims(kernels_swiglu) == {64}, (kernels, kernels_swiglu)  # (head_dim 64: that instantiation and no other)
    # the GELU and the SwiGLU form of the activation producer are two instantiations of one kernel template
    assert {k for k in kernels if "act_rows_kernel<tia::q8::E4m3" in k} != {k for k in kernels_swiglu if "act_rows_kernel<tia::q8::E4m3" in k}
    for ks in (kernels, kernels_swiglu):  # every FP8 layer's producer is the quantising one: no half LayerNorm / activation pass
        assert not {k for k in ks if "gelu_rows_h_kernel" in k or "swiglu_rows_h_kernel" in k}, ks
        assert not {k for k in ks if _banned(k)}, ks


def test_a_layer_off_the_fp8_shapes_stays_on_the_half_kernel(caplog):
    """``mlp_dim = 576``: ``fc2`` (576 -> 128) is off the FP8 GEMM's ``K % 128`` and on the half GEMM's ``cin % 32``; ``qkv`` and
    ``fc1`` (128 -> 576) go to FP8.  (``mlp_dim = 544`` cannot be built: ``fc1``'s 544 outputs are off the half GEMM's
    ``cout % 64``, which ``FusedViT``'s constructor refuses for every ``linear_dtype``, as ``tests/test_vit.py`` pins.)"""
    from tiatoolbox_amd.models.architecture.unet_fused import UnsupportedLayerError
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    with pytest.raises(UnsupportedLayerError, match="cout % 64"):
        FusedViT(tiny_vit(mlp_dim=544))
    vit = tiny_vit(mlp_dim=576)
    with caplog.at_level(logging.INFO, logger="tiatoolbox_amd"):
        fused = _fp8_graph(vit)
    said = [r.getMessage() for r in caplog.records if "half kernel" in r.getMessage()]
    assert len(said) == 1 and "blocks.0.mlp.fc2" in said[0] and "blocks.1.mlp.fc2" in said[0] and "fc1" not in said[0], said
    kinds = {name: {type(layer[name]).__name__ for layer in fused.layers} for name in ("qkv", "proj", "fc1", "fc2")}
    assert kinds == {"qkv": {"_LinearFp8"}, "proj": {"_Linear"}, "fc1": {"_LinearFp8"}, "fc2": {"_Linear"}}
    x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        kernels = _device_kernels(lambda: fused(x.cuda().to(BF16)))
    assert any("gelu_rows_h_kernel" in k for k in kernels) and not any("act_rows_kernel<tia::q8::E4m3" in k for k in kernels), kernels
    assert any("linear_rows_kernel<tia::q8::E4m3" in k for k in kernels) and any("layernorm_rows_kernel<tia::q8::E4m3" in k for k in kernels), kernels
    # the yardstick for this model quantises what the graph quantises: qkv and fc1 only
    with torch.inference_mode():
        ref = vit(x)
        got = fused(x.cuda().to(BF16))
        yard_mod = copy.deepcopy(vit).cuda()
        fc2 = {n: copy.deepcopy(m) for n, m in yard_mod.named_modules() if n.endswith("mlp.fc2")}
        yard_mod = fake_quantised_module(yard_mod)
        for n, m in fc2.items():  # fc2 back to its own weights, no hook
            parent = yard_mod.get_submodule(n.rsplit(".", 1)[0])
            parent.fc2 = m.to(BF16)
        yard = yard_mod(x.cuda().to(BF16)).float()
    e_new, e_yard = rel_error(got, ref), rel_error(yard, ref)
    print(f"mlp_dim 576: e_fp8_graph {e_new:.3e}  e_yardstick {e_yard:.3e}")
    assert bool(torch.isfinite(got).all()) and e_new <= 2.0 * e_yard


# ------------------------------------------------------------------------------------------------------------------- the engines
NAME = "vit_small_patch16_224"


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def _rule(got: np.ndarray, yard: np.ndarray, ref: np.ndarray, what: str) -> None:
    scale = max(float(np.abs(ref).max()), 1.0)
    e_new, e_yard = float(np.abs(got - ref).max()) / scale, float(np.abs(yard - ref).max()) / scale
    print(f"{what}: e_fp8 {e_new:.3e}  e_yardstick {e_yard:.3e}")
    assert got.shape == ref.shape and got.dtype == np.float32 and bool(np.isfinite(got).all()) and e_new <= 2.0 * e_yard


def _no_warning(caplog) -> None:
    assert not [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and r.name.startswith("tiatoolbox_amd")]


def test_feature_extractor_runs_fp8(caplog):
    from tiatoolbox_amd.models import DeepFeatureExtractor

    patches = np.random.default_rng(0).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    cpu = DeepFeatureExtractor(NAME, batch_size=2)
    randomise(cpu.model.feat_extract)
    ref = cpu.run(patches, patch_mode=True, ioconfig=_cfg())["probabilities"]
    eng = DeepFeatureExtractor(NAME, batch_size=2, device="cuda")
    eng.model.feat_extract.load_state_dict(cpu.model.feat_extract.state_dict(), strict=True)
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=FP8)["probabilities"]
    _no_warning(caplog)
    assert eng.compute_dtype == FP8
    fast = eng._inference_model(BF16)  # noqa: SLF001  (the cached copy the run used)
    graphs = [m for m in fast.modules() if type(m).__name__ == "FusedViT"]
    assert len(graphs) == 1 and graphs[0].linear_dtype == FP8 and next(fast.parameters()).dtype == BF16
    with torch.inference_mode():
        x = torch.from_numpy(patches).cuda().to(BF16).permute(0, 3, 1, 2)
        yard = fake_quantised_module(copy.deepcopy(cpu.model).cuda())(x).float().cpu().numpy()
    _rule(got, yard, ref, "DeepFeatureExtractor vit_small float8_e4m3")
    # the cache tells the option from plain bfloat16: another copy, without FP8 layers, and back again
    plain = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")["probabilities"]
    bf = eng._inference_model(BF16)  # noqa: SLF001
    assert bf is not fast and [m.linear_dtype for m in bf.modules() if type(m).__name__ == "FusedViT"] == [None]
    assert not np.array_equal(plain, got)
    again = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=FP8)["probabilities"]
    assert np.array_equal(again, got)


def test_patch_predictor_runs_a_timm_model_in_fp8(caplog):
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
    # 16 patches: e is a maximum over patches x 9 probabilities of (roughly) random projections of the feature error, for the graph and
    # for the yardstick alike; over 3 patches (27 values) the ratio of two such maxima scatters by more than the rule's factor of 2
    # while the feature errors themselves agree to 10 % (test_feature_extractor_runs_fp8), over 144 values it does not
    patches = np.random.default_rng(8).integers(0, 256, (16, 224, 224, 3), dtype=np.uint8)
    ref = PatchPredictor(copy.deepcopy(model), batch_size=8).run(patches, patch_mode=True, ioconfig=_cfg(),
                                                                 return_probabilities=True)["probabilities"]
    eng = PatchPredictor(copy.deepcopy(model), batch_size=8, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        out = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype=FP8)
    _no_warning(caplog)
    fast = eng._inference_model(BF16)  # noqa: SLF001
    assert type(fast) is FusedViTClassifier and fast.feat_extract.linear_dtype == FP8 and eng._defer_norm is True  # noqa: SLF001
    assert [type(m).__name__ for m in fast.modules()].count("FusedViT") == 1
    with torch.inference_mode():
        x = model.preproc_func.device_batch(torch.from_numpy(patches).cuda(), BF16).permute(0, 3, 1, 2)
        yard = fake_quantised_module(copy.deepcopy(model).cuda())(x).float().cpu().numpy()
    _rule(out["probabilities"], yard, ref, "PatchPredictor TimmModel vit_small float8_e4m3")
    assert float(np.abs(out["probabilities"].sum(-1) - 1).max()) <= 1e-6
    kernels = _device_kernels(lambda: eng.infer_patches(eng.dataloader))
    for wanted in ("vit_patchify_norm_u8_h_kernel", "linear_rows_kernel<tia::q8::E4m3", "layernorm_rows_kernel<tia::q8::E4m3", "act_rows_kernel<tia::q8::E4m3",
                   "linear_softmax_rows_f32_kernel"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert not {k for k in kernels if _banned(k)}, kernels


def test_engine_refuses_fp8_for_a_vit_the_graph_does_not_take():
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone(NAME)
    model.feat_extract = tiny_vit(num_heads=4, img_size=224, dynamic=False)  # 128 / 4 = 32 per head: FusedViT refuses it
    patches = np.random.default_rng(1).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    eng = DeepFeatureExtractor(model, batch_size=2, device="cuda")
    with pytest.raises(ValueError, match="float8_e4m3.*head_dim 64"):
        eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype=FP8)
    assert eng.compute_dtype == "float32"

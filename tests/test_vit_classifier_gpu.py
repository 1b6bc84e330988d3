"""``PatchPredictor(TimmModel)`` and ``DeepFeatureExtractor`` with a ``TimmNormPreproc`` hook on the GPU: uint8 patches to
probabilities on the hand-written kernels alone, against the CPU float32 engine run with the cast torch module as the yardstick
(the rule of ``test_vit_gpu.py``); the routes that stay as they were; when the normalisation is deferred and when not."""

from __future__ import annotations

import copy
import logging

import numpy as np
import pytest
import torch

from _vit_classifier_ref import redraw_classifier, timm_model
from _vit_ref import randomise
from _vit_virchow_ref import TINY_V2, tiny_virchow
from test_vit_gpu import _banned, _device_kernels, _mha_head_dims

pytestmark = pytest.mark.gpu

DTYPES = [("float16", torch.float16), ("bfloat16", torch.bfloat16)]
IDS = ["fp16", "bf16"]
NAME = "vit_small_patch16_224"


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def _torch_kernel(name: str) -> bool:
    """An element-wise, index or softmax kernel of torch (the head kernel's own name holds the word softmax)."""
    low = name.lower()
    return "linear_softmax_rows_f32_kernel" not in low and any(w in low for w in ("elementwise", "index", "softmax"))


def _new_model(num_classes: int = 9):
    from tiatoolbox_amd.models.architecture.vanilla import TimmModel
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    torch.manual_seed(0)
    model = TimmModel(NAME, num_classes)
    randomise(model.feat_extract)
    redraw_classifier(model.classifier)
    model.preproc_func = timm_preproc_func(NAME)
    return model.eval()


def _library(model, patches: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """The yardstick: the torch module cast to ``dtype`` on the device, fed the hook's batched device form."""
    with torch.inference_mode():
        x = model.preproc_func.device_batch(torch.from_numpy(patches).cuda(), dtype).permute(0, 3, 1, 2)
        return copy.deepcopy(model).cuda().to(dtype)(x).float().cpu().numpy()


def _within_rule(got: np.ndarray, lib: np.ndarray, ref: np.ndarray, what: str) -> None:
    scale = max(float(np.abs(ref).max()), 1.0)
    e_new, e_lib = float(np.abs(got - ref).max()) / scale, float(np.abs(lib - ref).max()) / scale
    print(f"{what}: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
    assert got.shape == ref.shape and got.dtype == np.float32 and bool(np.isfinite(got).all()) and e_new <= 2.0 * e_lib


@pytest.fixture(scope="module")
def runs():
    """One randomised ``vit_small_patch16_224`` ``TimmModel`` with 9 classes: patches, the model, its CPU float32 engine run."""
    from tiatoolbox_amd.models import PatchPredictor

    # (seed 8: the CPU run's own margins between the two largest probabilities are 0.23 .. 0.31 and both classes occur, so that equal
    # arg-maxima are a fair demand on a half-precision run; at seed 0 one patch has a margin of 0.018)
    patches = np.random.default_rng(8).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    model = _new_model()
    ref = PatchPredictor(copy.deepcopy(model), batch_size=2).run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True)
    assert ref["probabilities"].shape == (3, 9) and float(ref["probabilities"].max()) < 0.999  # noqa: PLR2004
    return patches, model, ref


@pytest.mark.parametrize(("name", "dtype"), DTYPES, ids=IDS)
def test_patch_predictor_runs_from_bytes_to_probabilities_on_the_kernels(runs, name, dtype, caplog):
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViTClassifier

    patches, model, ref = runs
    eng = PatchPredictor(copy.deepcopy(model), batch_size=2, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        out = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype=name)
    assert not [r for r in caplog.records if "Vision Transformer" in r.getMessage() or "torch" in r.getMessage()]
    fast = eng._inference_model(dtype)  # noqa: SLF001  (the cached copy the run used)
    assert type(fast) is FusedViTClassifier and fast.half_dtype == dtype and eng._defer_norm is True  # noqa: SLF001
    _within_rule(out["probabilities"], _library(model, patches, dtype), ref["probabilities"], f"PatchPredictor vit_small {name}")
    assert np.array_equal(out["predictions"], ref["predictions"])
    assert float(np.abs(out["probabilities"].sum(-1) - 1).max()) <= 1e-6
    # the second run, from the uint8 patches on the host to the probabilities on the device
    kernels = _device_kernels(lambda: eng.infer_patches(eng.dataloader))
    for wanted in ("vit_patchify_norm_u8_h_kernel", "linear_softmax_rows_f32_kernel", "mha_fwd_h_kernel", "conv_mfma_h"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert _mha_head_dims(kernels) == {64}, kernels  # (the head_dim-64 instantiation of the one attention kernel, and no other)
    assert not {k for k in kernels if _banned(k) or _torch_kernel(k)}, kernels
    assert not any("vit_patchify_h_kernel" in k for k in kernels), kernels
    # a batch that is already on the device takes the same route to the same bits
    again = eng.run(torch.from_numpy(patches).cuda(), patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype=name)
    assert np.array_equal(again["probabilities"], out["probabilities"])


def test_feature_extractor_defers_the_hook_too(runs):
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    patches, model, _ = runs
    hook = timm_preproc_func(NAME)
    cpu = DeepFeatureExtractor(NAME, batch_size=2)
    cpu.model.feat_extract.load_state_dict(model.feat_extract.state_dict(), strict=True)
    cpu.model.preproc_func = hook
    ref = cpu.run(patches, patch_mode=True, ioconfig=_cfg())["probabilities"]
    eng = DeepFeatureExtractor(copy.deepcopy(cpu.model), batch_size=2, device="cuda")
    got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")["probabilities"]
    assert eng._defer_norm is True and got.shape == (3, 384)  # noqa: SLF001
    _within_rule(got, _library(cpu.model, patches, torch.bfloat16), ref, "DeepFeatureExtractor vit_small bf16 with the hook")
    kernels = _device_kernels(lambda: eng.infer_patches(eng.dataloader))
    assert any("vit_patchify_norm_u8_h_kernel" in k for k in kernels), kernels
    assert not {k for k in kernels if _banned(k) or _torch_kernel(k)}, kernels


@pytest.mark.parametrize(("name", "dtype"), DTYPES, ids=IDS)
def test_token_mean_patch14_classifier(name, dtype):
    """Virchow2's form (a 14-pixel patch: the padded columns; class + mean-patch features, ``F = 2 D``) through ``FusedViTClassifier``."""
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViTClassifier
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    model = timm_model(tiny_virchow(TINY_V2), num_classes=9)
    model.preproc_func = hook = timm_preproc_func("Virchow2")
    patches = np.random.default_rng(14).integers(0, 256, (3, 28, 28, 3), dtype=np.uint8)
    with torch.inference_mode():
        ref = model(hook.device_batch(torch.from_numpy(patches), torch.float32).permute(0, 3, 1, 2)).numpy()
        fused = FusedViTClassifier(copy.deepcopy(model).cuda())
        fused.feat_extract.prepare(dtype)
        fused = fused.to(dtype)
        x = torch.from_numpy(patches).cuda()
        got = fused.forward_uint8(x, hook.device_table("cuda", dtype))
        assert torch.equal(got, fused(hook.device_batch(x, dtype).permute(0, 3, 1, 2)))  # the same tokens, the same bits
    _within_rule(got.cpu().numpy(), _library(model, patches, dtype), ref, f"tiny token_mean patch 14 {name}")


def test_float32_keeps_the_torch_module_and_its_one_warning(runs, caplog):
    from tiatoolbox_amd.models import PatchPredictor

    patches, model, ref = runs
    eng = PatchPredictor(copy.deepcopy(model), batch_size=2, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        out = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype="float32")
        eng.run(patches[:1], patch_mode=True, ioconfig=_cfg(), compute_dtype="float32")  # the same inference copy: no second warning
    said = [r.getMessage() for r in caplog.records if "Vision Transformer" in r.getMessage()]
    assert len(said) == 1 and 'compute_dtype="bfloat16"' in said[0] and "library" in said[0] and "TimmModel" in said[0]
    fast = eng._inference_model(torch.float32)  # noqa: SLF001
    assert not {"FusedViT", "FusedViTClassifier"} & {type(m).__name__ for m in fast.modules()} and eng._defer_norm is False  # noqa: SLF001
    assert float(np.abs(out["probabilities"] - ref["probabilities"]).max()) <= 1e-4
    assert np.array_equal(out["predictions"], ref["predictions"])


def test_more_classes_than_the_head_kernel_takes(caplog):
    from tiatoolbox_amd.models import PatchPredictor

    patches = np.random.default_rng(3).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)  # (CPU margins 0.33 .. 0.5)
    model = _new_model(65)
    ref = PatchPredictor(copy.deepcopy(model), batch_size=4).run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True)
    eng = PatchPredictor(copy.deepcopy(model), batch_size=4, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        out = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype="bfloat16")
        eng.run(patches[:1], patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")
    said = [r.getMessage() for r in caplog.records if "head kernel" in r.getMessage()]
    assert len(said) == 1 and "64 classes" in said[0], said
    assert eng._defer_norm is True  # noqa: SLF001  (the trunk is the fused graph all the same)
    _within_rule(out["probabilities"], _library(model, patches, torch.bfloat16), ref["probabilities"], "65 classes bf16")
    assert np.array_equal(out["predictions"], ref["predictions"])


@pytest.mark.parametrize("case", ["own_infer_batch", "host_float_batch", "lambda_hook"])
def test_everything_else_takes_the_hook_as_it_is(runs, case, monkeypatch):
    """The normalisation is deferred for the stock models, a ``TimmNormPreproc`` hook and uint8 batches only; every other case runs
    the hook (batched on the device, or per patch for a callable the engine does not know) and matches all the same."""
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture import vit_fused
    from tiatoolbox_amd.models.architecture.vanilla import TimmModel

    patches, model, ref = runs
    deferred = []
    real = vit_fused.hip_vit_patchify_norm_u8_h
    monkeypatch.setattr(vit_fused, "hip_vit_patchify_norm_u8_h", lambda *a, **k: (deferred.append(1), real(*a, **k))[1])
    model, images = copy.deepcopy(model), patches
    if case == "own_infer_batch":
        class Own(TimmModel):
            @staticmethod
            def infer_batch(model, batch_data, device="cpu"):
                return TimmModel.infer_batch(model, batch_data, device)

        model.__class__ = Own
    elif case == "host_float_batch":
        images = patches.astype(np.float32) / np.float32(255)  # ToTensor's own division: the hook's float form normalises it
    else:
        hook = model.preproc_func
        model.preproc_func = lambda img: hook(img)  # noqa: PLW0108  (a callable the engine knows nothing about)
    eng = PatchPredictor(model, batch_size=2, device="cuda")
    out = eng.run(images, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype="bfloat16")
    assert not deferred and type(eng._inference_model(torch.bfloat16)).__name__ == "FusedViTClassifier"  # noqa: SLF001
    _within_rule(out["probabilities"], _library(runs[1], patches, torch.bfloat16), ref["probabilities"], case)
    assert np.array_equal(out["predictions"], ref["predictions"])
    # and the stock model, hook and batch beside it: deferred
    eng = PatchPredictor(copy.deepcopy(runs[1]), batch_size=2, device="cuda")
    eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")
    assert len(deferred) == 2  # noqa: PLR2004  (batches of 2 and 1)

"""``TimmModel`` (Vision Transformer + linear classifier + softmax), the ``TimmNormPreproc`` hook and ``PatchPredictor`` on them, on the
CPU; and the wiring of ``FusedViTClassifier`` / ``FusedViT.forward_uint8`` with the kernels' wrappers restated in torch."""

from __future__ import annotations

import copy
import pickle

import numpy as np
import pytest
import torch

from _vit_classifier_ref import all_bytes_batch, norm_formula, timm_model, torch_vit_wrappers
from _vit_ref import tiny_vit
from _vit_virchow_ref import TINY_V2, tiny_virchow

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
H_OPTIMUS = ((0.707223, 0.578729, 0.703617), (0.211883, 0.230117, 0.177517))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
CONSTANTS = {"UNI": IMAGENET, "UNI2": IMAGENET, "prov-gigapath": IMAGENET, "Virchow": IMAGENET, "Virchow2": IMAGENET,
             "H-optimus-0": H_OPTIMUS, "H-optimus-1": H_OPTIMUS,
             "vit_small_patch16_224": HALF, "vit_base_patch16_224": HALF, "vit_large_patch16_224": HALF}


# ------------------------------------------------------------------------------------------------------------------ TimmModel
def test_forward_is_softmax_of_linear_of_features():
    model = timm_model(num_classes=5)
    x = torch.randn((3, 3, 32, 32), generator=torch.Generator().manual_seed(1))
    with torch.inference_mode():
        got = model(x)
        feat = torch.flatten(model.feat_extract(x), 1)
        exp = torch.softmax(model.classifier(feat).float(), -1)
    assert got.shape == (3, 5) and got.dtype == torch.float32 and torch.equal(got, exp)
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-6 and float(got.max()) < 0.999  # (a classifier that says something)


def test_state_dict_is_timms_plus_classifier_and_round_trips_strictly():
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone, TimmModel
    from tiatoolbox_amd.models.models_abc import ModelABC

    model = TimmModel("vit_small_patch16_224", num_classes=9)
    assert isinstance(model, ModelABC) and model.num_classes == 9 and model.pretrained is False  # noqa: PLR2004
    sd = model.state_dict()
    trunk = [f"feat_extract.{k}" for k in TimmBackbone("vit_small_patch16_224").feat_extract.state_dict()]
    assert list(sd) == [*trunk, "classifier.weight", "classifier.bias"]
    assert sd["classifier.weight"].shape == (9, 384) and sd["classifier.bias"].shape == (9,)
    other = TimmModel("vit_small_patch16_224", num_classes=9)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.25)
    other.load_state_dict(model.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), other.state_dict().values()))
    with pytest.raises(RuntimeError, match="classifier"):
        other.load_state_dict({k: v for k, v in sd.items() if not k.startswith("classifier")}, strict=True)
    assert TimmModel.postproc(np.array([[0.1, 0.7, 0.2]])).tolist() == [1]


@pytest.mark.parametrize(("name", "width"), [("Virchow2", 2560), ("Virchow", 2560), ("UNI", 1024), ("H-optimus-1", 1536)])
def test_classifier_width_follows_the_pool(name, width):
    from tiatoolbox_amd.models.architecture.vanilla import TimmModel

    with torch.device("meta"):
        model = TimmModel(name, num_classes=4)
    assert model.classifier.in_features == width and model.classifier.out_features == 4  # noqa: PLR2004
    assert model.feat_extract.embed_dim * (2 if name.startswith("Virchow") else 1) == width


def test_token_mean_trunk_runs_at_twice_the_width():
    model = timm_model(tiny_virchow(TINY_V2), num_classes=3)
    assert model.classifier.in_features == 640  # noqa: PLR2004
    with torch.inference_mode():
        got = model(torch.randn((2, 3, 28, 28), generator=torch.Generator().manual_seed(2)))
    assert got.shape == (2, 3) and float((got.sum(-1) - 1).abs().max()) <= 1e-6


def test_unknown_backbones_raise_and_pretrained_reads_local_weights(tmp_path, monkeypatch, caplog):
    import logging

    from tiatoolbox_amd.models.architecture.vanilla import TimmModel
    from tiatoolbox_amd.models.architecture.vit import VIT_CONFIGS

    for bad in ("resnet18", "H0-mini", "efficientnet_b0", "uni"):
        with pytest.raises(ValueError, match=f"Backbone `{bad}` is not supported."):
            TimmModel(bad)
    monkeypatch.setitem(VIT_CONFIGS, "UNI", {"embed_dim": 128, "depth": 2, "num_heads": 2, "mlp_dim": 512, "patch_size": 16,
                                             "img_size": 32, "init_values": 1e-5, "dynamic_img_size": True})
    monkeypatch.setenv("TIA_WEIGHTS_DIR", str(tmp_path))
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    monkeypatch.delenv("TIATOOLBOX_HOME", raising=False)
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        TimmModel("UNI", 3, pretrained=True)
    assert sum("No local weights for `UNI`" in r.getMessage() for r in caplog.records) == 1
    sd = tiny_vit(seed=5).state_dict()
    torch.save(sd, tmp_path / "UNI.pth")
    loaded = TimmModel("UNI", 3, pretrained=True)
    assert loaded.pretrained and all(torch.equal(loaded.feat_extract.state_dict()[k], v) for k, v in sd.items())


# ------------------------------------------------------------------------------------------------------------ TimmNormPreproc
@pytest.mark.parametrize("constants", [IMAGENET, H_OPTIMUS, HALF], ids=["imagenet", "h-optimus", "half"])
def test_every_form_of_the_hook_is_the_formula_bit_for_bit(constants):
    from tiatoolbox_amd.models.dataset.classification import TimmNormPreproc

    hook = TimmNormPreproc(*constants)
    assert hook.table.shape == (256, 3) and hook.table.dtype == torch.float32 and hook.table.device.type == "cpu"
    x = all_bytes_batch(2, 16, 16, seed=3)
    for c in range(3):
        assert set(np.unique(x[..., c]).tolist()) == set(range(256))
    exp = torch.from_numpy(norm_formula(x, *constants))
    called = torch.stack([hook(p) for p in x])
    assert called.dtype == torch.float32 and torch.equal(called, exp)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        got = hook.device_batch(torch.from_numpy(x), dtype)
        assert got.dtype == dtype and got.shape == x.shape and torch.equal(got, exp.to(dtype))
        assert torch.equal(hook.device_table("cpu", dtype), hook.table.to(dtype))
    again = pickle.loads(pickle.dumps(hook))
    assert torch.equal(again.table, hook.table) and torch.equal(again(x[0]), called[0])
    # a float batch is already in ToTensor's range: Normalize alone
    unit = torch.from_numpy(x).float() / 255
    assert torch.equal(hook.device_batch(unit, torch.float32), (unit - torch.tensor(constants[0])) / torch.tensor(constants[1]))
    # deferral is for uint8 CUDA batches only: a CPU batch is looked up
    assert torch.equal(hook.device_batch(torch.from_numpy(x), torch.float32, defer_norm=True), exp)


def test_published_constants_and_unknown_names():
    from tiatoolbox_amd.models.architecture.vit import VIRCHOW_CONFIGS, VIT_CONFIGS
    from tiatoolbox_amd.models.dataset.classification import NormUInt8, TimmNormPreproc, predefined_preproc_func, timm_preproc_func

    assert set(CONSTANTS) == set(VIT_CONFIGS) | set(VIRCHOW_CONFIGS)  # every name create_vit builds
    for name, (mean, std) in CONSTANTS.items():
        hook = timm_preproc_func(name)
        assert type(hook) is TimmNormPreproc
        assert hook.mean.tolist() == np.asarray(mean, np.float32).tolist() and hook.std.tolist() == np.asarray(std, np.float32).tolist()
    for bad in ("kather100k", "uni", "resnet18"):
        with pytest.raises(ValueError, match=f"`{bad}` does not exist"):
            timm_preproc_func(bad)
    with pytest.raises(ValueError, match="positive"):
        TimmNormPreproc(0.5, 0.0)
    with pytest.raises(TypeError, match="uint8"):
        NormUInt8(torch.zeros(1, 2, 2, 3), timm_preproc_func("UNI"))
    for name in ("kather100k", "pcam"):  # the earlier registry keeps its two names
        assert predefined_preproc_func(name).preprocs == ["ToTensor"]
    with pytest.raises(ValueError, match="does not exist"):
        predefined_preproc_func("UNI")


# ------------------------------------------------------------------------------------------------------------- PatchPredictor
def test_patch_predictor_runs_a_timm_model_on_the_cpu():
    from tiatoolbox_amd.models import IOPatchPredictorConfig, PatchPredictor
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    model = timm_model(num_classes=9)
    model.preproc_func = hook = timm_preproc_func("vit_small_patch16_224")
    patches = np.random.default_rng(5).integers(0, 256, (5, 32, 32, 3), dtype=np.uint8)
    cfg = IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(32, 32),
                                 stride_shape=(32, 32))
    eng = PatchPredictor(model, batch_size=2)
    out = eng.run(patches, patch_mode=True, ioconfig=cfg, return_probabilities=True)
    probs, preds = out["probabilities"], out["predictions"]
    assert probs.shape == (5, 9) and probs.dtype == np.float32 and float(np.abs(probs.sum(-1) - 1).max()) <= 1e-6
    assert np.array_equal(preds, probs.argmax(-1)) and len(set(preds.tolist())) > 1
    with torch.inference_mode():
        exp = model(torch.stack([hook(p) for p in patches]).permute(0, 3, 1, 2)).numpy()
    assert float(np.abs(probs - exp).max()) <= 1e-6  # (batches of 2 and 1 against one batch of 5: float32 summation orders)
    assert "probabilities" not in eng.run(patches, patch_mode=True, ioconfig=cfg)


# ------------------------------------------------------------------------------------------------ the graph's wiring, no GPU
@pytest.fixture
def torch_wrappers(monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    calls: dict = {}
    for name, fn in torch_vit_wrappers(calls).items():
        monkeypatch.setattr(vit_fused, name, fn, raising=False)  # (raising=False: without the feature the test fails further down)
    return calls


@pytest.mark.parametrize("form", ["patch16", "virchow2"])
def test_fused_classifier_wiring(torch_wrappers, form):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT, FusedViTClassifier
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    model = timm_model(num_classes=9) if form == "patch16" else timm_model(tiny_virchow(TINY_V2), num_classes=9)
    size = 32 if form == "patch16" else 28
    hook, dtype = timm_preproc_func("UNI"), torch.float16
    x = torch.from_numpy(all_bytes_batch(2, size, size, seed=6))
    fused = FusedViTClassifier(copy.deepcopy(model))
    assert isinstance(fused.feat_extract, FusedViT) and fused.head_kernel and fused.num_classes == 9  # noqa: PLR2004
    assert fused._w32.dtype == torch.float32 and torch.equal(fused._w32, model.classifier.weight.detach())  # noqa: SLF001
    fused.feat_extract.prepare(dtype)
    fused = fused.to(dtype)
    assert fused._w32.dtype == torch.float32 and fused.half_dtype == dtype  # noqa: SLF001  (the cast does not reach the head)
    table = hook.device_table("cpu", dtype)
    with torch.inference_mode():
        got = fused.forward_uint8(x, table)
        assert torch_wrappers == {"hip_vit_patchify_norm_u8_h": 1, "hip_linear_softmax_rows_f32": 1}
        same = fused(hook.device_batch(x, dtype).permute(0, 3, 1, 2))
        assert torch_wrappers == {"hip_vit_patchify_norm_u8_h": 1, "hip_linear_softmax_rows_f32": 2}
        feat = fused.feat_extract.forward_uint8(x, table)
        ref = model(hook.device_batch(x, torch.float32).permute(0, 3, 1, 2))
    assert got.shape == (2, 9) and got.dtype == torch.float32 and torch.equal(got, same)
    assert feat.shape == (2, model.classifier.in_features) and feat.dtype == torch.float32
    # fp16 activations (2^-11) through two blocks against the float32 module: a wiring mistake -- a channel order, a missing norm, a
    # head on the wrong rows -- moves a probability by tenths
    assert float((got - ref).abs().max()) <= 2e-2, float((got - ref).abs().max())
    assert torch.equal(got.argmax(-1), ref.argmax(-1))


def test_fused_classifier_refusals_and_wide_heads(torch_wrappers, caplog):
    import logging

    from tiatoolbox_amd.models.architecture.unet_fused import UnsupportedLayerError
    from tiatoolbox_amd.models.architecture.vit_fused import HEAD_MAX_CLASSES, FusedViT, FusedViTClassifier

    assert HEAD_MAX_CLASSES == 64 and FusedViT.accepts_uint8 is False  # noqa: PLR2004
    with pytest.raises(UnsupportedLayerError, match="head_dim 64"):
        FusedViTClassifier(timm_model(num_classes=3, num_heads=4))
    with pytest.raises(UnsupportedLayerError, match="TimmModel"):
        FusedViTClassifier(torch.nn.Sequential())
    fused = FusedViTClassifier(timm_model(num_classes=3))
    x = torch.zeros((1, 32, 32, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="prepare"):
        fused.forward_uint8(x, torch.zeros(256, 3, dtype=torch.float16))
    fused.feat_extract.prepare(torch.float16)
    with pytest.raises(ValueError, match="uint8"):
        fused.forward_uint8(x.float(), torch.zeros(256, 3, dtype=torch.float16))
    with pytest.raises(ValueError, match="multiple of the patch size"):
        fused.forward_uint8(torch.zeros((1, 40, 32, 3), dtype=torch.uint8), torch.zeros(256, 3, dtype=torch.float16))
    model = timm_model(num_classes=65)
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        wide = FusedViTClassifier(model)
    said = [r.getMessage() for r in caplog.records if "head kernel" in r.getMessage()]
    assert len(said) == 1 and "64 classes" in said[0] and not wide.head_kernel
    wide.feat_extract.prepare(torch.float16)
    with torch.inference_mode():
        got = wide.to(torch.float16)(torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(3)).half())
    assert got.shape == (2, 65) and got.dtype == torch.float32 and "hip_linear_softmax_rows_f32" not in torch_wrappers


def test_engine_defers_for_the_stock_models_only():
    """``_set_defer_norm`` on stand-in inference copies (no GPU): the rule of ``_set_defer_unit`` with a flag of its own."""
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone, TimmModel
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT, FusedViTClassifier

    def flag(model, *, prepared=True, device="cuda"):
        eng = PatchPredictor(model, batch_size=2)
        fast = copy.deepcopy(model)
        if type(fast).forward is TimmModel.forward and isinstance(fast, TimmModel):
            fast = FusedViTClassifier(fast)
        else:
            fast.feat_extract = FusedViT(fast.feat_extract)
        if prepared:
            fast.feat_extract.half_dtype = torch.bfloat16  # (what `prepare` leaves behind; nothing is packed here)
        eng.device = device
        eng._set_defer_norm(fast)  # noqa: SLF001
        assert not getattr(eng, "_defer_unit", False)
        return eng._defer_norm  # noqa: SLF001

    class OwnInfer(TimmModel):
        @staticmethod
        def infer_batch(model, batch_data, device="cpu"):
            return TimmModel.infer_batch(model, batch_data, device)

    class OwnForward(TimmModel):
        def forward(self, imgs):
            return super().forward(imgs * 1.0)

    def swap(model):
        model.feat_extract = tiny_vit()
        return model

    backbone = swap(TimmBackbone("vit_small_patch16_224"))
    assert flag(timm_model(num_classes=3)) is True and flag(backbone) is True
    assert flag(timm_model(num_classes=3), device="cpu") is False and flag(timm_model(num_classes=3), prepared=False) is False
    for cls in (OwnInfer, OwnForward):
        with torch.device("meta"):
            sub = cls("vit_small_patch16_224", 3)
        sub.feat_extract, sub.classifier = tiny_vit(), torch.nn.Linear(128, 3)
        assert flag(sub) is False
    eng = PatchPredictor(timm_model(num_classes=3), batch_size=2)
    eng._set_defer_norm(copy.deepcopy(eng.model))  # noqa: SLF001  (the torch module as inference copy: float32, the CPU, a refusal)
    assert eng._defer_norm is False  # noqa: SLF001

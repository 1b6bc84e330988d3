"""``return_cam`` / ``merge_cam``: class activation maps of the ``CNNModel`` classifiers (``models/engine/_cam.py`` states the quantity).

Host tests of the statement, the patch-mode run kwarg, every refusal and the static ``PatchPredictor.merge_cam``.  WSI mode itself
reads its patches with a HIP kernel (there is no host form of it), so the run with ``merge_cam=True`` at the end of this file carries
the ``gpu`` mark; what it writes is compared with the host NumPy loop."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _attention_merge_ref as ref  # noqa: E402

U = 2.0 ** -24  # unit round-off of float32


def _cfg(stride: int = 64):
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(64, 64),
                                  stride_shape=(stride, stride))


def _engine(backbone: str = "resnet18", classes: int = 3, device: str = "cpu", batch_size: int = 4):
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture.vanilla import CNNModel

    torch.manual_seed(7)
    return PatchPredictor(CNNModel(backbone, num_classes=classes).eval(), batch_size=batch_size, device=device, verbose=False)


@pytest.fixture(scope="module")
def patches():
    return np.random.default_rng(3).random((4, 64, 64, 3), dtype=np.float32)


@pytest.fixture(scope="module")
def runs(patches):
    """One engine, three runs: without the kwarg, with it (the module's own trunk output kept by a hook), and without it again."""
    eng = _engine()
    plain = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True)
    kept = []
    handle = eng.model.feat_extract.register_forward_hook(lambda _m, _i, out: kept.append(out.detach().clone()))
    try:
        with_cam = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, return_cam=True)
    finally:
        handle.remove()
    after = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True)
    return eng, plain, with_cam, after, torch.cat(kept)


def cam_bound(features, weight) -> np.ndarray:
    """``(C + 8) 2^-24 sum_c |W[k, c] F[n, c, y, x]| + 2^-120`` per entry, in float64: what every order of C float32 multiply-adds keeps
    to first order (the 8: slack for the second-order term)."""
    f, w = np.asarray(features, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    return (f.shape[1] + 8) * U * np.einsum("kc,nchw->nkhw", np.abs(w), np.abs(f)) + 2.0 ** -120


def test_statement_against_float64():
    from tiatoolbox_amd.models.engine import _cam

    rng = np.random.default_rng(0)
    f, w, b = np.abs(rng.standard_normal((3, 64, 2, 5))).astype(np.float32), rng.standard_normal((4, 64)).astype(np.float32), rng.standard_normal(4)
    got = _cam.class_activation_maps(f, w)
    exact = np.einsum("kc,nchw->nkhw", w.astype(np.float64), f.astype(np.float64))
    assert got.dtype == np.float32 and got.shape == (3, 4, 2, 5)
    assert (np.abs(got - exact) <= cam_bound(f, w)).all()
    # the same from half tensors, widened; and the torch form
    fh = torch.from_numpy(f).to(torch.bfloat16)
    assert np.array_equal(_cam.class_activation_maps(fh, w), _cam.class_activation_maps(fh.float().numpy(), w))
    tt = _cam.cam_torch(torch.from_numpy(f), torch.from_numpy(w))
    assert tt.dtype == torch.float32 and (np.abs(tt.numpy() - exact) <= cam_bound(f, w)).all()
    # the bias convention: the map leaves the bias out, and its mean plus the bias is the logit
    logits = _cam.logits_from_maps(got, b.astype(np.float32))
    exact_logits = np.einsum("kc,nc->nk", w.astype(np.float64), f.astype(np.float64).mean((2, 3))) + b.astype(np.float32)[None]
    assert np.abs(logits - exact_logits).max() <= 1e-5
    with pytest.raises(ValueError, match="must agree"):
        _cam.class_activation_maps(f, w[:, :32])


def test_patch_mode_maps(runs):
    from tiatoolbox_amd.models.engine import _cam

    eng, plain, with_cam, after, feat = runs
    cam = with_cam["cam"]
    assert isinstance(cam, np.ndarray) and cam.dtype == np.float32 and cam.shape == (4, 3, 2, 2)
    assert feat.shape == (4, 512, 2, 2)
    weight, bias = eng.model.classifier.weight.detach().numpy(), eng.model.classifier.bias.detach().numpy()
    stated = _cam.class_activation_maps(feat, weight)
    assert (np.abs(cam.astype(np.float64) - stated) <= 2 * cam_bound(feat.numpy(), weight)).all()  # (two float32 orders of summation)
    exact = np.einsum("kc,nchw->nkhw", weight.astype(np.float64), feat.numpy().astype(np.float64))
    assert (np.abs(cam - exact) <= cam_bound(feat.numpy(), weight)).all()
    assert np.abs(cam).max() > 0
    # softmax(mean(cam) + b) is the run's probability
    logits = _cam.logits_from_maps(cam, bias)
    e = np.exp(logits - logits.max(1, keepdims=True))
    assert np.abs(e / e.sum(1, keepdims=True) - with_cam["probabilities"]).max() <= 1e-6


def test_other_keys_are_bit_identical_and_nothing_stays_behind(runs):
    eng, plain, with_cam, after, _ = runs
    assert sorted(with_cam) == sorted([*plain, "cam"]) and "cam" not in plain and "cam" not in after
    for key in plain:
        assert np.array_equal(plain[key], with_cam[key]) and np.array_equal(plain[key], after[key]), key
        assert plain[key].dtype == with_cam[key].dtype
    from tiatoolbox_amd.models import PatchPredictor

    assert not hasattr(eng, "return_cam") and "merge_cam" not in vars(eng) and not hasattr(eng, "cam_interpolation")
    assert eng.merge_cam is PatchPredictor.merge_cam
    assert eng._return_cam is False and eng._merge_cam is False  # noqa: SLF001  (the per-call state is reset by the next call)
    assert not eng.model.feat_extract._forward_hooks  # noqa: SLF001  (the scope's hook is gone)


def test_resnext50_shape():
    eng = _engine("resnext50_32x4d", classes=2, batch_size=2)
    out = eng.run(np.random.default_rng(1).random((2, 64, 64, 3), dtype=np.float32), patch_mode=True, ioconfig=_cfg(), return_cam=True)
    assert out["cam"].shape == (2, 2, 2, 2) and out["cam"].dtype == np.float32 and eng.model.classifier.in_features == 2048  # noqa: PLR2004
    assert "probabilities" not in out and out["predictions"].shape == (2,)


def test_refusals(tmp_path, patches):
    """Everything the two options do not cover is a ``ValueError`` that names the option and what it got, before any launch (on a
    machine without a device: before WSI mode would fail for lack of one), and leaves nothing of the call behind."""
    from _vit_ref import tiny_vit

    from tiatoolbox_amd.models import DeepFeatureExtractor, PatchPredictor
    from tiatoolbox_amd.models.architecture.vanilla import CNNBackbone, CNNModel, TimmModel

    slides = [np.zeros((96, 128, 3), np.uint8)]
    eng = _engine()
    for bad in (1, "yes", None, np.True_):
        with pytest.raises(ValueError, match="return_cam .* and merge_cam .* are bool .*got return_cam="):
            eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_cam=bad, compute_dtype="bfloat16")
        with pytest.raises(ValueError, match="got merge_cam="):
            eng.run(slides, patch_mode=False, ioconfig=_cfg(), merge_cam=bad, save_dir=tmp_path / "a")
    assert eng.compute_dtype == "float32"  # refused before any kwarg of the call became an attribute
    with pytest.raises(ValueError, match=r"return_cam=True with patch_mode=False \(WSI mode has merge_cam\)"):
        eng.run(slides, patch_mode=False, ioconfig=_cfg(), return_cam=True, save_dir=tmp_path / "b")
    with pytest.raises(ValueError, match=r"merge_cam=True with patch_mode=True \(patch mode has return_cam\)"):
        eng.run(patches, patch_mode=True, ioconfig=_cfg(), merge_cam=True)
    with pytest.raises(ValueError, match="cam_interpolation='cubic'"):
        eng.run(slides, patch_mode=False, ioconfig=_cfg(), merge_cam=True, cam_interpolation="cubic", save_dir=tmp_path / "c")
    assert not hasattr(eng, "return_cam") and "merge_cam" not in vars(eng) and not hasattr(eng, "cam_interpolation")
    assert eng._return_cam is False and eng._merge_cam is False and not list(tmp_path.iterdir())  # noqa: SLF001

    # a Vision Transformer classifier: return_attention gives its maps
    with torch.device("meta"):
        vit = TimmModel("vit_small_patch16_224", num_classes=3)
    vit.feat_extract = tiny_vit()
    vit.classifier = torch.nn.Linear(vit.feat_extract.embed_dim, 3)
    timm = PatchPredictor(vit.eval(), batch_size=2, device="cpu", verbose=False)
    with pytest.raises(ValueError, match="return_cam=True for TimmModel.*return_attention gives its maps"):
        timm.run(patches, patch_mode=True, ioconfig=_cfg(), return_cam=True)
    with pytest.raises(ValueError, match="merge_cam=True for TimmModel.*merge_attention gives its maps"):
        timm.run(slides, patch_mode=False, ioconfig=_cfg(), merge_cam=True, save_dir=tmp_path / "d")

    # feature extractors have no classifier: the model class under PatchPredictor, both kwargs under DeepFeatureExtractor
    backbone = PatchPredictor(CNNBackbone("resnet18").eval(), batch_size=2, device="cpu", verbose=False)
    with pytest.raises(ValueError, match="return_cam=True for CNNBackbone, a feature extractor: it has no classifier"):
        backbone.run(patches, patch_mode=True, ioconfig=_cfg(), return_cam=True)
    for model in (CNNBackbone("resnet18").eval(), eng.model):
        dfe = DeepFeatureExtractor(model, batch_size=2, device="cpu", verbose=False)
        with pytest.raises(ValueError, match="no classifier; got return_cam=True for DeepFeatureExtractor"):
            dfe.run(patches, patch_mode=True, ioconfig=_cfg(), return_cam=True)
        with pytest.raises(ValueError, match="no classifier; got merge_cam=True for DeepFeatureExtractor"):
            dfe.run(slides, patch_mode=False, ioconfig=_cfg(), merge_cam=True, save_dir=tmp_path / "e")
        assert "cam" not in dfe.run(patches[:2], patch_mode=True, ioconfig=_cfg(), return_cam=False)  # (False asks for nothing)

    # any other model class: a CNNModel subclass with its own forward, another pool, another head
    class Own(CNNModel):
        def forward(self, imgs):
            return super().forward(imgs) * 1.0

    torch.manual_seed(0)
    own = PatchPredictor(Own("resnet18", num_classes=3).eval(), batch_size=2, device="cpu", verbose=False)
    with pytest.raises(ValueError, match="return_cam=True for Own, which is no CNNModel with the stock forward"):
        own.run(patches, patch_mode=True, ioconfig=_cfg(), return_cam=True)
    maxpool = _engine()
    maxpool.model.pool = torch.nn.AdaptiveMaxPool2d((1, 1))
    with pytest.raises(ValueError, match="which is no CNNModel with the stock forward, pool and nn.Linear"):
        maxpool.run(patches, patch_mode=True, ioconfig=_cfg(), return_cam=True)
    mlp = _engine()
    mlp.model.classifier = torch.nn.Sequential(torch.nn.Linear(512, 3))
    with pytest.raises(ValueError, match="pool and nn.Linear classifier"):
        mlp.run(patches, patch_mode=True, ioconfig=_cfg(), return_cam=True)
    assert not list(tmp_path.iterdir())
    # return_attention's own refusal of these models is as it was
    with pytest.raises(ValueError, match="no VisionTransformer"):
        eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_attention="class")


class _Slide:
    """What ``merge_cam`` reads of a slide reader (an ``ArrayWSIReader`` itself lives on the device)."""

    def __init__(self, width: int, height: int, mpp: float = 0.5, power: float = 20.0) -> None:
        self.slide_dimensions, self.mpp, self.power = (width, height), mpp, power


def test_static_merge_cam_on_a_dict_and_on_a_file(tmp_path):
    """The maps of a patch-mode run on an overlapping grid (64-pixel patches at stride 32 on a 160 x 96 slide, 8 patches), merged by the
    static method, equal the NumPy loop of ``_attention_merge`` and its independent restatement bit for bit, for both interpolations."""
    from tiatoolbox_amd.models import DeepFeatureExtractor, PatchPredictor
    from tiatoolbox_amd.models.engine import _attention_merge as am

    ws, hs = 160, 96
    slide = np.random.default_rng(5).random((hs, ws, 3), dtype=np.float32)
    coords = np.array([(x, y, x + 64, y + 64) for y in range(0, hs - 32, 32) for x in range(0, ws - 32, 32)], dtype=np.int64)
    tiles = np.stack([np.pad(slide[y0:y1, x0:x1], ((0, 64 - (min(y1, hs) - y0)), (0, 64 - (min(x1, ws) - x0)), (0, 0))) for x0, y0, x1, y1 in coords])
    eng = _engine(batch_size=5)
    cam = eng.run(tiles, patch_mode=True, ioconfig=_cfg(32), return_cam=True)["cam"]
    assert cam.shape == (len(coords), 3, 2, 2) and len(coords) == 8  # noqa: PLR2004
    reader, canvas = _Slide(ws, hs), (24, 40)  # 5x of a 20x slide: ratio 4
    output = {"coordinates": coords, "cam": cam, "resolution": 20.0, "units": "power"}
    merged = {}
    for mode in ("bilinear", "nearest"):
        exp = am.merge_patch_grids(coords, cam, (ws, hs), canvas, interpolation=mode, want=("raw", "count"), device="cpu")
        got, cover = PatchPredictor.merge_cam(reader, output, resolution=5.0, units="power", interpolation=mode, return_count=True)
        assert got.dtype == np.float32 and got.shape == (3, *canvas) and np.array_equal(got, exp["raw"])
        assert cover.dtype == np.int32 and np.array_equal(cover, exp["count"]) and cover.max() >= 4  # noqa: PLR2004
        assert np.array_equal(got, ref.merge(coords, cam, (ws, hs), canvas, mode)["raw"])
        merged[mode] = got
    assert not np.array_equal(merged["bilinear"], merged["nearest"])
    path = tmp_path / "slide.npz"
    np.savez(path, coordinates=coords, cam=cam, resolution=1.0, units="baseline")
    assert np.array_equal(PatchPredictor.merge_cam(reader, path, resolution=5.0), merged["bilinear"])
    assert PatchPredictor.merge_cam(reader, str(path)).shape == (3, 6, 10)  # the default: 1.25x, ratio 16
    assert DeepFeatureExtractor.merge_cam is PatchPredictor.merge_cam
    with pytest.raises(ValueError, match="merge_cam needs output\\['resolution'\\]"):
        PatchPredictor.merge_cam(reader, {"coordinates": coords, "cam": cam})
    with pytest.raises(ValueError, match="'cam'"):
        PatchPredictor.merge_cam(reader, {"coordinates": coords, "attention": cam, "resolution": 20.0, "units": "power"})
    with pytest.raises(ValueError, match="interpolation"):
        PatchPredictor.merge_cam(reader, output, interpolation="cubic")


def _load(path) -> dict:
    with np.load(path) as data:
        return {k: data[k] for k in data.files}


@pytest.mark.gpu
def test_wsi_mode_merge_cam(tmp_path):
    """A slide of 208 x 152 pixels, 64 x 64 patches at stride 32 (an overlapping grid): the ``.npz`` holds ``cam``, ``merged_cam`` and
    ``cam_coverage``; ``cam`` is bit for bit what a patch-mode ``return_cam`` run returns for the patches read at ``coordinates``;
    ``merged_cam`` is the NumPy loop on it, bit for bit, for both interpolations; the static method gives the same array; every other
    key is that of the run without the kwarg, whose file has exactly today's keys."""
    from tiatoolbox_amd.models import IOPatchPredictorConfig, PatchPredictor
    from tiatoolbox_amd.models.engine import _attention_merge as am
    from tiatoolbox_amd.utils import synth
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    cfg = IOPatchPredictorConfig(input_resolutions=[{"units": "mpp", "resolution": 0.5}], patch_input_shape=(64, 64), stride_shape=(32, 32))
    base = ArrayWSIReader(synth.g_he(1, 152, 208, seed=5)[0], mpp=0.5, power=20.0)
    eng = _engine(device="cuda", batch_size=6)
    kw = {"patch_mode": False, "ioconfig": cfg, "auto_get_mask": False, "return_probabilities": True}
    plain = _load(eng.run([base], save_dir=tmp_path / "plain", **kw)[0])
    assert sorted(plain) == ["coordinates", "predictions", "probabilities"]
    canvas = (38, 52)  # 5x of a 20x slide of 208 x 152: ratio 4
    out = {}
    for mode in ("bilinear", "nearest"):
        out[mode] = got = _load(eng.run([base], save_dir=tmp_path / mode, merge_cam=True, cam_interpolation=mode, merge_resolution=5.0,
                                        merge_units="power", merge_predictions=mode == "nearest", **kw)[0])
        added = ["cam", "cam_coverage", "merged_cam", *(["merged_predictions", "merged_probabilities"] if mode == "nearest" else [])]
        assert sorted(got) == sorted([*plain, *added])
        for key in plain:
            assert np.array_equal(got[key], plain[key]), key
        coords = got["coordinates"]
        assert len(coords) >= 15 and got["cam"].shape == (len(coords), 3, 2, 2) and got["cam"].dtype == np.float32  # noqa: PLR2004
        exp = am.merge_patch_grids(coords, got["cam"], (208, 152), canvas, interpolation=mode, want=("raw", "count"), device="cpu")
        assert got["merged_cam"].shape == (3, *canvas) and got["merged_cam"].dtype == np.float32 and got["cam_coverage"].dtype == np.int32
        assert np.array_equal(got["merged_cam"], exp["raw"]) and np.array_equal(got["cam_coverage"], exp["count"]) and exp["count"].max() >= 4  # noqa: PLR2004
        assert np.array_equal(exp["raw"], ref.merge(coords, got["cam"], (208, 152), canvas, mode)["raw"])
        told = got | {"resolution": 0.5, "units": "mpp"}
        assert np.array_equal(PatchPredictor.merge_cam(base, told, resolution=5.0, interpolation=mode), got["merged_cam"])
    assert np.array_equal(out["bilinear"]["cam"], out["nearest"]["cam"])
    assert not np.array_equal(out["bilinear"]["merged_cam"], out["nearest"]["merged_cam"])
    tiles = base.read_bounds_batch(coords).cpu().numpy()
    per_patch = eng.run(tiles, patch_mode=True, ioconfig=cfg, return_cam=True)["cam"]
    assert np.array_equal(out["bilinear"]["cam"], per_patch)
    assert eng.merge_cam is PatchPredictor.merge_cam  # the run option did not become an attribute
    assert sorted(_load(eng.run([base], save_dir=tmp_path / "after", **kw)[0])) == sorted(plain)

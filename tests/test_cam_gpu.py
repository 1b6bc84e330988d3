"""``return_cam`` / ``merge_cam`` on the device: the engine's maps against float64 on the feature map the forward left behind, the bias
convention against the run's own logits and probabilities, what the option launches, and one WSI-mode run."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
from tiatoolbox_amd.utils import synth

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
HALF_U = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}


@pytest.fixture(scope="module")
def patches():
    return synth.g_he(4, 224, 224, seed=41)


def _softmax(logits: np.ndarray) -> np.ndarray:
    e = np.exp(logits - logits.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _check_engine(name: str, patches, *, compute_dtype: str, conv_algo: str | None, trunk: str) -> None:
    from torch.profiler import ProfilerActivity, profile

    x = torch.from_numpy(patches).cuda()
    eng = PatchPredictor(name, batch_size=2, device="cuda", verbose=False)
    kw = {"patch_mode": True, "return_probabilities": True, "compute_dtype": compute_dtype}
    if conv_algo is not None:
        kw["conv_algo"] = conv_algo
    eng.run(x, **kw)  # builds the inference copy; library convolutions (the folded module) settle on their solvers
    plain = eng.run(x, **kw)
    fast = eng._inference_model(torch.float32 if compute_dtype == "float32" else getattr(torch, compute_dtype))  # noqa: SLF001
    assert type(fast.feat_extract).__name__ == trunk and fast is not eng.model
    feats, logits = [], []
    hooks = [fast.feat_extract.register_forward_hook(lambda _m, _i, out: feats.append(out.detach().clone())),
             fast.classifier.register_forward_hook(lambda _m, _i, out: logits.append(out.detach().clone()))]
    try:
        got = eng.run(x, return_cam=True, **kw)
    finally:
        for h in hooks:
            h.remove()
    assert fast is eng._inference_model(next(fast.parameters()).dtype)  # noqa: SLF001  (the same copy ran)
    feat, logit = torch.cat(feats), torch.cat(logits).double().cpu().numpy()
    want_dtype = getattr(torch, compute_dtype)
    assert feat.dtype == want_dtype and fast.classifier.weight.dtype == want_dtype and len(feats) == 2  # noqa: PLR2004

    # every other key bit for bit, and nothing left behind
    assert sorted(got) == sorted([*plain, "cam"])
    again = eng.run(x, **kw)
    for key in plain:
        assert np.array_equal(plain[key], again[key]), f"{key}: two runs without the kwarg differ (the route itself is not reproducible)"
        assert np.array_equal(plain[key], got[key]), key
    assert not hasattr(eng, "return_cam") and not fast.feat_extract._forward_hooks  # noqa: SLF001

    # the maps against float64 on the captured feature map and the copy's weights, both widened
    cam = got["cam"]
    n, c, h, w = feat.shape
    k = fast.classifier.out_features
    assert cam.dtype == np.float32 and cam.shape == (4, k, h, w) and (h, w) == (7, 7) and k == 9  # noqa: PLR2004
    f64, w64 = feat.double().cpu().numpy(), fast.classifier.weight.detach().double().cpu().numpy()
    b64 = fast.classifier.bias.detach().double().cpu().numpy()
    ref = np.einsum("kc,nchw->nkhw", w64, f64)
    s = np.einsum("kc,nchw->nkhw", np.abs(w64), np.abs(f64))
    err = np.abs(cam.astype(np.float64) - ref)
    bound = (c + 8) * U32 * s + 2.0 ** -120
    print(f"{name} {compute_dtype} {conv_algo}: cam error at most {float((err / bound).max()):.3f} of the bound")
    assert (err <= bound).all(), float((err / bound).max())
    assert np.abs(cam).max() > 0

    # the bias convention: mean(cam) + b against the logits the classifier produced, softmax of it against the run's probabilities
    from tiatoolbox_amd.models.engine import _cam

    from_maps = _cam.logits_from_maps(cam, b64)
    t = np.einsum("kc,nc->nk", np.abs(w64), np.abs(f64).mean((2, 3))) + np.abs(b64)[None]  # sum_c |W| gap + |b|  (gap >= 0 after the ReLU)
    if compute_dtype == "float32":
        # maps: (c + 8) u per entry, kept by the mean; torch: the pooled features (h w + 2) u each, the Linear (c + 8) u, the sum with
        # the bias and its rounding 2 u -- all relative to t
        logit_bound = (2 * (c + 8) + h * w + 4) * U32 * t
    else:
        logit_bound = 3 * HALF_U[compute_dtype] * t  # torch rounds the pooled features and the logit once each; 3 covers both and the float32 terms
    gap = np.abs(from_maps - logit)
    print(f"{name} {compute_dtype} {conv_algo}: logits at most {float((gap / logit_bound).max()):.3f} of the bound")
    assert (gap <= logit_bound).all(), float((gap / logit_bound).max())
    # |d softmax_k| <= p_k (|d l_k| + max_j |d l_j|) <= 2 max_j |d l_j|; the run's softmax is float32 on the (widened) logits
    prob_bound = 2 * logit_bound.max(1, keepdims=True) + 8 * U32
    assert (np.abs(_softmax(from_maps) - got["probabilities"]) <= prob_bound).all()

    # what the option launches: one cam kernel per batch and nothing else
    def kernel_names(**extra):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            eng.run(x, **extra, **kw)
            torch.cuda.synchronize()
        events = [e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()]
        return [n for n in events if "memcpy" not in n.lower() and "memset" not in n.lower()]

    without, with_maps = kernel_names(), kernel_names(return_cam=True)
    assert [n for n in without if "cam" in n] == []
    assert len([n for n in with_maps if "cam" in n]) == 2 and all("cam_nhwc_kernel" in n for n in with_maps if "cam" in n)  # noqa: PLR2004
    assert {n for n in with_maps if "cam" not in n} == set(without)
    assert len(with_maps) == len(without) + 2


@pytest.mark.parametrize("name", ["resnet18-kather100k", "resnet50-kather100k"])
def test_float32(patches, name, conv_algo):
    _check_engine(name, patches, compute_dtype="float32", conv_algo=conv_algo, trunk="MfmaResNet")


@pytest.mark.parametrize("compute_dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", ["resnet18-kather100k", "resnet50-kather100k"])
def test_half(patches, name, compute_dtype):
    _check_engine(name, patches, compute_dtype=compute_dtype, conv_algo=None, trunk="MfmaResNet")


def test_half_resnext_on_the_folded_module(patches):
    """Half-precision ResNeXt runs the BatchNorm-folded torch module; its output goes through the same kernel.  The module's
    convolutions are the library's, and left to choose freely the library does not repeat its own bits from one run to the next
    (measured on an MI355X: two runs WITHOUT the kwarg differ by up to 6e-6 in the probabilities), which would hide what the kwarg
    does; so every run of this test, with and without the kwarg, asks the library for its deterministic solvers."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        _check_engine("resnext50_32x4d-kather100k", patches, compute_dtype="float16", conv_algo=None, trunk="Sequential")
    finally:
        torch.backends.cudnn.deterministic = before


def test_wsi_mode(tmp_path):
    """One WSI-mode run of ``resnet18-kather100k`` in bf16 on a 560 x 448 slide, 224-pixel patches at stride 112: ``merged_cam`` equals the
    NumPy loop applied to the file's own ``cam``, bit for bit, and ``cam`` the patch-mode maps of the same patches."""
    from tiatoolbox_amd.models import IOPatchPredictorConfig
    from tiatoolbox_amd.models.engine import _attention_merge as am
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    cfg = IOPatchPredictorConfig(input_resolutions=[{"units": "mpp", "resolution": 0.5}], patch_input_shape=(224, 224), stride_shape=(112, 112))
    base = ArrayWSIReader(synth.g_he(1, 448, 560, seed=9)[0], mpp=0.5, power=20.0)
    eng = PatchPredictor("resnet18-kather100k", batch_size=8, device="cuda", verbose=False)
    kw = {"ioconfig": cfg, "compute_dtype": "bfloat16"}
    path = eng.run([base], patch_mode=False, save_dir=tmp_path / "out", auto_get_mask=False, merge_cam=True, merge_resolution=2.5,
                   merge_units="power", **kw)[0]
    with np.load(path) as data:
        out = {key: data[key] for key in data.files}
    assert sorted(out) == ["cam", "cam_coverage", "coordinates", "merged_cam", "predictions"]
    coords, canvas = out["coordinates"], (56, 70)  # 2.5x of a 20x slide of 560 x 448: ratio 8
    assert len(coords) >= 12 and out["cam"].shape == (len(coords), 9, 7, 7) and out["cam"].dtype == np.float32  # noqa: PLR2004
    exp = am.merge_patch_grids(coords, out["cam"], (560, 448), canvas, want=("raw", "count"), device="cpu")
    assert out["merged_cam"].shape == (9, *canvas) and out["merged_cam"].dtype == np.float32
    assert np.array_equal(out["merged_cam"], exp["raw"]) and np.array_equal(out["cam_coverage"], exp["count"]) and exp["count"].max() >= 4  # noqa: PLR2004
    tiles = base.read_bounds_batch(coords)
    per_patch = eng.run(tiles, patch_mode=True, return_cam=True, **kw)
    assert np.array_equal(per_patch["cam"], out["cam"]) and np.array_equal(per_patch["predictions"], out["predictions"])

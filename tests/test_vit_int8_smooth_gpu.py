"""``FusedViT`` with ``linear_dtype="int8", smoothing=scales`` and the engines' ``int8_smoothing`` on the device: the smoothed graph
against the smoothed yardstick (``_vit_int8_smooth_ref.smoothed_fake_quantised_module``, at most twice its error against the float32
module) on the model forms of the INT8 tests with outlier channels, the calibration against torch statistics of the same graph, bit
identity with the unsmoothed graph under all-ones scales, routing of a layer off the INT8 shapes, and both engines from uint8 patches."""

from __future__ import annotations

import copy
import logging

import numpy as np
import pytest
import torch

from _vit_classifier_ref import redraw_classifier
from _vit_foundation_ref import TINY_REG, tiny_foundation
from _vit_int8_ref import gelu64, layernorm64, rel_error, swiglu64
from _vit_int8_smooth_ref import absmax64, calibration_case, near_tie_columns, smoothed_fake_quantised_module, with_outliers
from _vit_ref import randomise, tiny_vit
from _vit_virchow_ref import TINY_V2, tiny_virchow
from test_vit_gpu import _banned, _device_kernels

pytestmark = pytest.mark.gpu

INT8 = "int8"
BF16 = torch.bfloat16
SMOOTH_KERNEL = "act_rows_smooth_kernel<tia::q8::Int8"


def _calibrate(vit, batches, alpha: float = 0.5) -> dict[str, torch.Tensor]:
    from tiatoolbox_amd.models.architecture.vit_fused import calibrate_int8_smoothing

    return calibrate_int8_smoothing(copy.deepcopy(vit).cuda(), [b.cuda() for b in batches], alpha=alpha)


def _graph(vit, smoothing=None):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(copy.deepcopy(vit).cuda())
    fused.prepare(BF16, linear_dtype=INT8, **({} if smoothing is None else {"smoothing": smoothing}))
    return fused.to(BF16)


def _device_input(x: torch.Tensor) -> torch.Tensor:
    return x.cuda().to(BF16).contiguous(memory_format=torch.channels_last)


FORMS = {
    "tiny-ls": (lambda: tiny_vit(layer_scale=True), (64, 64)),
    "tiny-no-ls": (lambda: tiny_vit(layer_scale=False), (64, 64)),
    "registers-swiglu": (lambda: tiny_foundation({**TINY_REG, "reg_tokens": 4}), (42, 56)),
    "token-mean": (lambda: tiny_virchow(TINY_V2), (28, 28)),
}


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_smoothed_graph_matches_the_smoothed_yardstick(form, n):
    """Scenario B (one LayerNorm channel x 60 in front of ``qkv`` and ``fc1``, one ``fc1`` output channel x 30), scales calibrated on
    the device on 8 other patches: ``e_graph <= 2 e_yardstick`` against the float32 module on the CPU.  The unsmoothed graph's error
    on the same model is printed beside it, not gated."""
    make, (h, w) = FORMS[form]
    vit = with_outliers(make(), "B")
    g = torch.Generator().manual_seed(40 + n)
    x, cal = torch.randn((n, 3, h, w), generator=g), torch.randn((8, 3, h, w), generator=g)
    scales = _calibrate(vit, [cal])
    with torch.inference_mode():
        ref = vit(x)
        yard = smoothed_fake_quantised_module(copy.deepcopy(vit).cuda(), scales)(x.cuda().to(BF16)).float()
        fused = _graph(vit, scales)
        got, unsmoothed = fused(_device_input(x)), _graph(vit)(_device_input(x))
    assert fused.linear_dtype == INT8 and set(fused.smoothing) == set(scales) and got.shape == ref.shape and got.dtype == torch.float32
    smoothed_fc2 = [layer["fc2"].inv_smooth is not None for layer in fused.layers]
    assert all(smoothed_fc2) and all(k.endswith("fc2") for k in scales) == (form == "token-mean")
    e_new, e_yard = rel_error(got, ref), rel_error(yard, ref)
    print(f"{form} n={n}: e_smoothed_graph {e_new:.3e}  e_smoothed_yardstick {e_yard:.3e}  |  not gated: unsmoothed graph e {rel_error(unsmoothed, ref):.3e}")
    assert bool(torch.isfinite(got).all()) and e_new <= 2.0 * e_yard


def test_device_calibration_is_the_torch_statistics_of_the_same_graph(monkeypatch):
    """The scales calibrated on the device equal those from torch statistics -- float64 LayerNorm / GELU of the very tensors the
    bfloat16 graph hands its taps -- except, by at most one binade, on columns whose real exponent sits within 1e-3 of a rounding
    tie; those columns are counted and may be at most 1 % of all."""
    from tiatoolbox_amd.models.architecture import vit_fused

    vit, batches = calibration_case()
    ref64: dict[int, torch.Tensor] = {}
    seen = {}
    ln_tap, act_tap, begin = vit_fused.hip_layernorm_rows_absmax_h, vit_fused.hip_act_rows_absmax_h, vit_fused.FusedViT.begin_int8_calibration

    def keep(amax, v64):
        new = absmax64(v64)
        ref64[amax.data_ptr()] = torch.maximum(ref64[amax.data_ptr()], new) if amax.data_ptr() in ref64 else new

    def ln_and_reference(x, gamma, beta, amax, *, eps):
        keep(amax, layernorm64(x.reshape(-1, x.shape[-1]), gamma, beta, eps))
        return ln_tap(x, gamma, beta, amax, eps=eps)

    def act_and_reference(x, amax, *, swiglu):
        keep(amax, (swiglu64 if swiglu else gelu64)(x.reshape(-1, x.shape[-1])))
        return act_tap(x, amax, swiglu=swiglu)

    def begin_and_keep(self):
        begin(self)
        seen["graph"] = self

    monkeypatch.setattr(vit_fused, "hip_layernorm_rows_absmax_h", ln_and_reference)
    monkeypatch.setattr(vit_fused, "hip_act_rows_absmax_h", act_and_reference)
    monkeypatch.setattr(vit_fused.FusedViT, "begin_int8_calibration", begin_and_keep)
    scales = _calibrate(vit, batches)
    graph = seen["graph"]
    assert set(scales) == {f"blocks.{i}.{n}" for i in range(2) for n in ("attn.qkv", "mlp.fc1", "mlp.fc2")}
    total = near = moved = 0
    for name, tap in graph._taps.items():  # noqa: SLF001
        amax_w = graph._amax_w[name]  # noqa: SLF001
        want = vit_fused.int8_smoothing_scales(ref64[tap.data_ptr()], amax_w, 0.5)
        tie = near_tie_columns(ref64[tap.data_ptr()], amax_w, 0.5)
        differ = scales[name] != want
        ratio = scales[name][differ] / want[differ]
        assert bool((differ <= tie).all()) and bool(((ratio == 2.0) | (ratio == 0.5)).all()), (name, int(differ.sum()))  # noqa: PLR2004
        total, near, moved = total + tap.numel(), near + int(tie.sum()), moved + int(differ.sum())
    print(f"{moved} of {total} scales differ from the torch reference; {near} columns within 1e-3 of a rounding tie")
    assert total == 2 * (128 + 128 + 512) and near <= total // 100
    assert float(scales["blocks.0.attn.qkv"][5]) >= 16.0 and float(scales["blocks.1.mlp.fc2"][7]) >= 4.0  # the outlier channels  # noqa: PLR2004


def test_all_ones_scales_and_repeated_forwards_are_bit_identical():
    vit = with_outliers(tiny_vit(layer_scale=True, embed_dim=384, num_heads=6, mlp_dim=1536, img_size=224), "B")
    swiglu = tiny_foundation({**TINY_REG, "reg_tokens": 4})
    for model, shape in ((vit, (3, 3, 224, 224)), (swiglu, (2, 3, 42, 56))):
        g = torch.Generator().manual_seed(3)
        x, cal = _device_input(torch.randn(shape, generator=g)), torch.randn(shape, generator=g)
        scales = _calibrate(model, [cal])
        ones = {k: torch.ones_like(v) for k, v in scales.items()}
        with torch.inference_mode():
            plain, unit, smooth = _graph(model), _graph(model, ones), _graph(model, scales)
            want, got = plain(x), unit(x)
            first, second, other = smooth(x), smooth(x), _graph(model, scales)(x)
            kernels = _device_kernels(lambda unit=unit, x=x: unit(x))
        assert any(SMOOTH_KERNEL in k for k in kernels), kernels  # the all-ones graph did run the smoothed producer
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(first.view(torch.int32), second.view(torch.int32)) and torch.equal(first.view(torch.int32), other.view(torch.int32))
        assert not torch.equal(first, want)


def test_a_layer_off_the_int8_shapes_is_neither_smoothed_nor_quantised(caplog):
    """``mlp_dim = 576``: ``fc2`` (576 -> 128) is off the INT8 GEMM's ``K % 128`` and stays on the half kernel behind the half GELU; the
    calibration has no entry for it, and one given anyway is ignored with an ``info`` line."""
    vit = with_outliers(tiny_vit(mlp_dim=576), "A")
    g = torch.Generator().manual_seed(2)
    x, cal = torch.randn((2, 3, 32, 32), generator=g), torch.randn((8, 3, 32, 32), generator=g)
    scales = _calibrate(vit, [cal])
    assert set(scales) == {f"blocks.{i}.{n}" for i in range(2) for n in ("attn.qkv", "mlp.fc1")}
    with caplog.at_level(logging.INFO, logger="tiatoolbox_amd"):
        fused = _graph(vit, {**scales, "blocks.0.mlp.fc2": torch.ones(576)})
    said = [r.getMessage() for r in caplog.records]
    kept = [m for m in said if "layer(s) stay on the half kernel:" in m]
    ignored = [m for m in said if "ignored" in m]
    assert len(kept) == 1 and "blocks.0.mlp.fc2" in kept[0] and "blocks.1.mlp.fc2" in kept[0] and "fc1" not in kept[0], said
    assert len(ignored) == 1 and "blocks.0.mlp.fc2" in ignored[0] and "neither smoothed nor quantised" in ignored[0], said
    assert set(fused.smoothing) == set(scales) and all(type(layer["fc2"]).__name__ == "_Linear" for layer in fused.layers)
    with torch.inference_mode():
        kernels = _device_kernels(lambda: fused(x.cuda().to(BF16)))
        ref = vit(x)
        yard = smoothed_fake_quantised_module(copy.deepcopy(vit).cuda(), scales)(x.cuda().to(BF16)).float()
        got = fused(x.cuda().to(BF16))
    assert any("gelu_rows_h_kernel" in k for k in kernels) and not any("act_rows" in k for k in kernels), kernels
    assert any("linear_rows_kernel<tia::q8::Int8" in k for k in kernels) and any("layernorm_rows_kernel<tia::q8::Int8" in k for k in kernels), kernels
    assert rel_error(got, ref) <= 2.0 * rel_error(yard, ref)


# ------------------------------------------------------------------------------------------------------------------- the engines
NAME = "vit_small_patch16_224"


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def _check_engine(eng, patches, calibration, key: str, extra_kernels=()) -> None:
    run = lambda **kw: eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype=INT8, **kw)[key]  # noqa: E731
    first = run(int8_smoothing=0.5, int8_calibration=calibration)
    scales = eng.int8_smoothing_scales
    fast = eng._inference_model(BF16)  # noqa: SLF001  (the cached copy the run used)
    graphs = [m for m in fast.modules() if type(m).__name__ == "FusedViT"]
    assert len(graphs) == 1 and graphs[0].linear_dtype == INT8 and eng._defer_norm is True  # noqa: SLF001
    assert isinstance(scales, dict) and len(scales) == 3 * 12 and set(graphs[0].smoothing) == set(scales)  # noqa: PLR2004
    assert all(torch.equal(graphs[0].smoothing[k], scales[k]) for k in scales) and any(bool((v != 1.0).any()) for v in scales.values())
    assert np.isfinite(first).all() and eng.int8_smoothing == 0.5 and eng.int8_calibration is calibration  # noqa: PLR2004
    kernels = _device_kernels(lambda: eng.infer_patches(eng.dataloader))
    for wanted in ("vit_patchify_norm_u8_h_kernel", SMOOTH_KERNEL, "linear_rows_kernel<tia::q8::Int8", "layernorm_rows_kernel<tia::q8::Int8", *extra_kernels):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert not any("act_rows_kernel<tia::q8::Int8" in k or "absmax" in k for k in kernels), kernels  # no unsmoothed producer, no calibration
    assert not {k for k in kernels if _banned(k)}, kernels
    # the same alpha and no new calibration: the cached copy, not another calibration
    assert np.array_equal(run(), first) and eng._inference_model(BF16) is fast and eng.int8_smoothing_scales is scales  # noqa: SLF001
    # the returned scales dict in place of the patches: the same bits
    assert np.array_equal(run(int8_smoothing=0.5, int8_calibration=scales), first) and eng.int8_smoothing_scales is scales
    # and the unsmoothed option is another copy with other bits
    eng.int8_smoothing = eng.int8_calibration = None
    plain = eng.run(patches, patch_mode=True, ioconfig=_cfg(), return_probabilities=True, compute_dtype=INT8)[key]
    assert [m.smoothing for m in eng._inference_model(BF16).modules() if type(m).__name__ == "FusedViT"] == [None]  # noqa: SLF001
    assert not np.array_equal(plain, first)


def test_feature_extractor_runs_smoothed_int8_from_uint8_patches():
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    rng = np.random.default_rng(0)
    patches, calibration = rng.integers(0, 256, (3, 224, 224, 3), dtype=np.uint8), rng.integers(0, 256, (5, 224, 224, 3), dtype=np.uint8)
    eng = DeepFeatureExtractor(NAME, batch_size=2, device="cuda")
    randomise(eng.model.feat_extract)
    eng.model.preproc_func = timm_preproc_func(NAME)
    _check_engine(eng, patches, calibration, "probabilities")


def test_patch_predictor_runs_a_timm_model_in_smoothed_int8():
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture.vanilla import TimmModel
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    torch.manual_seed(0)
    model = TimmModel(NAME, 9)
    randomise(model.feat_extract)
    redraw_classifier(model.classifier)
    model.preproc_func = timm_preproc_func(NAME)
    rng = np.random.default_rng(8)
    patches, calibration = rng.integers(0, 256, (4, 224, 224, 3), dtype=np.uint8), rng.integers(0, 256, (5, 224, 224, 3), dtype=np.uint8)
    eng = PatchPredictor(model.eval(), batch_size=4, device="cuda")
    _check_engine(eng, patches, torch.from_numpy(calibration), "probabilities", extra_kernels=("linear_softmax_rows_f32_kernel",))

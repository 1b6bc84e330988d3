"""``int8_smoothing`` without a GPU: the scales formula against known answers, the exactness of the power-of-two recipe, the accuracy
gates on the two outlier scenarios, the wiring of the smoothed graph on torch stand-ins of its wrappers with faults that each must
fail, every new refusal of ``prepare`` and of the engines, and the ``torch.save`` round trip of a calibration."""

from __future__ import annotations

import copy
import functools
import inspect
import logging
from pathlib import Path

import numpy as np
import pytest
import torch

from _vit_int8_ref import fake_quantised_module, rel_error, torch_int8_wrappers
from _vit_int8_smooth_ref import (absmax64, reference_calibration, routed_linears, smoothed_fake_quantised_module, torch_smooth_wrappers,
                                  with_outliers)
from _vit_ref import tiny_vit
from _vit_virchow_ref import TINY_V2, tiny_virchow

INT8 = "int8"
BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------- the symbols
def test_symbols_and_signatures():
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture import vit_fused

    for name in ("int8_smoothing_scales", "calibrate_int8_smoothing", "hip_act_rows_qi8_smooth", "hip_layernorm_rows_absmax_h",
                 "hip_act_rows_absmax_h"):
        assert hasattr(vit_fused, name), name
    assert list(inspect.signature(vit_fused.FusedViT.prepare).parameters) == ["self", "dtype", "linear_dtype", "residual_dtype", "smoothing"]
    assert list(inspect.signature(vit_fused.FusedViTClassifier.prepare).parameters) == ["self", "dtype", "linear_dtype", "residual_dtype", "smoothing"]
    assert list(inspect.signature(vit_fused.hip_act_rows_qi8_smooth).parameters) == ["x", "inv_smooth", "swiglu"]
    assert inspect.signature(vit_fused.calibrate_int8_smoothing).parameters["alpha"].default == 0.5  # noqa: PLR2004
    sig, lib = _lib._SIGNATURES, _lib.load()  # noqa: SLF001
    for plain, smooth in (("tia_gelu_rows_qi8", "tia_gelu_rows_qi8_smooth"), ("tia_swiglu_rows_qi8", "tia_swiglu_rows_qi8_smooth")):
        assert sig[smooth][0] == [sig[plain][0][0], sig[plain][0][0], *sig[plain][0][1:]] and hasattr(lib, smooth)  # one pointer more
    assert sig["tia_gelu_rows_absmax_h"] == sig["tia_swiglu_rows_absmax_h"] and len(sig["tia_layernorm_rows_absmax_h"][0]) == 10  # noqa: PLR2004
    assert lib.tia_abi_version() == 6  # additive  # noqa: PLR2004
    header = (Path(__file__).resolve().parents[1] / "include" / "tiatoolbox_amd.h").read_text()
    for name in ("tia_gelu_rows_qi8_smooth", "tia_swiglu_rows_qi8_smooth", "tia_layernorm_rows_absmax_h", "tia_gelu_rows_absmax_h",
                 "tia_swiglu_rows_absmax_h"):
        assert f"int {name}(" in header, name


# ------------------------------------------------------------------------------------------------------------ the scales formula
def test_scales_are_the_stated_powers_of_two():
    from tiatoolbox_amd.models.architecture.vit_fused import int8_smoothing_scales

    # alpha = 0.5: e = round(0.5 log2 a - 0.5 log2 w).  (a, w) = (64, 1) -> 3 -> 8;  (1, 16) -> -2 -> 0.25;  (4, 4) -> 0 -> 1;
    # (2, 1) -> 0.5 -> ties to even 0 -> 1;  (8, 1) -> 1.5 -> 2 -> 4;  (60, 1 / 60) -> 5.9 -> 6 -> 64
    a = torch.tensor([64.0, 1.0, 4.0, 2.0, 8.0, 60.0])
    w = torch.tensor([1.0, 16.0, 4.0, 1.0, 1.0, 1.0 / 60.0])
    s = int8_smoothing_scales(a, w, 0.5)
    assert s.dtype == torch.float32 and s.tolist() == [8.0, 0.25, 1.0, 1.0, 4.0, 64.0]
    # alpha = 1: the activation range alone;  alpha = 0.25: 0.25 * 8 - 0.75 * -4 = 5
    assert int8_smoothing_scales(torch.tensor([32.0, 0.125]), torch.tensor([7.0, 7.0]), 1.0).tolist() == [32.0, 0.125]
    assert int8_smoothing_scales(torch.tensor([256.0]), torch.tensor([1.0 / 16.0]), 0.25).tolist() == [32.0]
    # the clamp at 2^+-24, and 1 where the activation or the weight column is zero (a SwiGLU pad lane is both)
    s = int8_smoothing_scales(torch.tensor([1e30, 1e-30, 0.0, 5.0, 0.0]), torch.tensor([1e-30, 1e30, 3.0, 0.0, 0.0]), 0.5)
    assert s.tolist() == [2.0 ** 24, 2.0 ** -24, 1.0, 1.0, 1.0]
    # float64 on the host: half-precision and device inputs change nothing, and every result is a power of two
    g = torch.Generator().manual_seed(0)
    a, w = torch.rand(512, generator=g) * 100.0, torch.rand(512, generator=g)
    s = int8_smoothing_scales(a, w, 0.5)
    mantissa, _ = torch.frexp(s)
    assert bool((mantissa == 0.5).all()) and torch.equal(s, int8_smoothing_scales(a.double(), w.double()))  # noqa: PLR2004
    want = torch.exp2(torch.round(0.5 * torch.log2(a.double()) - 0.5 * torch.log2(w.double()))).float()
    assert torch.equal(s, want)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_scales_refuse_non_finite_activations_and_a_bad_alpha(bad):
    from tiatoolbox_amd.models.architecture.vit_fused import int8_smoothing_scales

    with pytest.raises(ValueError, match="not finite.*calibration data produced non-finite activations"):
        int8_smoothing_scales(torch.tensor([1.0, bad, 2.0]), torch.ones(3), 0.5)
    for alpha in (0.0, -0.5, 1.5, None, "0.5", True):
        with pytest.raises(ValueError, match=r"alpha lies in \(0, 1\]"):
            int8_smoothing_scales(torch.ones(3), torch.ones(3), alpha)
    with pytest.raises(ValueError, match="3 activation maxima beside 4 weight columns"):
        int8_smoothing_scales(torch.ones(3), torch.ones(4), 0.5)


# --------------------------------------------------------------------------------------------------------------------- the wiring
@pytest.fixture
def stand_ins(monkeypatch):
    """``vit_fused`` with every wrapper ``FusedViT`` calls replaced by its torch restatement: the half ones of ``_vit_classifier_ref``,
    the INT8 ones of ``_vit_int8_ref`` and the smoothing ones of ``_vit_int8_smooth_ref``."""
    from _vit_classifier_ref import torch_vit_wrappers

    from tiatoolbox_amd.models.architecture import vit_fused

    table = {**torch_vit_wrappers({}), **torch_int8_wrappers(), **torch_smooth_wrappers()}
    for name, fn in table.items():
        monkeypatch.setattr(vit_fused, name, fn)
    return table


def _graph(vit, smoothing=None):
    from tiatoolbox_amd.models.architecture import vit_fused

    fused = vit_fused.FusedViT(copy.deepcopy(vit))
    fused.prepare(BF16, linear_dtype=INT8, **({} if smoothing is None else {"smoothing": smoothing}))
    return fused.to(BF16)


def _pow2_scales(vit, seed: int = 0, span: int = 4) -> dict[str, torch.Tensor]:
    """Arbitrary powers of two in 2^-span .. 2^span for every layer the INT8 GEMM serves, at the graph's (padded) widths."""
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    probe = FusedViT(copy.deepcopy(vit))
    probe._pad_swiglu_for_quant()  # noqa: SLF001
    g = torch.Generator().manual_seed(seed)
    return {layer[n].name: torch.exp2(torch.randint(-span, span + 1, (layer[n].cin,), generator=g).float())
            for layer in probe.layers for n in ("qkv", "fc1", "fc2") if layer[n].cin % 128 == 0 and layer[n].cout % 16 == 0}


def _eval_batch(seed: int = 0, n: int = 4, size: int = 64) -> torch.Tensor:
    return torch.randn((n, 3, size, size), generator=torch.Generator().manual_seed(100 + seed))


def test_all_ones_scales_reproduce_the_unsmoothed_graph_bit_for_bit(stand_ins):
    for vit, x in ((tiny_vit(), _eval_batch(0, 2, 32)), (tiny_virchow(TINY_V2), _eval_batch(1, 2, 28))):
        ones = {k: torch.ones_like(v) for k, v in _pow2_scales(vit).items()}
        with torch.inference_mode():
            plain, smooth = _graph(vit), _graph(vit, ones)
            want, got = plain(x.to(BF16)), smooth(x.to(BF16))
        assert smooth.smoothing is not None and plain.smoothing is None and set(smooth.smoothing) == set(ones)
        assert all(layer["fc2"].inv_smooth is not None for layer in smooth.layers)  # the smoothed producer did run
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        for a, b in zip(plain.layers, smooth.layers):
            for name in ("qkv", "fc1", "fc2"):
                if type(a[name]).__name__ == "_LinearInt8":
                    assert torch.equal(a[name].packed.codes, b[name].packed.codes) and torch.equal(a[name].packed.scales, b[name].packed.scales)


def test_the_folded_layernorm_is_the_unfolded_one_divided_by_s(stand_ins):
    """With arbitrary powers of two: the folded LayerNorm's dequantised output times ``s`` equals the float64 LayerNorm within the
    quantisation bound -- half a code step of that row, ``_vit_int8_ref.quantised_rows_figures``'s bound, in units of ``s[j]``."""
    from _vit_int8_ref import layernorm64

    g = torch.Generator().manual_seed(3)
    d = 256
    x = (torch.randn((1, 37, d), generator=g) * 2.0 + 0.5).to(BF16)
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.1
    gamma[5], beta[5] = gamma[5] * 60.0, beta[5] * 60.0
    s = torch.exp2(torch.randint(-6, 7, (d,), generator=g).float())
    s[5] = 64.0
    rows = stand_ins["hip_layernorm_rows_qi8"](x, gamma / s, beta / s, eps=1e-6)
    assert torch.equal((gamma / s) * s, gamma) and torch.equal((beta / s) * s, beta)  # the fold is exact
    want = layernorm64(x.reshape(-1, d), gamma, beta, 1e-6)
    row_scale = rows.scales.double()[:, None]
    got = rows.codes.reshape(-1, d).double() * row_scale * s.double()
    bound = (0.5 * row_scale * (1.0 + 2.0 ** -10) + 2.0 ** -10 * row_scale) * s.double()
    worst = float(((got - want).abs() / bound).max())
    print(f"folded LayerNorm: worst element {worst:.3f} of its bound")
    assert worst <= 1.0


def test_smoothing_leaves_the_real_valued_gemm_unchanged(stand_ins):
    """``W' = W s`` and ``x' = x / s`` are exact in float32, so ``x' W'^T == x W^T`` as real numbers: checked in float64 on the weights
    a smoothed ``prepare`` hands to the packer."""
    from tiatoolbox_amd.models.architecture import vit_fused

    vit = with_outliers(tiny_vit(), "B")
    scales = _pow2_scales(vit, seed=2, span=8)
    packed = {}
    pack = vit_fused.pack_linear_weights_int8

    def keep(weight):
        packed[len(packed)] = weight.detach().clone()
        return pack(weight)

    vit_fused.pack_linear_weights_int8 = keep
    try:
        fused = _graph(vit, scales)
    finally:
        vit_fused.pack_linear_weights_int8 = pack
    unsmoothed = vit_fused.FusedViT(copy.deepcopy(vit))
    order = [(layer[n].name, layer[n].weight32) for layer in unsmoothed.layers for n in ("qkv", "fc1", "fc2")]
    assert len(packed) == len(order) == 6  # noqa: PLR2004
    g = torch.Generator().manual_seed(4)
    for i, (name, w) in enumerate(order):
        s, w_s = scales[name], packed[i]
        assert torch.equal(w_s / s, w) and torch.equal(fused.smoothing[name], s)  # W s is exact
        x = torch.randn((9, w.shape[1]), generator=g)
        assert torch.equal((x / s) * s, x)  # x / s is exact
        y, y_s = x.double() @ w.double().T, (x / s).double() @ w_s.double().T
        assert float((y - y_s).abs().max()) <= 1e-12 * float(y.abs().max())
    for layer, plain in zip(fused.layers, unsmoothed.layers):  # the affine in front of qkv / fc1 carries 1 / s; fc2's producer gets it
        assert torch.equal(layer["norm1"][0] * scales[layer["qkv"].name], plain["norm1"][0])
        assert torch.equal(layer["norm2"][1] * scales[layer["fc1"].name], plain["norm2"][1])
        assert torch.equal(layer["fc2"].inv_smooth * scales[layer["fc2"].name], torch.ones_like(layer["fc2"].inv_smooth))


# ------------------------------------------------------------------------------------------------------------------ the accuracy
@functools.lru_cache(maxsize=None)
def _accuracy_figures(depth: int, carrier: torch.dtype, seed: int) -> dict[str, float]:
    """Everything against the float32 module of the same weights, on 4 evaluation patches; scales calibrated (alpha = 0.5) on 8 others
    through the bfloat16 graph on its torch stand-ins.  ``e_plain``: the unsmoothed yardstick on the model without outliers."""
    vit = tiny_vit(depth=depth, seed=seed)
    x, cal = _eval_batch(seed), torch.randn((8, 3, 64, 64), generator=torch.Generator().manual_seed(500 + seed))
    out = {}
    with torch.inference_mode():
        for tag, model in (("none", vit), ("A", with_outliers(vit, "A")), ("B", with_outliers(vit, "B"))):
            ref = model(x)
            scales, _, _ = reference_calibration(model, cal, 0.5)
            out[f"unsmoothed_{tag}"] = rel_error(fake_quantised_module(copy.deepcopy(model), carrier)(x.to(carrier)).float(), ref)
            out[f"smooth_{tag}"] = rel_error(smoothed_fake_quantised_module(copy.deepcopy(model), scales, carrier)(x.to(carrier)).float(), ref)
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("carrier", [torch.float32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("depth", [2, 8])
def test_smoothing_restores_the_accuracy_of_a_model_without_outliers(depth, carrier, seed):
    e = _accuracy_figures(depth, carrier, seed)
    e_plain = e["unsmoothed_none"]
    print(f"depth {depth} {carrier} seed {seed}: e_plain {e_plain:.3e} | A: unsmoothed {e['unsmoothed_A']:.3e} smooth {e['smooth_A']:.3e} "
          f"({e['smooth_A'] / e_plain:.2f} x e_plain) | B: unsmoothed {e['unsmoothed_B']:.3e} smooth {e['smooth_B']:.3e} "
          f"({e['smooth_B'] / e_plain:.2f} x) | no outliers, smoothing on {e['smooth_none']:.3e} ({e['smooth_none'] / e_plain:.2f} x)")
    k = 3.0
    assert e["smooth_A"] <= k * e_plain and e["smooth_B"] <= k * e_plain
    assert e["unsmoothed_A"] >= 4.0 * e["smooth_A"]
    assert e["smooth_none"] <= 2.0 * e_plain


# ---------------------------------------------------------------------------------------------------------- the graph and its faults
@functools.lru_cache(maxsize=None)
def _scenario_b():
    vit = with_outliers(tiny_vit(), "B")
    cal = torch.randn((8, 3, 64, 64), generator=torch.Generator().manual_seed(77))
    return vit, _eval_batch(5), reference_calibration(vit, cal, 0.5)[0]


def _parity(fused, vit, x, scales) -> tuple[float, float]:
    with torch.inference_mode():
        ref = vit(x)
        yard = smoothed_fake_quantised_module(copy.deepcopy(vit), scales)(x.to(BF16)).float()
        got = fused(x.to(BF16))
    e_new, e_yard = rel_error(got, ref), rel_error(yard, ref)
    print(f"e_smoothed_graph {e_new:.3e}  e_smoothed_yardstick {e_yard:.3e}")
    return e_new, e_yard


def test_wiring_matches_the_smoothed_yardstick(stand_ins):
    vit, x, scales = _scenario_b()
    assert set(scales) == {f"blocks.{i}.{n}" for i in range(2) for n in ("attn.qkv", "mlp.fc1", "mlp.fc2")}
    assert float(scales["blocks.0.attn.qkv"][5]) >= 16.0 and float(scales["blocks.0.mlp.fc2"][7]) >= 4.0  # the outlier channels  # noqa: PLR2004
    fused = _graph(vit, scales)
    assert fused.linear_dtype == INT8 and all(torch.equal(fused.smoothing[k], scales[k]) for k in scales)
    e_new, e_yard = _parity(fused, vit, x, scales)
    assert e_new <= 2.0 * e_yard
    # the same model unsmoothed is what the README warns of: several times further from the float32 module
    with torch.inference_mode():
        e_unsmoothed = rel_error(_graph(vit)(x.to(BF16)), vit(x))
    print(f"unsmoothed graph on the same model: {e_unsmoothed:.3e}")
    assert e_unsmoothed >= 3.0 * e_new
    # the token-mean form: qkv and fc1 stay half (K = 320), fc2 is smoothed at its padded width 640 and the pad lanes keep scale 1
    vit = tiny_virchow(TINY_V2)
    x = _eval_batch(6, 2, 28)
    scales, amax_x, _ = reference_calibration(vit, _eval_batch(7, 4, 28), 0.5)
    assert set(scales) == {"blocks.0.mlp.fc2", "blocks.1.mlp.fc2"} and scales["blocks.0.mlp.fc2"].shape == (640,)
    assert bool((scales["blocks.0.mlp.fc2"][520:] == 1.0).all()) and not bool(amax_x["blocks.0.mlp.fc2"][520:].any())
    fused = _graph(vit, scales)
    assert not bool(fused.layers[0]["fc2"].packed.codes[:, 520:].any())
    e_new, e_yard = _parity(fused, vit, x, scales)
    assert e_new <= 2.0 * e_yard


def test_the_calibration_statistics_are_the_column_maxima_of_the_producers(stand_ins):
    """The taps sit where the quantising producers sit: block 0's ``qkv`` statistics are the float64 LayerNorm of the assembled tokens,
    and two calibration batches accumulate to the maximum over both."""
    vit, _, _ = _scenario_b()
    a, b = _eval_batch(8, 3), _eval_batch(9, 2)
    _, both, amax_w = reference_calibration(vit, [a, b], 0.5)
    _, first, _ = reference_calibration(vit, a, 0.5)
    _, second, _ = reference_calibration(vit, b, 0.5)
    for name in both:
        assert torch.equal(both[name], torch.maximum(first[name], second[name])), name
    lin = routed_linears(vit)
    for name, w in amax_w.items():  # LayerScale folds into fc2's rows: the column maxima are those of the folded weights
        gamma = getattr(vit.blocks[int(name.split(".")[1])], "ls2").gamma if name.endswith("fc2") else None
        folded = lin[name].weight.detach() * (gamma[:, None] if gamma is not None else 1.0)
        assert torch.allclose(w, absmax64(folded.T.contiguous().T).float(), rtol=1e-6), name
    assert float(both["blocks.0.attn.qkv"][5]) > 10.0 * float(both["blocks.0.attn.qkv"].median())  # noqa: PLR2004


def _fault_fails(fused) -> None:
    vit, x, scales = _scenario_b()
    e_new, e_yard = _parity(fused, vit, x, scales)
    assert e_new > 2.0 * e_yard


def test_fault_weights_scaled_but_the_layernorm_affine_not_folded(stand_ins):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    vit, _, scales = _scenario_b()
    fused, plain = _graph(vit, scales), FusedViT(copy.deepcopy(vit))
    for layer, orig in zip(fused.layers, plain.layers):
        layer["norm1"], layer["norm2"] = orig["norm1"], orig["norm2"]
    _fault_fails(fused)


def test_fault_fc2_inv_smooth_dropped(stand_ins):
    vit, _, scales = _scenario_b()
    fused = _graph(vit, scales)
    for layer in fused.layers:
        layer["fc2"].inv_smooth = None  # the unsmoothed producer in front of weights that carry s
    _fault_fails(fused)


def test_fault_fc1_scales_given_to_qkv(stand_ins):
    """``qkv`` and ``fc1`` have the same ``cin``: a LayerNorm in front of ``qkv`` folded with ``fc1``'s scales has the right length, and
    only the numbers tell."""
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    vit, _, scales = _scenario_b()
    assert scales["blocks.0.attn.qkv"].shape == scales["blocks.0.mlp.fc1"].shape
    assert not torch.equal(scales["blocks.0.attn.qkv"], scales["blocks.0.mlp.fc1"])
    fused, plain = _graph(vit, scales), FusedViT(copy.deepcopy(vit))
    for layer, orig in zip(fused.layers, plain.layers):
        layer["norm1"] = tuple(t / scales[layer["fc1"].name] for t in orig["norm1"])
    _fault_fails(fused)


def test_fault_a_scale_of_three_is_refused(stand_ins):
    vit, _, scales = _scenario_b()
    bad = {k: v.clone() for k, v in scales.items()}
    bad["blocks.1.mlp.fc1"][11] = 3.0
    with pytest.raises(ValueError, match=r"smoothing\['blocks.1.mlp.fc1'\].*powers of two.*channel 11 is 3.0"):
        _graph(vit, bad)


# ----------------------------------------------------------------------------------------------------------------- the refusals
def test_prepare_refuses_what_smoothing_does_not_cover(stand_ins, caplog):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    vit, _, scales = _scenario_b()

    def refused(match, smoothing, dtype=BF16, **kw):
        fused = FusedViT(copy.deepcopy(vit))
        with pytest.raises(ValueError, match=match):
            fused.prepare(dtype, smoothing=smoothing, **kw)
        assert fused.half_dtype is None and fused.linear_dtype is None and fused.smoothing is None  # nothing is packed or folded
        assert all(type(layer[n]).__name__ == "_Linear" and layer[n].packed is None for layer in fused.layers for n in ("qkv", "fc1", "fc2"))

    for other in (None, "float8_e4m3"):
        refused(f"smoothing=.*linear_dtype='int8' only.*got linear_dtype={other!r}", scales, linear_dtype=other)
    refused("smoothing=.*linear_dtype='int8' only", scales, dtype=torch.float32, linear_dtype="bfloat16x3")
    refused("smoothing=.*linear_dtype='int8' only", scales, residual_dtype="float32")
    refused("bfloat16 carrier only", scales, dtype=torch.float16, linear_dtype=INT8)  # the unsmoothed option's refusals come as they were
    refused("no scales for `blocks.1.mlp.fc2`", {k: v for k, v in scales.items() if k != "blocks.1.mlp.fc2"}, linear_dtype=INT8)
    refused(r"smoothing\['blocks.0.attn.qkv'\].*\[128\]; got \(127,\)", {**scales, "blocks.0.attn.qkv": torch.ones(127)}, linear_dtype=INT8)
    refused(r"smoothing\['blocks.0.attn.qkv'\].*\[128\]; got \(128,\), torch.int64", {**scales, "blocks.0.attn.qkv": torch.ones(128, dtype=torch.long)},
            linear_dtype=INT8)
    for bad in (0.0, -2.0, float("inf"), float("nan"), 0.75):
        wrong = {k: v.clone() for k, v in scales.items()}
        wrong["blocks.0.mlp.fc2"][3] = bad
        refused(r"smoothing\['blocks.0.mlp.fc2'\].*finite positive powers of two.*channel 3", wrong, linear_dtype=INT8)
    refused("smoothing is a dict", [1.0], linear_dtype=INT8)
    # a key of a layer that stays on the half kernel is ignored with one info line: mlp_dim 576 keeps fc2 (K = 576) off the INT8 GEMM
    vit576 = tiny_vit(mlp_dim=576)
    sc = {**_pow2_scales(vit576), "blocks.0.mlp.fc2": torch.ones(576), "blocks.1.mlp.fc2": torch.ones(576)}
    with caplog.at_level(logging.INFO, logger="tiatoolbox_amd"):
        fused = _graph(vit576, sc)
    said = [r.getMessage() for r in caplog.records if "ignored" in r.getMessage()]
    assert len(said) == 1 and "blocks.0.mlp.fc2, blocks.1.mlp.fc2" in said[0] and "neither smoothed nor quantised" in said[0], said
    assert set(fused.smoothing) == {f"blocks.{i}.{n}" for i in range(2) for n in ("attn.qkv", "mlp.fc1")}
    assert all(type(layer["fc2"]).__name__ == "_Linear" for layer in fused.layers)


def _patches(n: int = 2) -> np.ndarray:
    return np.random.default_rng(0).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def _tiny_backbone():
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone("vit_small_patch16_224")
    model.feat_extract = tiny_vit(img_size=224, dynamic=False)
    return model


def _reset(eng) -> bool:
    return eng.compute_dtype == "float32" and eng.int8_smoothing is None and eng.int8_calibration is None and eng.residual_dtype is None


@pytest.mark.parametrize("kind", ["DeepFeatureExtractor", "PatchPredictor"])
def test_engines_refuse_each_combination_and_leave_nothing_behind(kind, monkeypatch):
    from _vit_classifier_ref import timm_model

    from tiatoolbox_amd import models

    model = _tiny_backbone() if kind == "DeepFeatureExtractor" else timm_model(img_size=224, dynamic=False)
    eng = getattr(models, kind)(model, batch_size=2)  # device="cpu"
    assert _reset(eng) and eng.int8_smoothing_scales is None
    run = functools.partial(eng.run, _patches(), patch_mode=True, ioconfig=_cfg())
    # without compute_dtype="int8" (any other value), with either new kwarg
    for kw in ({"int8_smoothing": 0.5}, {"int8_calibration": _patches()}, {"int8_smoothing": 0.5, "int8_calibration": _patches()},
               {"int8_smoothing": 0.5, "int8_calibration": _patches(), "compute_dtype": "bfloat16"}):
        with pytest.raises(ValueError, match="int8_smoothing=alpha.*compute_dtype=\"int8\" run.*got int8_smoothing=.*with compute_dtype="):
            run(**kw)
        assert _reset(eng)
    # on the CPU compute_dtype="int8" itself is refused first, with its own text -- and the new values do not stay either
    with pytest.raises(ValueError, match="compute_dtype=\"int8\" covers Vision Transformer.*CUDA"):
        run(compute_dtype=INT8, int8_smoothing=0.5, int8_calibration=_patches())
    assert _reset(eng)
    # the rest is decided before any device work: a CUDA device in name only
    monkeypatch.setattr(eng, "device", "cuda")

    def refused(match, **kw):
        eng.compute_dtype, eng.residual_dtype = INT8, None
        eng.int8_smoothing, eng.int8_calibration = kw.get("int8_smoothing"), kw.get("int8_calibration")
        with pytest.raises(ValueError, match=match):
            eng._inference_model(BF16)  # noqa: SLF001
        assert _reset(eng)

    refused("int8_smoothing=alpha.*got int8_smoothing=0.5 without int8_calibration", int8_smoothing=0.5)
    refused("int8_smoothing=alpha.*got int8_calibration without int8_smoothing", int8_calibration=_patches())
    for alpha in (0.0, 1.5, -1.0, "half", True):
        refused(f"int8_smoothing=alpha.*got int8_smoothing={alpha!r}", int8_smoothing=alpha, int8_calibration=_patches())
    refused("int8_smoothing=alpha.*got int8_calibration of type list", int8_smoothing=0.5, int8_calibration=[1, 2])
    refused("int8_smoothing=alpha.*got int8_calibration of type ndarray, shape \\(224, 224, 3\\)", int8_smoothing=0.5, int8_calibration=_patches()[0])
    assert eng.run(_patches(), patch_mode=True, ioconfig=_cfg(), device="cpu") is not None  # the engine is usable afterwards


def test_the_cache_key_carries_alpha_and_the_identity_of_the_scales(monkeypatch):
    """As ``test_vit_int8.test_the_cache_key_carries_the_option``: with the key of one smoothed copy in place, the same alpha and
    scales dict return the cached model; another alpha, another dict or no smoothing start a new copy.  Without the kwargs the key is
    the eight-element one it was."""
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.engine.engine_abc import _weights_version

    eng = DeepFeatureExtractor(_tiny_backbone(), batch_size=2)

    class CopyStartedError(Exception):
        pass

    def deepcopy(_model):
        raise CopyStartedError

    monkeypatch.setattr(copy, "deepcopy", deepcopy)
    monkeypatch.setattr(eng, "device", "cuda")
    cached, scales, other = object(), {"blocks.0.attn.qkv": torch.ones(128)}, {"blocks.0.attn.qkv": torch.ones(128)}
    base = (BF16, "cuda", id(eng.model), eng.fold_batchnorm, _weights_version(eng.model), "winograd", INT8, None)

    def run(key, alpha, calib):
        eng.compute_dtype, eng.residual_dtype, eng.int8_smoothing, eng.int8_calibration = INT8, None, alpha, calib
        eng._fast_model, eng._fast_key = cached, key  # noqa: SLF001
        return eng._inference_model(BF16)  # noqa: SLF001

    assert run(base, None, None) is cached
    assert run((*base, 0.5, id(scales)), 0.5, scales) is cached and eng.int8_smoothing_scales is scales
    for key, alpha, calib in (((*base, 0.5, id(scales)), 0.25, scales), ((*base, 0.5, id(scales)), 0.5, other), (base, 0.5, scales),
                              ((*base, 0.5, id(scales)), None, None)):
        with pytest.raises(CopyStartedError):
            run(key, alpha, calib)


# --------------------------------------------------------------------------------------------------------------- the round trip
def test_a_saved_calibration_prepares_the_same_codes(stand_ins, tmp_path):
    vit, x, scales = _scenario_b()
    torch.save(scales, tmp_path / "scales.pt")
    loaded = torch.load(tmp_path / "scales.pt")
    assert set(loaded) == set(scales) and all(torch.equal(loaded[k], scales[k]) and loaded[k].dtype == torch.float32 for k in scales)
    first, second = _graph(vit, scales), _graph(vit, loaded)
    for a, b in zip(first.layers, second.layers):
        for name in ("qkv", "fc1", "fc2"):
            assert torch.equal(a[name].packed.codes, b[name].packed.codes) and torch.equal(a[name].packed.scales, b[name].packed.scales)
        assert torch.equal(a["norm1"][0], b["norm1"][0]) and torch.equal(a["fc2"].inv_smooth, b["fc2"].inv_smooth)
    with torch.inference_mode():
        assert torch.equal(first(x.to(BF16)), second(x.to(BF16)))


def test_the_calibration_case_has_few_columns_near_a_rounding_tie():
    """The GPU calibration test allows one binade on columns within 1e-3 of a tie and caps their number at 1 % of all columns: on
    the torch reference the chosen seeds stay under that cap."""
    from _vit_int8_smooth_ref import calibration_case, near_tie_columns

    vit, batches = calibration_case()
    _, amax_x, amax_w = reference_calibration(vit, batches, 0.5)
    near = sum(int(near_tie_columns(amax_x[k], amax_w[k], 0.5).sum()) for k in amax_x)
    total = sum(v.numel() for v in amax_x.values())
    print(f"{near} of {total} columns within 1e-3 of a rounding tie")
    assert total == 2 * (128 + 128 + 512) and near <= total // 100

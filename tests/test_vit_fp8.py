"""``compute_dtype="float8_e4m3"`` without a GPU: the quantisation recipe against known answers, and what the option refuses."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _vit_ref import tiny_vit


def _codes(q: torch.Tensor) -> list[int]:
    return q.view(torch.uint8).reshape(-1).tolist()


def test_recipe_rounds_ties_to_even_and_saturates():
    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_e4m3

    # amax = 448 makes inv = s = 1: the codes are the conversion of the values themselves.  Between 16 and 32 the step is 2: 17 is the
    # tie between 16 (mantissa 000, even) and 18 (001), 19 between 18 and 20 (010); 21 -> 20, 23 -> 24; 27 and 29 -> 28 either way
    row = torch.tensor([[448.0, 17.0, 19.0, 21.0, 23.0, -17.0, -19.0, 18.5, 0.0]])
    q, s = quantize_rows_e4m3(row)
    assert s.tolist() == [1.0] and q.dtype == torch.float8_e4m3fn
    assert q.float().tolist() == [[448.0, 16.0, 20.0, 20.0, 24.0, -16.0, -20.0, 18.0, 0.0]]
    assert _codes(q)[0] == 0x7E  # 448 = 1.75 * 2^8, the largest finite code  # noqa: PLR2004
    # the conversion saturates: 460 (below the tie to the absent 480) -> 448, as torch's CPU conversion does; the recipe's clamp keeps
    # that beyond 464 as well, where the bare conversion makes a NaN
    assert torch.tensor([460.0, -460.0]).to(torch.float8_e4m3fn).float().tolist() == [448.0, -448.0]
    assert torch.tensor([1e6, -3e38]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float().tolist() == [448.0, -448.0]


def test_recipe_scales_by_the_row_maximum():
    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_e4m3

    # amax = 896 -> s = 2, inv = 0.5 (both exact): 34 -> 17 -> 16 (tie to even) -> dequantised 32; the row maximum is code 0x7e
    q, s = quantize_rows_e4m3(torch.tensor([[-896.0, 34.0, 38.0, 2.0], [3.5, 0.0, -0.875, 1.75]]))
    assert s.tolist() == [2.0, 3.5 / 448.0]
    assert (q[0].float() * s[0]).tolist() == [-896.0, 32.0, 40.0, 2.0]
    assert _codes(q[0])[0] == 0xFE and _codes(q[1])[0] == 0x7E  # noqa: PLR2004
    assert q[1].float().tolist() == [448.0, 0.0, -112.0, 224.0]  # 3.5 * (448 / 3.5) etc.: exact powers of two apart
    # float32 divisions, as stated: the scale of amax = 3 is fl(3 / 448), and the codes come from v * fl(448 / 3)
    q, s = quantize_rows_e4m3(torch.tensor([[3.0, 1.0]]))
    assert s.item() == (np.float32(3.0) / np.float32(448.0)).item()
    inv = np.float32(448.0) / np.float32(3.0)
    assert q.float().tolist() == [[448.0, torch.tensor(float(np.float32(1.0) * inv)).to(torch.float8_e4m3fn).float().item()]]


def test_recipe_subnormal_step_and_zero_row():
    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_e4m3

    # below 2^-6 the codes step by 2^-9: with inv = 1, 2^-9 is code 1, 2^-10 is the tie between codes 0 and 1 (-> 0, even),
    # 3 * 2^-10 the tie between 1 and 2 (-> 2), 7.5 * 2^-9 the tie between 7 and 8 (-> 8 = 2^-6, the smallest normal)
    row = torch.tensor([[448.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 7.5 * 2.0 ** -9, -(2.0 ** -9), 2.0 ** -11, 1.2 * 2.0 ** -10]])
    q, s = quantize_rows_e4m3(row)
    assert s.item() == 1.0
    assert _codes(q)[1:] == [1, 0, 2, 8, 0x81, 0, 1]
    # an all-zero row keeps scale 1 and zero codes; a leading batch axis is kept
    q, s = quantize_rows_e4m3(torch.zeros((2, 3, 8)))
    assert s.shape == (2, 3) and bool((s == 1.0).all()) and _codes(q) == [0] * 48


def test_recipe_matches_the_value_table_of_the_helper():
    from _vit_fp8_ref import E4M3_VALUES, FINITE_CODES, decode, encode_exact, ulp_e4m3

    vals = decode(FINITE_CODES)
    assert float(vals.abs().max()) == 448.0 and float(vals[vals > 0].min()) == 2.0 ** -9  # noqa: PLR2004
    assert torch.equal(encode_exact(vals), FINITE_CODES)
    assert bool(torch.isnan(E4M3_VALUES[0x7F])) and bool(torch.isnan(E4M3_VALUES[0xFF]))
    pos = vals[(vals > 0)].sort().values
    assert torch.equal(ulp_e4m3(pos[:-1]), pos[1:] - pos[:-1])  # the spacing above every positive code


def test_tie_rows_hold_every_midpoint_and_the_recipe_rounds_them_to_even():
    """The rows the device's packing kernel is held to (``test_pack_weights_rounds_every_tie_as_the_recipe``): every row's scale is 1,
    every midpoint of two adjacent magnitudes goes to the one with the even code, its neighbours to the nearer magnitude, in both
    signs -- worked out here from the code table, not from the conversion."""
    from _vit_fp8_ref import FINITE_CODES, decode, e4m3_tie_rows

    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_e4m3

    rows = e4m3_tie_rows(16)
    q, s = quantize_rows_e4m3(rows)
    assert rows.shape == (16, 768) and bool((s == 1.0).all()) and bool((rows[:, 0] == 448.0).all())  # noqa: PLR2004
    assert all(torch.equal(rows[r, 1:].sort().values, rows[0, 1:].sort().values) for r in range(16))  # rotations of one another
    mags = decode(FINITE_CODES[:127])
    lo, hi = torch.arange(126), torch.arange(1, 127)
    even = torch.where(lo % 2 == 0, lo, hi)
    want = torch.stack([lo, even, hi], dim=1).reshape(-1).to(torch.uint8)  # below the midpoint, on it, above it
    codes = q.view(torch.uint8)[0]
    assert int(codes[0]) == 0x7E and torch.equal(codes[1:379], want) and torch.equal(codes[379:757], want | 0x80)  # noqa: PLR2004
    assert torch.equal(rows[0, 2:379:3].double(), (mags[:-1] + mags[1:]) / 2) and bool((codes[757:] == 0).all())


def _patches(n: int = 2) -> np.ndarray:
    return np.random.default_rng(0).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def test_engine_refuses_fp8_on_the_cpu():
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone("vit_small_patch16_224")
    model.feat_extract = tiny_vit(img_size=224, dynamic=False)
    eng = DeepFeatureExtractor(model, batch_size=2)  # device="cpu"
    with pytest.raises(ValueError, match="float8_e4m3.*Vision Transformer.*CUDA"):
        eng.run(_patches(), patch_mode=True, ioconfig=_cfg(), compute_dtype="float8_e4m3")
    assert eng.compute_dtype == "float32"  # the refused value is not left behind for the next run
    assert eng.run(_patches(), patch_mode=True, ioconfig=_cfg())["probabilities"].shape == (2, 128)


def test_engine_refuses_fp8_for_a_cnn():
    from tiatoolbox_amd.models import PatchPredictor

    eng = PatchPredictor("resnet18-kather100k", batch_size=2)
    with pytest.raises(ValueError, match="float8_e4m3.*Vision Transformer"):
        eng.run(_patches(), patch_mode=True, compute_dtype="float8_e4m3")


def test_fp8_is_an_option_of_the_graph_not_a_parameter_dtype():
    """The carrier of ``"float8_e4m3"`` is bfloat16 (what the model copy is cast to); no other name changes its meaning."""
    from tiatoolbox_amd.models.engine import engine_abc

    assert engine_abc._carrier_dtype("float8_e4m3") == torch.bfloat16 and engine_abc._carrier_dtype("bfloat16") == torch.bfloat16  # noqa: SLF001
    assert engine_abc._carrier_dtype(torch.float16) == torch.float16 and engine_abc._carrier_dtype("float32") == torch.float32  # noqa: SLF001
    with pytest.raises(KeyError):
        engine_abc._carrier_dtype("float8_e5m2")  # noqa: SLF001


def test_prepare_refuses_fp8_on_an_fp16_carrier_and_unknown_names():
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    with pytest.raises(ValueError, match="bfloat16 carrier"):
        FusedViT(tiny_vit()).prepare(torch.float16, linear_dtype="float8_e4m3")
    with pytest.raises(ValueError, match="linear_dtype"):
        FusedViT(tiny_vit()).prepare(torch.bfloat16, linear_dtype="float8_e5m2")
    with pytest.raises(ValueError, match="float16 or bfloat16"):  # the pinned refusals come first, with or without the argument
        FusedViT(tiny_vit()).prepare(torch.float32, linear_dtype="float8_e4m3")


@pytest.fixture
def torch_wrappers(monkeypatch):
    from _vit_classifier_ref import torch_vit_wrappers

    from tiatoolbox_amd.models.architecture import vit_fused

    calls: dict = {}
    for name, fn in torch_vit_wrappers(calls).items():
        monkeypatch.setattr(vit_fused, name, fn)
    return calls


def test_prepare_without_the_argument_keeps_the_half_path(torch_wrappers, monkeypatch):
    """On torch stand-ins of the half wrappers (any device): ``prepare(torch.bfloat16)`` makes no FP8 layer and the forward calls none of
    the FP8 wrappers -- they are replaced by functions that fail."""
    from tiatoolbox_amd.models.architecture import vit_fused

    def fail(*_a, **_k):
        raise AssertionError("an FP8 wrapper was called on the half path")

    for name in ("pack_linear_weights_fp8", "hip_linear_fp8_rows", "hip_layernorm_rows_q8", "hip_act_rows_q8", "linear_fp8_serves"):
        monkeypatch.setattr(vit_fused, name, fail)
    vit = tiny_vit()
    fused = vit_fused.FusedViT(vit)
    fused.prepare(torch.bfloat16)
    assert fused.linear_dtype is None and fused.half_dtype == torch.bfloat16
    assert all(type(layer[name]).__name__ == "_Linear" for layer in fused.layers for name in ("qkv", "proj", "fc1", "fc2"))
    x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(0))
    with torch.inference_mode():
        got, ref = fused(x), vit(x)
    assert got.dtype == torch.float32 and float((got - ref).abs().max()) <= 0.1 * max(float(ref.abs().max()), 1.0)  # (bf16: sanity)

"""``compute_dtype="int8"`` without a GPU: the symbols, the quantisation recipe against known answers, what the option refuses, the
cache key, and the wiring of the graph on torch stand-ins of its wrappers against the yardstick, with faults that each must fail."""

from __future__ import annotations

import copy
import ctypes
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

from _vit_int8_ref import fake_quantised_module, rel_error, torch_int8_wrappers
from _vit_ref import tiny_vit
from _vit_virchow_ref import TINY_V2, tiny_virchow

INT8 = "int8"
BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------- the symbols
def test_symbols_and_signatures():
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture import vit_fused
    from tiatoolbox_amd.models.engine import engine_abc

    assert vit_fused.INT8_LINEAR == INT8 and engine_abc.INT8_COMPUTE == INT8
    for name in ("quantize_rows_int8", "pack_linear_weights_int8", "hip_linear_int8_rows", "hip_layernorm_rows_qi8", "hip_act_rows_qi8",
                 "linear_int8_serves", "_LinearInt8"):
        assert hasattr(vit_fused, name), name
    assert hasattr(vit_fused.FusedViT, "_route_int8")
    assert list(inspect.signature(vit_fused.hip_linear_int8_rows).parameters) == ["a", "w", "bias", "residual", "dtype"]
    assert list(inspect.signature(vit_fused.hip_layernorm_rows_qi8).parameters) == ["x", "gamma", "beta", "eps"]
    assert list(inspect.signature(vit_fused.hip_act_rows_qi8).parameters) == ["x", "swiglu"]
    sig = _lib._SIGNATURES  # noqa: SLF001
    lib = _lib.load()
    for fp8, int8 in (("tia_linear_fp8_rows", "tia_linear_int8_rows"), ("tia_linear_fp8_pack_weights", "tia_linear_int8_pack_weights"),
                      ("tia_linear_fp8_serves", "tia_linear_int8_serves"), ("tia_layernorm_rows_q8", "tia_layernorm_rows_qi8"),
                      ("tia_gelu_rows_q8", "tia_gelu_rows_qi8"), ("tia_swiglu_rows_q8", "tia_swiglu_rows_qi8")):
        a, b = getattr(lib, fp8), getattr(lib, int8)
        assert b.argtypes == a.argtypes and b.restype is ctypes.c_int, int8  # the FP8 entry's argument list
        assert sig[int8] == sig[fp8]
    assert lib.tia_abi_version() == 6  # additive  # noqa: PLR2004
    # the host-only routing answer needs no device
    assert lib.tia_linear_int8_serves(1, 16, 128) == 1 and lib.tia_linear_int8_serves(1, 16, 65536) == 1
    assert lib.tia_linear_int8_serves(1, 16, 65536 + 128) == 0 and lib.tia_linear_int8_serves(1, 16, 96) == 0
    assert lib.tia_linear_int8_serves(1, 24, 128) == 0 and lib.tia_linear_int8_serves(0, 16, 128) == -1
    header = (Path(__file__).resolve().parents[1] / "include" / "tiatoolbox_amd.h").read_text()
    for name in ("tia_linear_int8_rows", "tia_linear_int8_pack_weights", "tia_linear_int8_serves", "tia_layernorm_rows_qi8",
                 "tia_gelu_rows_qi8", "tia_swiglu_rows_qi8"):
        assert f"int {name}(" in header, name


# -------------------------------------------------------------------------------------------------------------------- the recipe
def test_recipe_rounds_ties_to_even_and_maps_the_maximum_to_127():
    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_int8

    # amax = 127 makes inv = s = 1: the codes are the rounded values themselves.  0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4 (ties to even)
    row = torch.tensor([[127.0, 0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 126.5, -126.5, 125.5, 0.49999997, 0.0]])
    q, s = quantize_rows_int8(row)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and s.tolist() == [1.0]
    assert q.tolist() == [[127, 0, 2, 2, 4, 0, -2, -2, 126, -126, 126, 0, 0]]
    # the row maximum maps to +-127 exactly, whatever it is; amax = 254 -> s = 2, inv = 0.5 (both exact): 3 -> 1.5 -> 2, 5 -> 2.5 -> 2
    q, s = quantize_rows_int8(torch.tensor([[-254.0, 3.0, 5.0, 1.0], [0.3, 0.0, -0.15, 0.075]]))
    assert s.tolist() == [2.0, (np.float32(0.3) / np.float32(127.0)).item()]
    assert q.tolist()[0] == [-127, 2, 2, 0] and q.tolist()[1][0] == 127  # noqa: PLR2004
    g = torch.Generator().manual_seed(0)
    v = torch.randn((64, 384), generator=g) * torch.exp2(torch.randint(-20, 20, (64, 1), generator=g).float())
    q, s = quantize_rows_int8(v)
    assert bool((q.abs().amax(dim=1) == 127).all()) and int(q.min()) >= -127  # noqa: PLR2004
    idx = v.abs().argmax(dim=1)
    assert torch.equal(q[torch.arange(64), idx].float(), torch.sign(v[torch.arange(64), idx]) * 127)
    # float32 divisions, as stated: the scale of amax = 3 is fl(3 / 127), and the codes come from v * fl(127 / 3)
    q, s = quantize_rows_int8(torch.tensor([[3.0, 1.0, -2.0]]))
    inv = np.float32(127.0) / np.float32(3.0)
    assert s.item() == (np.float32(3.0) / np.float32(127.0)).item()
    assert q.tolist() == [[127, int(np.rint(np.float32(1.0) * inv)), int(np.rint(np.float32(-2.0) * inv))]]


def test_recipe_never_makes_minus_128_and_keeps_a_zero_row():
    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_int8

    # every row whose maximum is negative: the code is -127, never -128, also where fl(v * fl(127 / amax)) lands above 127
    mags = torch.cat([torch.arange(1, 4097).float() / 7.0, torch.exp2(torch.arange(-126.0, 127.0)), torch.tensor([3.4e38, 1.2e-38])])
    q, s = quantize_rows_int8(torch.stack([-mags, mags * 0.999999, mags * 0.5], dim=1))
    assert int(q.min()) == -127 and int(q.max()) == 127 and bool((q[:, 0] == -127).all())  # noqa: PLR2004
    assert bool(torch.isfinite(s).all())
    # an all-zero row keeps scale 1 and zero codes; a leading batch axis is kept
    q, s = quantize_rows_int8(torch.zeros((2, 3, 8)))
    assert s.shape == (2, 3) and bool((s == 1.0).all()) and q.shape == (2, 3, 8) and not bool(q.any())


def test_recipe_gives_non_finite_rows_a_non_finite_scale():
    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_int8

    nan, inf = float("nan"), float("inf")
    v = torch.tensor([[1.0, -2.0, 0.5, 4.0], [1.0, nan, 0.5, 4.0], [1.0, -inf, 0.5, 4.0], [inf, nan, 0.0, 1.0], [4.0, 2.0, -1.0, 0.0]])
    q, s = quantize_rows_int8(v)
    assert bool(torch.isnan(s[1])) and float(s[2]) == inf and bool(torch.isnan(s[3]))  # the maximum propagates the NaN
    assert bool(torch.isfinite(s[[0, 4]]).all()) and q[0].tolist() == [32, -64, 16, 127] and q[4].tolist() == [127, 64, -32, 0]
    assert int(q.min()) >= -127 and int(q.max()) <= 127  # noqa: PLR2004
    assert q[1].tolist() == [0, 0, 0, 0] and q[2].tolist() == [0, 0, 0, 0]  # NaN products (inf * 0 among them) are code 0
    # every output of such a token is non-finite under the GEMM's formula, whatever the accumulator: acc * s is NaN or +-inf
    for sc in (s[1], s[2]):
        for acc in (0.0, 5.0, -7.0):
            assert not bool(torch.isfinite(torch.tensor(acc) * sc * 0.25 + 1.0))


# ----------------------------------------------------------------------------------------------------------------- the refusals
def test_prepare_refuses_each_combination_with_a_message_of_its_own():
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    said = []
    for dtype, kw in ((torch.float16, {}), (BF16, {"residual_dtype": "float32"}), (torch.float32, {})):
        fused = FusedViT(tiny_vit())
        with pytest.raises(ValueError, match="int8") as info:
            fused.prepare(dtype, linear_dtype=INT8, **kw)
        said.append(str(info.value))
        assert fused.half_dtype is None and fused.linear_dtype is None  # refused before any device work: nothing is packed
        assert all(type(layer[n]).__name__ == "_Linear" and layer[n].packed is None for layer in fused.layers for n in ("qkv", "fc1", "fc2"))
    assert len(set(said)) == 3  # noqa: PLR2004
    assert "bfloat16 carrier" in said[0] and "residual" in said[1] and "float32" in said[2] and "carrier" in said[2]
    # the existing refusals keep their text
    with pytest.raises(ValueError, match="bfloat16 carrier only \\(there is no fp16 form\\)"):
        FusedViT(tiny_vit()).prepare(torch.float16, linear_dtype="float8_e4m3")
    with pytest.raises(ValueError, match="linear_dtype is None or 'float8_e4m3'"):
        FusedViT(tiny_vit()).prepare(BF16, linear_dtype="float8_e5m2")
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        FusedViT(tiny_vit()).prepare(torch.float32, linear_dtype="float8_e4m3")
    with pytest.raises(ValueError, match="tia_layernorm_rows_q8 that reads the float32 stream"):
        FusedViT(tiny_vit()).prepare(BF16, linear_dtype="float8_e4m3", residual_dtype="float32")


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


def test_feature_extractor_refuses_int8_on_the_cpu():
    from tiatoolbox_amd.models import DeepFeatureExtractor

    eng = DeepFeatureExtractor(_tiny_backbone(), batch_size=2)  # device="cpu"
    with pytest.raises(ValueError, match="int8.*Vision Transformer.*CUDA"):
        eng.run(_patches(), patch_mode=True, ioconfig=_cfg(), compute_dtype=INT8)
    assert eng.compute_dtype == "float32" and eng.residual_dtype is None  # the refused value is not left behind for the next run
    with pytest.raises(ValueError, match="int8.*Vision Transformer.*residual_dtype"):
        eng.run(_patches(), patch_mode=True, ioconfig=_cfg(), compute_dtype=INT8, residual_dtype="float32")
    assert eng.compute_dtype == "float32" and eng.residual_dtype is None
    assert eng.run(_patches(), patch_mode=True, ioconfig=_cfg())["probabilities"].shape == (2, 128)


def test_patch_predictor_refuses_int8_for_a_cnn_and_on_the_cpu():
    from _vit_classifier_ref import timm_model

    from tiatoolbox_amd.models import PatchPredictor

    eng = PatchPredictor("resnet18-kather100k", batch_size=2)
    with pytest.raises(ValueError, match="int8.*Vision Transformer"):
        eng.run(_patches(), patch_mode=True, compute_dtype=INT8)
    assert eng.compute_dtype == "float32" and eng.residual_dtype is None
    assert eng.run(_patches(), patch_mode=True)["predictions"].shape == (2,)
    vit = PatchPredictor(timm_model(img_size=224, dynamic=False), batch_size=2)
    with pytest.raises(ValueError, match="int8.*Vision Transformer.*CUDA"):
        vit.run(_patches(), patch_mode=True, ioconfig=_cfg(), compute_dtype=INT8)
    assert vit.compute_dtype == "float32" and vit.residual_dtype is None
    assert vit.run(_patches(), patch_mode=True, ioconfig=_cfg())["predictions"].shape == (2,)


@pytest.mark.parametrize("kind", ["unet", "hovernet"])
def test_the_option_refuses_segmentation_models(kind):
    """``_inference_model`` is the one place every engine's model copy is made: a UNet or HoVer-Net in it is refused like a CNN."""
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.models.architecture.hovernet import HoVerNet
    from tiatoolbox_amd.models.architecture.unet import UNetModel

    eng = PatchPredictor("resnet18-kather100k", batch_size=2)
    with torch.device("meta"):
        eng.model = UNetModel(3, 2) if kind == "unet" else HoVerNet(num_types=None, mode="fast")
    eng.compute_dtype, eng.residual_dtype = INT8, None
    with pytest.raises(ValueError, match="int8.*Vision Transformer.*(UNetModel|HoVerNet)"):
        eng._inference_model(BF16)  # noqa: SLF001
    assert eng.compute_dtype == "float32" and eng.residual_dtype is None


def test_int8_is_an_option_of_the_graph_with_a_bfloat16_carrier():
    from tiatoolbox_amd.models.engine import engine_abc

    assert engine_abc._carrier_dtype(INT8) == BF16 and engine_abc._carrier_dtype("float8_e4m3") == BF16  # noqa: SLF001
    assert engine_abc._carrier_dtype("bfloat16x3") == torch.float32 and engine_abc._carrier_dtype(torch.float16) == torch.float16  # noqa: SLF001
    with pytest.raises(KeyError):
        engine_abc._carrier_dtype("float8_e5m2")  # noqa: SLF001
    with pytest.raises(KeyError):
        engine_abc._carrier_dtype("int4")  # noqa: SLF001


def test_the_cache_key_carries_the_option(monkeypatch):
    """The inference copy is cached under a key.  ``"int8"``, ``"float8_e4m3"`` and ``"bfloat16"`` share one carrier and must be three
    keys: with the cached key of one option in place, a run under another starts a new copy (``copy.deepcopy`` is where it starts --
    it is replaced by a function that raises, and nothing reaches a device), and a run under the same one returns the cached model."""
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.engine.engine_abc import _weights_version

    eng = DeepFeatureExtractor(_tiny_backbone(), batch_size=2)

    class CopyStartedError(Exception):
        pass

    def deepcopy(_model):
        raise CopyStartedError

    monkeypatch.setattr(copy, "deepcopy", deepcopy)
    monkeypatch.setattr(eng, "device", "cuda")
    cached = object()

    def key(option):
        return (BF16, "cuda", id(eng.model), eng.fold_batchnorm, _weights_version(eng.model), "winograd", option, None)

    def run(name, option):
        eng.compute_dtype, eng.residual_dtype = name, None
        eng._fast_model, eng._fast_key = cached, key(option)  # noqa: SLF001
        return eng._inference_model(BF16)  # noqa: SLF001

    assert run(INT8, INT8) is cached  # the option is an element of the key
    assert run("float8_e4m3", True) is cached and run("bfloat16", False) is cached  # the other two keys are what they were
    for name, option in ((INT8, True), (INT8, False), ("float8_e4m3", INT8), ("bfloat16", INT8)):
        with pytest.raises(CopyStartedError):
            run(name, option)


# --------------------------------------------------------------------------------------------------------------------- the wiring
@pytest.fixture
def stand_ins(monkeypatch):
    """``vit_fused`` with every wrapper ``FusedViT`` calls replaced by its torch restatement: the half ones of
    ``_vit_classifier_ref`` and the INT8 ones of ``_vit_int8_ref``."""
    from _vit_classifier_ref import torch_vit_wrappers

    from tiatoolbox_amd.models.architecture import vit_fused

    table = {**torch_vit_wrappers({}), **torch_int8_wrappers()}
    real = vit_fused.hip_linear_int8_rows
    for name, fn in table.items():
        monkeypatch.setattr(vit_fused, name, fn)
    return {**table, "the real hip_linear_int8_rows": real}


def _errors(vit, x, layers=("qkv", "fc1", "fc2")) -> tuple[float, float, object]:
    """``(e_graph, e_yardstick, graph)`` against the float32 module: the INT8 graph on the stand-ins, and the bfloat16 torch module
    with the ``layers`` the graph routes fake-quantised."""
    from tiatoolbox_amd.models.architecture import vit_fused

    with torch.inference_mode():
        ref = vit(x)
        yard = fake_quantised_module(copy.deepcopy(vit), layers=layers)(x.to(BF16)).float()
        fused = vit_fused.FusedViT(copy.deepcopy(vit))
        fused.prepare(BF16, linear_dtype=INT8)
        got = fused.to(BF16)(x.to(BF16))
    assert got.shape == ref.shape and got.dtype == torch.float32
    return rel_error(got, ref), rel_error(yard, ref), fused


def _tiny_case():
    return tiny_vit(), torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(0))


def _virchow_case():
    # D = 320: qkv and fc1 are off K % 128 and stay half; H = 520 -> 544 -> 640 puts 96 + 24 pad lanes in front of the INT8 fc2
    return tiny_virchow(TINY_V2), torch.randn((2, 3, 28, 28), generator=torch.Generator().manual_seed(1))


def test_wiring_matches_the_yardstick(stand_ins):
    e_new, e_yard, fused = _errors(*_tiny_case())
    print(f"tiny: e_int8_graph {e_new:.3e}  e_yardstick {e_yard:.3e}")
    assert fused.linear_dtype == INT8 and fused.half_dtype == BF16
    kinds = {name: {type(layer[name]).__name__ for layer in fused.layers} for name in ("qkv", "proj", "fc1", "fc2")}
    assert kinds == {"qkv": {"_LinearInt8"}, "proj": {"_Linear"}, "fc1": {"_LinearInt8"}, "fc2": {"_LinearInt8"}}
    assert all(layer[n].packed.codes.dtype == torch.int8 and layer[n].weight32 is None for layer in fused.layers for n in ("qkv", "fc1", "fc2"))
    assert e_new <= 2.0 * e_yard
    e_new, e_yard, fused = _errors(*_virchow_case(), layers=("fc2",))
    print(f"token_mean, SwiGLU padded: e_int8_graph {e_new:.3e}  e_yardstick {e_yard:.3e}")
    kinds = {name: {type(layer[name]).__name__ for layer in fused.layers} for name in ("qkv", "proj", "fc1", "fc2")}
    assert kinds == {"qkv": {"_Linear"}, "proj": {"_Linear"}, "fc1": {"_Linear"}, "fc2": {"_LinearInt8"}}
    assert fused.layers[0]["fc2"].cin == 640 and not bool(fused.layers[0]["fc2"].packed.codes[:, 520:].any())  # noqa: PLR2004
    assert e_new <= 2.0 * e_yard


def _fault_fails(case=_tiny_case, layers=("qkv", "fc1", "fc2")) -> None:
    e_new, e_yard, _ = _errors(*case(), layers=layers)
    print(f"with the fault: e_int8_graph {e_new:.3e}  e_yardstick {e_yard:.3e}")
    assert e_new > 2.0 * e_yard


def test_fault_a_wrong_producer_in_front_of_fc2(stand_ins, monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    layernorm = stand_ins["hip_layernorm_rows_qi8"]
    monkeypatch.setattr(vit_fused, "hip_act_rows_qi8",  # quantises fc1's output without the GELU
                        lambda x, *, swiglu: layernorm(x, torch.ones(x.shape[-1]), torch.zeros(x.shape[-1]), eps=1e-6))  # noqa: ARG005
    _fault_fails()


def test_fault_a_dropped_residual(stand_ins, monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    linear = stand_ins["hip_linear_int8_rows"]
    monkeypatch.setattr(vit_fused, "hip_linear_int8_rows", lambda a, w, bias, residual=None, *, dtype: linear(a, w, bias, None, dtype=dtype))  # noqa: ARG005
    _fault_fails()


def test_fault_weights_quantised_per_input_channel(stand_ins, monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    def pack_columns(weight):  # one scale per INPUT channel decides the codes; the [cout] scales are the per-row ones
        q_col, _ = vit_fused.quantize_rows_int8(weight.detach().float().T.contiguous())
        _, s_row = vit_fused.quantize_rows_int8(weight.detach().float())
        return vit_fused.QuantRows(q_col.T.contiguous(), s_row)

    monkeypatch.setattr(vit_fused, "pack_linear_weights_int8", pack_columns)
    _fault_fails()


def test_fault_scales_swapped_between_tokens(stand_ins, monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    layernorm = stand_ins["hip_layernorm_rows_qi8"]

    def swapped(x, gamma, beta, *, eps):
        rows = layernorm(x, gamma, beta, eps=eps)
        return vit_fused.QuantRows(rows.codes, rows.scales.flip(0))

    monkeypatch.setattr(vit_fused, "hip_layernorm_rows_qi8", swapped)
    _fault_fails()


def test_fault_padding_lanes_not_zero(stand_ins, monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    pad_to = vit_fused.pad_swiglu_to

    def leaky(fc1_w, fc1_b, fc2_w, target):
        half = fc2_w.shape[1]
        w1, b1, w2 = pad_to(fc1_w, fc1_b, fc2_w, target)
        if target > half:  # a pad lane now computes silu(1) * 1 and meets a weight
            b1, w2 = b1.clone(), w2.clone()
            b1[half:target], b1[target + half:], w2[:, half:] = 1.0, 1.0, 0.05
        return w1, b1, w2

    monkeypatch.setattr(vit_fused, "pad_swiglu_to", leaky)
    _fault_fails(_virchow_case, layers=("fc2",))


def test_fault_an_int8_layer_fed_fp8_codes_is_refused(stand_ins, monkeypatch):
    """The two code formats travel as two tensor dtypes.  The wrappers themselves (their checks come before any device work): the
    INT8 GEMM's refuses the FP8 recipe's uint8 codes, on either operand, and the FP8 GEMM's refuses int8 codes.  And in the graph: an
    FP8 producer in front of an INT8 layer stops the forward at that layer."""
    from tiatoolbox_amd.models.architecture import vit_fused

    linear_int8, linear_fp8 = stand_ins["the real hip_linear_int8_rows"], vit_fused.hip_linear_fp8_rows
    rows8 = vit_fused.QuantRows(*vit_fused.quantize_rows_int8(torch.randn((1, 4, 128))))
    q, s = vit_fused.quantize_rows_e4m3(torch.randn((1, 4, 128)))
    fp8 = vit_fused.QuantRows(q.view(torch.uint8), s.reshape(-1))
    w8 = vit_fused.QuantRows(*vit_fused.quantize_rows_int8(torch.randn((16, 128))))
    wq, ws = vit_fused.quantize_rows_e4m3(torch.randn((16, 128)))
    wfp8 = vit_fused.QuantRows(wq.view(torch.uint8), ws)
    with pytest.raises(ValueError, match="torch.int8 codes.*got torch.uint8 beside torch.int8"):
        linear_int8(fp8, w8, None, dtype=BF16)
    with pytest.raises(ValueError, match="torch.int8 codes.*got torch.int8 beside torch.uint8"):
        linear_int8(rows8, wfp8, None, dtype=BF16)
    with pytest.raises(ValueError, match="hip_linear_fp8_rows takes uint8.*torch.int8"):
        linear_fp8(rows8, wfp8, None, dtype=BF16)

    def fp8_layernorm(x, gamma, beta, *, eps):
        q, s = vit_fused.quantize_rows_e4m3(torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), gamma, beta, eps))
        return vit_fused.QuantRows(q.view(torch.uint8), s.reshape(-1))

    monkeypatch.setattr(vit_fused, "hip_layernorm_rows_qi8", fp8_layernorm)
    monkeypatch.setattr(vit_fused, "hip_linear_int8_rows", linear_int8)  # the real wrapper: it must refuse before it reaches the library
    vit, x = _tiny_case()
    fused = vit_fused.FusedViT(vit)
    fused.prepare(BF16, linear_dtype=INT8)
    with torch.inference_mode(), pytest.raises(ValueError, match="torch.int8 codes.*got torch.uint8"):
        fused.to(BF16)(x.to(BF16))


def test_prepare_without_the_argument_makes_no_int8_layer(stand_ins, monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    def fail(*_a, **_k):
        raise AssertionError("an INT8 wrapper was called on the half path")

    for name in torch_int8_wrappers():
        monkeypatch.setattr(vit_fused, name, fail)
    fused = vit_fused.FusedViT(tiny_vit())
    fused.prepare(BF16)
    assert fused.linear_dtype is None and fused.half_dtype == BF16
    assert all(type(layer[name]).__name__ == "_Linear" for layer in fused.layers for name in ("qkv", "proj", "fc1", "fc2"))
    with torch.inference_mode():
        assert fused(torch.randn((1, 3, 32, 32), generator=torch.Generator().manual_seed(0))).shape == (1, 128)

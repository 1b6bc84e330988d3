"""The plain-encoder and concat-skip UNets on the GPU (``-m gpu``): the two streaming kernels against the CPU references of
``_unet_plain_ref.py``, the graphs against the plain module, and what ``SemanticSegmentor`` runs for them.

* ``tia_avgpool2x2_nhwc_*``: EQUALITY with CPU ``F.avg_pool2d(x, 2, 2)`` in float32 / fp16 / bf16 (``test_unet_plain.py`` shows that
  to be the sequential order ``((x00 + x01) + x10) + x11`` and the pairwise order to differ on these inputs);
* ``tia_upsample2x_concat_act_nhwc_*``: EQUALITY with the torch expression evaluated on the CPU in float32, then ``.to(dtype)``;
  one hand-worked pixel on which a fused multiply-add gives another number;
* both with element offsets beyond 2^31 (fp16; only the last image goes to the CPU);
* graphs: float32 logits within 2e-4 of their range (the bound ``test_semantic.py`` uses for ``FusedUNet``); fp16 / bf16
  ``e_new <= 2 * e_lib`` as defined at the top of ``test_unet_half_gpu.py``.
"""

from __future__ import annotations

import copy
import logging
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _unet_half_ref as R  # noqa: E402, N812
from _unet_plain_ref import (CONCAT_SHAPES, CONFIGS, DTYPES, POOL_SHAPES, build, concat_hand_example, concat_ref,  # noqa: E402
                             fused_class)

pytestmark = pytest.mark.gpu

DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
IDS = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
all_dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=[IDS[d] for d in DTYPES])
halves = pytest.mark.parametrize("dtype", R.HALVES, ids=[IDS[d] for d in R.HALVES])
EINVAL, ESIZE = -1, -3


def _nhwc(t):  # NCHW values -> the same tensor stored channels-last on the device
    return t.cuda().contiguous(memory_format=torch.channels_last)


# --------------------------------------------------------------------------------------------------------------------- pooling
@all_dtypes
def test_avgpool_equals_cpu_avg_pool2d(dtype):
    from tiatoolbox_amd.models.architecture.fused import hip_avgpool2x2

    g = torch.Generator().manual_seed(21)
    shapes = POOL_SHAPES + (((2, 2, 2, 4),) if dtype == torch.float32 else ())  # one float32 vector per pixel
    for n, h, w, c in shapes:
        x = (torch.randn((n, c, h, w), generator=g) * 3).to(dtype)
        want = F.avg_pool2d(x, 2, 2)
        got = hip_avgpool2x2(_nhwc(x))
        assert got.dtype == dtype and got.shape == (n, c, h // 2, w // 2) and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got.cpu(), want), (n, h, w, c, float((got.cpu().float() - want.float()).abs().max()))


@all_dtypes
def test_avgpool_refuses_what_it_cannot_take(dtype):
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_avgpool2x2

    lib, stream = _lib.load(), _lib.current_stream()
    vec = 4 if dtype == torch.float32 else 8
    x = torch.ones((1, 4, 4, 2 * vec), dtype=dtype, device="cuda")  # NHWC
    out = torch.zeros((1, 2, 2, 2 * vec), dtype=dtype, device="cuda")

    def call(xp, yp, n, h, w, c, code=DT[dtype]):
        if dtype == torch.float32:
            return lib.tia_avgpool2x2_nhwc_f32(xp, yp, n, h, w, c, stream)
        return lib.tia_avgpool2x2_nhwc_h(xp, yp, n, h, w, c, code, stream)

    assert call(x.data_ptr(), out.data_ptr(), 1, 4, 4, vec // 2) == ESIZE      # less than a 16-byte vector of channels
    assert call(x.data_ptr(), out.data_ptr(), 1, 4, 4, vec + vec // 2) == ESIZE
    assert call(x.data_ptr(), out.data_ptr(), 1, 1, 4, 2 * vec) == EINVAL      # h < 2
    assert call(x.data_ptr(), out.data_ptr(), 1, 4, 1, 2 * vec) == EINVAL      # w < 2
    assert call(x.data_ptr(), out.data_ptr(), 0, 4, 4, 2 * vec) == EINVAL
    assert call(x.data_ptr(), out.data_ptr(), -1, 4, 4, 2 * vec) == EINVAL
    assert call(0, out.data_ptr(), 1, 4, 4, 2 * vec) == EINVAL and call(x.data_ptr(), 0, 1, 4, 4, 2 * vec) == EINVAL
    assert call(x.data_ptr() + 8, out.data_ptr(), 1, 2, 2, 2 * vec) == EINVAL  # misaligned
    assert call(x.data_ptr(), out.data_ptr() + 8, 1, 2, 2, 2 * vec) == EINVAL
    if dtype != torch.float32:
        assert call(x.data_ptr(), out.data_ptr(), 1, 4, 4, 2 * vec, code=0) == EINVAL  # the float32 dtype code
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched
    assert call(x.data_ptr(), out.data_ptr(), 1, 4, 4, 2 * vec) == 0 and bool((out == 1).all())  # (the same arguments, accepted)
    with pytest.raises(ValueError, match="c % 8 == 0"):
        hip_avgpool2x2(_nhwc(torch.zeros((1, vec // 2, 4, 4), dtype=dtype)))
    with pytest.raises(ValueError, match="h >= 2"):
        hip_avgpool2x2(_nhwc(torch.zeros((1, vec, 1, 4), dtype=dtype)))
    with pytest.raises(ValueError, match="channels-last"):
        hip_avgpool2x2(torch.zeros((1, vec, 4, 4), dtype=dtype, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------- concat
@all_dtypes
def test_concat_equals_the_float32_torch_expression(dtype):
    from tiatoolbox_amd.models.architecture.fused import hip_upsample2x_concat

    g = torch.Generator().manual_seed(31)
    shapes = CONCAT_SHAPES + (((2, 1, 1, 4, 4),) if dtype == torch.float32 else ())
    for n, h, w, cx, cy in shapes:
        x = torch.randn((n, cx, h, w), generator=g).to(dtype)
        y = torch.randn((n, cy, 2 * h, 2 * w), generator=g).to(dtype)
        sc, sh = torch.rand(cx + cy, generator=g) + 0.5, torch.randn(cx + cy, generator=g)
        for act in (False, True):
            want = concat_ref(x, y, sc if act else None, sh if act else None)
            got = hip_upsample2x_concat(_nhwc(x), _nhwc(y), sc.cuda() if act else None, sh.cuda() if act else None)
            assert got.dtype == dtype and got.shape == (n, cx + cy, 2 * h, 2 * w)
            assert got.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(got.cpu(), want), (n, h, w, cx, cy, act, float((got.cpu().float() - want.float()).abs().max()))
            if act:
                assert (want == 0).any() and (want > 0).any()  # the ReLU cuts


@all_dtypes
def test_concat_hand_worked_pixel_on_the_device(dtype):
    """The pixel that tells two roundings from a fused multiply-add: the two really differ on it (asserted on the CPU), and the
    kernel gives the separately rounded one."""
    from tiatoolbox_amd.models.architecture.fused import hip_upsample2x_concat

    x, y, scale, shift, want_act, want_plain = concat_hand_example(dtype)
    assert torch.equal(concat_ref(x, y, scale, shift).double(), want_act)
    assert not torch.equal(concat_ref(x, y, scale, shift, variant="fma").double(), want_act)
    assert torch.equal(hip_upsample2x_concat(_nhwc(x), _nhwc(y), scale.cuda(), shift.cuda()).cpu().double(), want_act)
    assert torch.equal(hip_upsample2x_concat(_nhwc(x), _nhwc(y)).cpu().double(), want_plain)


@all_dtypes
def test_concat_refuses_what_it_cannot_take(dtype):
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_upsample2x_concat

    lib, stream = _lib.load(), _lib.current_stream()
    vec = 4 if dtype == torch.float32 else 8
    x = torch.ones((1, 2, 2, 2 * vec), dtype=dtype, device="cuda")  # NHWC
    y = torch.ones((1, 4, 4, 2 * vec), dtype=dtype, device="cuda")
    out = torch.zeros((1, 4, 4, 4 * vec), dtype=dtype, device="cuda")
    aff = torch.ones(4 * vec + 4, device="cuda")

    def call(xp, yp, scp, shp, op, n, h, w, cx, cy, code=DT[dtype]):
        if dtype == torch.float32:
            return lib.tia_upsample2x_concat_act_nhwc_f32(xp, yp, scp, shp, op, n, h, w, cx, cy, stream)
        return lib.tia_upsample2x_concat_act_nhwc_h(xp, yp, scp, shp, op, n, h, w, cx, cy, code, stream)

    xp, yp, op, ap = x.data_ptr(), y.data_ptr(), out.data_ptr(), aff.data_ptr()
    assert call(xp, yp, 0, 0, op, 1, 2, 2, vec // 2, 2 * vec) == ESIZE and call(xp, yp, 0, 0, op, 1, 2, 2, 2 * vec, vec + vec // 2) == ESIZE
    assert call(xp, yp, 0, 0, op, 0, 2, 2, 2 * vec, 2 * vec) == EINVAL and call(xp, yp, 0, 0, op, 1, 0, 2, 2 * vec, 2 * vec) == EINVAL
    assert call(xp, yp, 0, 0, op, 1, 2, 0, 2 * vec, 2 * vec) == EINVAL and call(xp, yp, 0, 0, op, 1, 2, 2, 0, 2 * vec) == EINVAL
    assert call(0, yp, 0, 0, op, 1, 2, 2, 2 * vec, 2 * vec) == EINVAL and call(xp, 0, 0, 0, op, 1, 2, 2, 2 * vec, 2 * vec) == EINVAL
    assert call(xp, yp, 0, 0, 0, 1, 2, 2, 2 * vec, 2 * vec) == EINVAL
    assert call(xp, yp, ap, 0, op, 1, 2, 2, 2 * vec, 2 * vec) == EINVAL and call(xp, yp, 0, ap, op, 1, 2, 2, 2 * vec, 2 * vec) == EINVAL  # one of the two
    assert call(xp + 8, yp, 0, 0, op, 1, 1, 1, 2 * vec, 2 * vec) == EINVAL and call(xp, yp + 8, 0, 0, op, 1, 1, 1, 2 * vec, 2 * vec) == EINVAL
    assert call(xp, yp, 0, 0, op + 8, 1, 1, 1, 2 * vec, 2 * vec) == EINVAL and call(xp, yp, ap + 4, ap, op, 1, 2, 2, 2 * vec, 2 * vec) == EINVAL
    if dtype != torch.float32:
        assert call(xp, yp, 0, 0, op, 1, 2, 2, 2 * vec, 2 * vec, code=0) == EINVAL
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched
    assert call(xp, yp, 0, 0, op, 1, 2, 2, 2 * vec, 2 * vec) == 0 and bool((out == 1).all())  # (the same arguments, accepted)
    xc, yc = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match="one dtype"):
        hip_upsample2x_concat(xc, yc.to(torch.float16 if dtype != torch.float16 else torch.float32))
    with pytest.raises(ValueError, match="one dtype"):
        hip_upsample2x_concat(xc, yc[:, :, :2, :2])  # not [2h, 2w]
    with pytest.raises(ValueError, match="scale / shift in float32"):
        hip_upsample2x_concat(xc, yc, aff[:4 * vec].to(torch.float64), aff[:4 * vec].to(torch.float64))
    with pytest.raises(ValueError, match="scale / shift in float32"):
        hip_upsample2x_concat(xc, yc, aff[:2 * vec], aff[:2 * vec])  # x's channels only
    with pytest.raises(ValueError, match="both or neither"):
        hip_upsample2x_concat(xc, yc, aff[:4 * vec], None)


# ----------------------------------------------------------------------------------------------------- offsets beyond 2^31 elements
def test_avgpool_offsets_beyond_2_31_elements():
    """[33, 1024, 1024, 64] fp16: the last image starts at element 2^31 exactly."""
    from tiatoolbox_amd.models.architecture.fused import hip_avgpool2x2

    torch.manual_seed(5)
    x = (torch.randn((33, 1024, 1024, 64), dtype=torch.float16, device="cuda") * 3).permute(0, 3, 1, 2)
    assert x.numel() > 2 ** 31 and x.is_contiguous(memory_format=torch.channels_last)
    got = hip_avgpool2x2(x)
    assert got.shape == (33, 64, 512, 512)
    assert torch.equal(got[-1:].cpu(), F.avg_pool2d(x[-1:].cpu(), 2, 2))
    assert torch.equal(got[:1], hip_avgpool2x2(x[:1]))  # (and the first one is what a call below 2^31 gives)


def test_concat_offsets_beyond_2_31_elements():
    """To [17, 1024, 1024, 128] fp16: the last output image starts at element 2^31 exactly."""
    from tiatoolbox_amd.models.architecture.fused import hip_upsample2x_concat

    torch.manual_seed(6)
    x = torch.randn((17, 512, 512, 64), dtype=torch.float16, device="cuda").permute(0, 3, 1, 2)
    y = torch.randn((17, 1024, 1024, 64), dtype=torch.float16, device="cuda").permute(0, 3, 1, 2)
    got = hip_upsample2x_concat(x, y)
    assert got.shape == (17, 128, 1024, 1024) and got.numel() > 2 ** 31
    assert torch.equal(got[-1:].cpu(), concat_ref(x[-1:].cpu(), y[-1:].cpu()))
    assert torch.equal(got[:1], hip_upsample2x_concat(x[:1], y[:1]))


# ---------------------------------------------------------------------------------------------------------------------- graphs
@pytest.fixture(scope="module")
def cases():
    """``{name: (model, x, float32 CPU logits)}``: built and run on the CPU once; the tests leave them unchanged."""
    out = {}
    for name in CONFIGS:
        model, x = build(name)
        with torch.inference_mode():
            out[name] = (model, x, model(x))
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_float32_graph_matches_the_plain_module(cases, conv_algo, name):
    from tiatoolbox_amd.models.architecture.hovernet_fused import set_conv_algo

    model, x, ref = cases[name]
    fused = fused_class(name)(copy.deepcopy(model).cuda()).cuda().eval()
    set_conv_algo(fused, "winograd" if conv_algo == "auto" else conv_algo)  # what the engine does with the run kwarg
    with torch.inference_mode():
        got = fused(_nhwc(x)).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    err, bound = float((got - ref).abs().max()), 2e-4 * max(float(ref.abs().max()), 1.0)
    print(f"graph fp32 {name} {conv_algo}: max err {err:.3e}  bound {bound:.3e}")
    assert err <= bound


@halves
@pytest.mark.parametrize("name", list(CONFIGS))
def test_half_graph_is_as_close_to_float32_as_the_cast_module(cases, name, dtype):
    model, x, ref = cases[name]
    fused = fused_class(name)(copy.deepcopy(model).cuda())
    fused.prepare(dtype)
    fused = fused.to(dtype).to(memory_format=torch.channels_last).eval()
    yard, cast = "the cast torch module on the GPU", None
    try:
        cast = copy.deepcopy(model).cuda().to(dtype).to(memory_format=torch.channels_last).eval()
        with torch.inference_mode():
            cast(_nhwc(x.to(dtype)))
            torch.cuda.synchronize()
    except RuntimeError as exc:  # the library has no kernel for this dtype here: the CPU module cast to it is the yardstick
        yard, cast = f"the cast torch module on the CPU (the GPU library refused {dtype}: {exc})", copy.deepcopy(model).to(dtype).eval()
    with torch.inference_mode():
        x_half = x.to(dtype)  # 0 .. 255 are half numbers
        got = fused(_nhwc(x_half))
        dev = next(cast.parameters()).device
        lib = cast(x_half.to(dev).contiguous(memory_format=torch.channels_last)).float().cpu()
    assert got.dtype == torch.float32 and got.shape == ref.shape and torch.isfinite(got).all()
    e_new, e_lib = R.rel_err(got.cpu(), ref), R.rel_err(lib, ref)
    print(f"graph {IDS[dtype]} {name}: e_new {e_new:.3e}  e_lib {e_lib:.3e}  ({yard})")
    assert e_new <= 2 * e_lib, f"e_new {e_new:.3e} > 2 x e_lib {e_lib:.3e}; yardstick: {yard}"


# ---------------------------------------------------------------------------------------------------------------------- engine
def _engine(device: str, **model_kwargs):
    from tiatoolbox_amd.models.architecture.unet import UNetModel
    from tiatoolbox_amd.models.engine.io_config import IOSegmentorConfig
    from tiatoolbox_amd.models.engine.semantic_segmentor import SemanticSegmentor

    torch.manual_seed(4)
    model = UNetModel(3, 2, "unet", decoder_block=[3], **model_kwargs).eval()
    R.randomise_bn(model, 6)
    cfg = IOSegmentorConfig(input_resolutions=[{"units": "mpp", "resolution": 0.25}],
                            output_resolutions=[{"units": "mpp", "resolution": 0.25}], patch_input_shape=[64, 64],
                            patch_output_shape=[32, 32], stride_shape=[32, 32],
                            save_resolution={"units": "mpp", "resolution": 0.25})
    return SemanticSegmentor(model, batch_size=2, device=device), cfg


@pytest.fixture(scope="module")
def patches():
    from tiatoolbox_amd.utils import synth

    return synth.g_he(2, 64, 64, seed=4)


def _probs(eng, cfg, patches, **kwargs):
    return np.asarray(eng.run(patches, patch_mode=True, ioconfig=cfg, return_probabilities=True, **kwargs)["probabilities"])


def test_engine_runs_the_plain_unet_on_the_fused_graph(patches):
    eng, cfg = _engine("cuda")
    for dtype in (torch.float32, torch.float16):
        m = eng._inference_model(dtype)  # noqa: SLF001
        assert type(m).__name__ == "FusedPlainUNet" and m.half_dtype == (None if dtype == torch.float32 else dtype)
    cpu, cfg_cpu = _engine("cpu")
    want = _probs(cpu, cfg_cpu, patches)
    got = _probs(eng, cfg, patches)
    assert got.shape == want.shape == (2, 96, 96, 2) and got.dtype == np.float32  # full-resolution logits x 2, less h // 2
    assert np.abs(got - want).max() <= 1e-4, np.abs(got - want).max()


def test_engine_plain_unet_run_launches_the_hand_written_kernels_only(patches):
    from torch.profiler import ProfilerActivity, profile

    eng, cfg = _engine("cuda")
    _probs(eng, cfg, patches)  # builds the inference copy
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out = _probs(eng, cfg, patches)
        torch.cuda.synchronize()
    assert np.isfinite(out).all()
    names = {e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()}
    kernels = {n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()}
    assert any("avgpool2x2" in k for k in kernels), kernels
    assert any("conv_mfma_f32_kernel" in k for k in kernels), kernels
    banned = ("igemm", "naive_conv", "SubTensorOp", "ck::", "miopen", "MIOpen", "Im2Col", "gemm_conv", "grouped_conv_fwd")
    banned += ("avg_pool2d", "upsample_nearest", "CatArray")  # the ATen kernels the two new passes replace
    offenders = {k for k in kernels if any(b in k for b in banned)}
    assert not offenders, offenders


def test_engine_warns_once_and_runs_the_torch_module_when_a_layer_has_no_kernel(patches, caplog):
    eng, cfg = _engine("cuda", encoder_levels=[4, 8, 16])
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = _probs(eng, cfg, patches)
        got_again = _probs(eng, cfg, patches)  # the cached copy: no second warning
    warned = [r.getMessage() for r in caplog.records if "library" in r.getMessage()]
    assert len(warned) == 1 and "backbone.blocks.0.0.0" in warned[0], [r.getMessage() for r in caplog.records]
    assert type(eng._inference_model(torch.float32)).__name__ == "UNetModel"  # noqa: SLF001
    cpu, cfg_cpu = _engine("cpu", encoder_levels=[4, 8, 16])
    want = _probs(cpu, cfg_cpu, patches)
    assert np.array_equal(got, got_again) and np.abs(got - want).max() <= 1e-4, np.abs(got - want).max()


def test_engine_names_a_library_convolution_inside_a_fused_unet(caplog):
    """A ResNet-50 UNet with a 64 -> 48 decoder convolution still runs on ``FusedUNet`` in float32; the engine says which layers call
    the library, once per inference copy."""
    from tiatoolbox_amd.models.engine.semantic_segmentor import SemanticSegmentor

    model, _ = build("resnet50-concat")
    model = copy.deepcopy(model)
    model.uplist[3][5] = torch.nn.Conv2d(64, 48, 3, padding=1, bias=False)
    model.clf = torch.nn.Conv2d(48, 5, 1)
    eng = SemanticSegmentor(model, batch_size=2, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        m = eng._inference_model(torch.float32)  # noqa: SLF001
        eng._inference_model(torch.float32)  # noqa: SLF001  (cached: no second warning)
    warned = [r.getMessage() for r in caplog.records if "library" in r.getMessage()]
    assert type(m).__name__ == "FusedUNet" and len(warned) == 1 and "up.3.2, clf" in warned[0], warned

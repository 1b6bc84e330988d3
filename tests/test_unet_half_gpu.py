"""The half-precision ``FusedUNet`` on the GPU (``-m gpu``): its three glue kernels against the CPU references of
``_unet_half_ref.py``, the whole graph against the plain module, and what ``SemanticSegmentor`` runs for
``compute_dtype="float16" | "bfloat16"``.

* ``tia_upsample2x_add_act_nhwc_h``: EQUALITY with the float32 sequence of separate torch ops followed by ``.to(dtype)``;
* ``tia_stem_conv7x7_pool_conv_nhwc``: both half maps BIT-EQUAL to the float32 kernel's maps through ``.to(dtype)``;
* ``tia_conv1x1_head_nhwc_h``: float64 reference on the half inputs, bound ``66 * 2^-24 * (sum |w * pre(x)| + |bias|)``;
* graph: ``e_new <= 2 * e_lib`` with ``e = max |logits - ref| / max(max |ref|, 1)``, ``ref`` the plain float32 CPU module, ``e_lib`` the
  error of the torch module cast to the dtype (what the option ran before): both round every activation once per layer.
"""

from __future__ import annotations

import copy
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _unet_half_ref as R  # noqa: E402, N812

pytestmark = pytest.mark.gpu

DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
IDS = {torch.float16: "fp16", torch.bfloat16: "bf16"}
halves = pytest.mark.parametrize("dtype", R.HALVES, ids=[IDS[d] for d in R.HALVES])


def _nhwc(t):  # NCHW values -> the same tensor stored channels-last on the device
    return t.cuda().contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------ upsample + add (+ BN + ReLU)
@halves
@pytest.mark.parametrize("layout", ["dense", "view"])
def test_upsample_add_equals_the_float32_op_sequence(dtype, layout):
    """n = 2; h x w in {1 x 1, 3 x 5, 8 x 8}; c in {8, 64, 136} (one vector, the UNet's narrowest map, no power of two); the skip
    dense or a centre-cropped view of a buffer with a wider row and image stride; with and without scale / shift; values of both
    signs, so the ReLU cuts about half of them.  8 x 8 x 136 channels is several workgroup rows and two blocks per row."""
    from tiatoolbox_amd.models.architecture.fused import hip_upsample2x_add

    g = torch.Generator().manual_seed(11)
    for h, w in ((1, 1), (3, 5), (8, 8)):
        for c in (8, 64, 136):
            x = torch.randn((2, c, h, w), generator=g).to(dtype)
            if layout == "dense":
                y = torch.randn((2, c, 2 * h, 2 * w), generator=g).to(dtype)
                y_dev = _nhwc(y)
            else:
                buf = torch.randn((2, c, 2 * h + 3, 2 * w + 5), generator=g).to(dtype)
                y = buf[:, :, 1:1 + 2 * h, 2:2 + 2 * w]
                y_dev = _nhwc(buf)[:, :, 1:1 + 2 * h, 2:2 + 2 * w]
                assert not y_dev.is_contiguous(memory_format=torch.channels_last)
                assert y_dev.stride(2) == (2 * w + 5) * c and y_dev.stride(0) == (2 * h + 3) * (2 * w + 5) * c
            sc, sh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
            for act in (False, True):
                want = R.upsample_add_ref(x, y, sc if act else None, sh if act else None)
                got = hip_upsample2x_add(_nhwc(x), y_dev, sc.cuda() if act else None, sh.cuda() if act else None)
                assert got.dtype == dtype and got.is_contiguous(memory_format=torch.channels_last)
                assert torch.equal(got.cpu(), want), (h, w, c, act, float((got.cpu().float() - want.float()).abs().max()))
                if act:
                    assert (want == 0).any() and (want > 0).any()


@halves
def test_upsample_add_hand_worked_pixel_on_the_device(dtype):
    """The pixel that tells two roundings from a fused multiply-add, and a late rounding of ``s`` from an early one."""
    from tiatoolbox_amd.models.architecture.fused import hip_upsample2x_add

    x, y, scale, shift, want_act, want_plain = R.hand_example(dtype)
    assert torch.equal(hip_upsample2x_add(_nhwc(x), _nhwc(y), scale.cuda(), shift.cuda()).cpu().double(), want_act)
    assert torch.equal(hip_upsample2x_add(_nhwc(x), _nhwc(y)).cpu().double(), want_plain)


@halves
def test_upsample_add_refuses_what_it_cannot_take(dtype):
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_upsample2x_add

    lib = _lib.load()
    x4, y4 = _nhwc(torch.zeros((1, 4, 2, 2), dtype=dtype)), _nhwc(torch.zeros((1, 4, 4, 4), dtype=dtype))
    with pytest.raises(ValueError, match="c % 8 == 0"):
        hip_upsample2x_add(x4, y4)  # 4 halves are 8 bytes
    out = torch.zeros((1, 8, 4, 4), dtype=dtype, device="cuda")
    stream = _lib.current_stream()
    assert lib.tia_upsample2x_add_act_nhwc_h(x4.data_ptr(), y4.data_ptr(), 64, 16, 0, 0, out.data_ptr(), 1, 2, 2, 4, DT[dtype], stream) == -3
    # a view whose base sits 8 bytes into a 16-byte unit, and one whose row stride is no multiple of 8 elements
    x8 = _nhwc(torch.zeros((1, 8, 2, 2), dtype=dtype))
    flat = torch.zeros(4 + 4 * 4 * 8 + 64, dtype=dtype, device="cuda")
    off = torch.as_strided(flat, (1, 8, 4, 4), (128, 1, 32, 8), storage_offset=4)
    assert off.data_ptr() % 16 == 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip_upsample2x_add(x8, off)
    assert lib.tia_upsample2x_add_act_nhwc_h(x8.data_ptr(), off.data_ptr(), 128, 32, 0, 0, out.data_ptr(), 1, 2, 2, 8, DT[dtype], stream) == -1
    odd = torch.as_strided(flat, (1, 8, 4, 4), (160, 1, 36, 8))
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip_upsample2x_add(x8, odd)
    assert lib.tia_upsample2x_add_act_nhwc_h(x8.data_ptr(), flat.data_ptr(), 160, 36, 0, 0, out.data_ptr(), 1, 2, 2, 8, DT[dtype], stream) == -1
    # mixed dtypes, half scale / shift, float32 dtype code
    with pytest.raises(ValueError, match="one dtype"):
        hip_upsample2x_add(x8, torch.zeros((1, 8, 4, 4), device="cuda").contiguous(memory_format=torch.channels_last))
    y8 = _nhwc(torch.zeros((1, 8, 4, 4), dtype=dtype))
    with pytest.raises(ValueError, match="scale / shift in float32"):
        hip_upsample2x_add(x8, y8, torch.ones(8, dtype=dtype, device="cuda"), torch.zeros(8, dtype=dtype, device="cuda"))
    assert lib.tia_upsample2x_add_act_nhwc_h(x8.data_ptr(), y8.data_ptr(), 128, 32, 0, 0, out.data_ptr(), 1, 2, 2, 8, 0, stream) == -1
    assert not out.any()  # nothing was launched


# ------------------------------------------------------------------------------------------------------------------------ stem
def _stem_parts():
    torch.manual_seed(7)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3)
    with torch.no_grad():
        conv.bias.normal_(0, 0.3)  # about half of the channels' outputs are cut by the ReLU
    return conv.cuda()


@halves
@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 130, 70)], ids=["2x64x96", "1x130x70"])
def test_stem_half_outputs_are_the_float32_outputs_rounded_once(dtype, shape):
    """uint8 patches; 130 x 70 has odd conv (65 x 35) and pooled (33 x 18) sizes.  Both maps of the half call == the float32 kernel's
    maps through ``.to(dtype)`` bit for bit, and the old symbol still writes the float32 maps it wrote (also beside a half pooled map)."""
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_stem_conv_pool, pack_stem_weights

    conv = _stem_parts()
    wp, bias = pack_stem_weights(conv), conv.bias.detach()
    n, h, w = shape
    x = torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(h), dtype=torch.uint8).cuda()
    pooled32, conv32 = hip_stem_conv_pool(x, wp, bias, return_conv=True)
    assert pooled32.dtype == conv32.dtype == torch.float32 and (conv32 == 0).any() and (conv32 > 0).any()
    pooled_h, conv_h = hip_stem_conv_pool(x, wp, bias, out_dtype=dtype, return_conv=True)
    assert pooled_h.dtype == conv_h.dtype == dtype and conv_h.shape == (n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    assert torch.equal(pooled_h, pooled32.to(dtype)) and torch.equal(conv_h, conv32.to(dtype))
    assert torch.equal(hip_stem_conv_pool(x, wp, bias, out_dtype=dtype), pooled_h)  # without the pre-pool map: the fast path of the kernel
    # the old symbol, called directly: float32 maps as before, and float32 pre-pool map beside a half pooled map
    lib, stream = _lib.load(), _lib.current_stream()
    for y_dtype, want in ((torch.float32, pooled32), (dtype, pooled_h)):
        y_old = torch.full_like(want, -1.0)
        c_old = torch.full_like(conv32, -1.0)
        rc = lib.tia_stem_conv7x7_pool_nhwc(x.data_ptr(), 1, wp.data_ptr(), bias.data_ptr(), y_old.data_ptr(), DT[y_dtype], c_old.data_ptr(),
                                            n, h, w, stream)
        assert rc == 0 and torch.equal(y_old, want) and torch.equal(c_old, conv32)
    with pytest.raises(ValueError, match="computes in float32"):
        hip_stem_conv_pool(x, wp, bias.to(dtype), out_dtype=dtype, return_conv=True)


# ------------------------------------------------------------------------------------------------------------------------ head
@halves
@pytest.mark.parametrize("with_pre", [False, True], ids=["plain", "pre"])
@pytest.mark.parametrize("cout", [1, 5, 8])
def test_head_within_the_float32_dot_product_bound(dtype, with_pre, cout):
    """npix in {1, 63, 4096 + 5} (less than one 8-pixel group; a ragged last group; more than one pass of a wave, ragged) against
    float64 on the half inputs.  Per element |got - ref| <= 66 * 2^-24 * (sum_c |w * pre(x)| + |bias|); the bound is also asserted
    to be >= 100 x smaller than the range of the outputs of the three sizes together (one pixel with one class has no range of
    its own), so the comparison cannot pass vacuously."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv1x1_head

    g = torch.Generator().manual_seed(100 + cout)
    wgt, bias = torch.randn((cout, 64), generator=g) * 0.2, torch.randn(cout, generator=g)
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.5
    refs, bounds = [], []
    for npix in (1, 63, 4096 + 5):
        x = torch.randn((npix, 64), generator=g).to(dtype)
        ref, bound = R.head_ref(x, wgt, bias, sc if with_pre else None, sh if with_pre else None)
        x_dev = x.cuda().view(1, npix, 1, 64).permute(0, 3, 1, 2)  # [1, 64, npix, 1] stored channels-last
        got = hip_conv1x1_head(x_dev, wgt.cuda(), bias.cuda(), pre_scale=sc.cuda() if with_pre else None,
                               pre_shift=sh.cuda() if with_pre else None)
        assert got.dtype == torch.float32 and got.shape == (1, cout, npix, 1)
        got = got.permute(0, 2, 3, 1).reshape(npix, cout).cpu().double()
        excess = ((got - ref).abs() - bound).max()
        print(f"head {IDS[dtype]} cout {cout} pre {with_pre} npix {npix}: max err {float((got - ref).abs().max()):.3e}, "
              f"max err / bound {float(((got - ref).abs() / bound).max()):.3f}")
        assert float(excess) <= 0.0, (npix, float(excess))
        refs.append(ref.flatten())
        bounds.append(bound.flatten())
    refs, bounds = torch.cat(refs), torch.cat(bounds)
    assert float(bounds.max()) * 100 <= float(refs.max() - refs.min())


@halves
def test_head_refuses_mixed_dtypes(dtype):
    from tiatoolbox_amd.models.architecture.fused import hip_conv1x1_head

    x = _nhwc(torch.zeros((1, 64, 2, 2), dtype=dtype))
    with pytest.raises(ValueError, match="in float32 beside"):
        hip_conv1x1_head(x, torch.zeros((5, 64), dtype=dtype, device="cuda"), None)
    with pytest.raises(ValueError, match="64 channels"):
        hip_conv1x1_head(_nhwc(torch.zeros((1, 32, 2, 2), dtype=dtype)), torch.zeros((5, 32), device="cuda"), None)


# ----------------------------------------------------------------------------------------------------------------------- graph
def _half_fused(model, dtype):
    from tiatoolbox_amd.models.architecture.unet_fused import FusedUNet

    fused = FusedUNet(copy.deepcopy(model).cuda())
    fused.prepare(dtype)
    return fused.to(dtype).to(memory_format=torch.channels_last).eval()


@halves
def test_half_graph_is_as_close_to_float32_as_the_cast_module(dtype):
    model, cases = R.graph_case()
    fused = _half_fused(model, dtype)
    yard, cast = "the cast torch module on the GPU", None
    try:
        cast = copy.deepcopy(model).cuda().to(dtype).to(memory_format=torch.channels_last).eval()
        with torch.inference_mode():
            cast(cases[0][0][:1, :, :32, :32].cuda().to(dtype))
            torch.cuda.synchronize()
    except RuntimeError as exc:  # the library has no kernel for this dtype here: the CPU module cast to it is the yardstick
        yard, cast = f"the cast torch module on the CPU (the GPU library refused {dtype}: {exc})", copy.deepcopy(model).to(dtype).eval()
    for x, ref in cases:
        with torch.inference_mode():
            x_half = x.to(dtype)  # 0 .. 255 are half numbers
            got = fused(_nhwc(x_half))
            got_u8 = fused(x.to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2))
            dev = next(cast.parameters()).device
            lib = cast(x_half.to(dev).contiguous(memory_format=torch.channels_last)).float().cpu()
        assert got.dtype == got_u8.dtype == torch.float32 and got.shape == ref.shape
        assert torch.isfinite(got).all() and torch.equal(got, got_u8)
        e_new, e_lib = R.rel_err(got.cpu(), ref), R.rel_err(lib, ref)
        print(f"graph {IDS[dtype]} {tuple(x.shape)}: e_new {e_new:.3e}  e_lib {e_lib:.3e}  ({yard})")
        assert e_new <= 2 * e_lib, f"e_new {e_new:.3e} > 2 x e_lib {e_lib:.3e}; yardstick: {yard}"


def test_prepare_raises_for_a_layer_without_a_half_kernel():
    """A decoder narrower than the MFMA tile has no half kernel: ``TypeError`` when the half copy is prepared, no library fall-back."""
    from tiatoolbox_amd.models.architecture.unet_fused import FusedUNet

    model, _ = R.graph_case()
    m = copy.deepcopy(model)
    m.uplist[3][5] = torch.nn.Conv2d(64, 48, 3, padding=1, bias=False)  # cout % 64 != 0 (float32 runs it as a torch convolution)
    m.clf = torch.nn.Conv2d(48, 5, 1)
    fused = FusedUNet(m.cuda())
    with pytest.raises(TypeError, match="no torch.float16 kernel"):
        fused.prepare(torch.float16)


# ---------------------------------------------------------------------------------------------------------------------- engine
def _engine():
    from tiatoolbox_amd.models.engine.io_config import IOSegmentorConfig
    from tiatoolbox_amd.models.engine.semantic_segmentor import SemanticSegmentor

    model, _ = R.graph_case()
    cfg = IOSegmentorConfig(input_resolutions=[{"units": "mpp", "resolution": 0.25}],
                            output_resolutions=[{"units": "mpp", "resolution": 0.25}], patch_input_shape=[128, 128],
                            patch_output_shape=[64, 64], stride_shape=[50, 50],
                            save_resolution={"units": "mpp", "resolution": 0.25})
    return SemanticSegmentor(copy.deepcopy(model), batch_size=2, device="cuda"), cfg


@halves
def test_engine_builds_the_fused_unet_for_half(dtype):
    eng, _ = _engine()
    m = eng._inference_model(dtype)  # noqa: SLF001
    assert type(m).__name__ == "FusedUNet" and m.half_dtype == dtype and next(m.parameters()).dtype == dtype
    assert type(eng._inference_model(torch.float32)).__name__ == "FusedUNet"  # noqa: SLF001
    assert eng._inference_model(torch.float32).half_dtype is None  # noqa: SLF001


def test_engine_patch_mode_float16_and_float32_unchanged_around_it():
    from tiatoolbox_amd.models.architecture.unet import UNetModel
    from tiatoolbox_amd.utils import synth

    eng, cfg = _engine()
    patches = synth.g_he(3, 128, 128, seed=4)
    before = eng.run(patches, patch_mode=True, ioconfig=cfg, return_probabilities=True, compute_dtype="float32")
    out = eng.run(patches, patch_mode=True, ioconfig=cfg, return_probabilities=True, compute_dtype="float16")
    probs = np.asarray(out["probabilities"])
    assert probs.shape == (3, 64, 64, 5) and probs.dtype == np.float32 and np.isfinite(probs).all()
    copy_h = eng._inference_model(torch.float16)  # noqa: SLF001  (the cached copy the run used)
    assert type(copy_h).__name__ == "FusedUNet"
    want = torch.cat([UNetModel.infer_batch(copy_h, torch.from_numpy(patches[i:i + 2]).cuda(), device="cuda") for i in (0, 2)]).cpu().numpy()
    assert np.abs(probs - want).max() <= 1e-6
    after = eng.run(patches, patch_mode=True, ioconfig=cfg, return_probabilities=True, compute_dtype="float32")
    assert np.array_equal(np.asarray(before["probabilities"]), np.asarray(after["probabilities"]))  # the cache key separates the copies
    assert np.array_equal(np.asarray(before["predictions"]), np.asarray(after["predictions"]))


def test_engine_wsi_mode_float16_writes_the_slide():
    from tiatoolbox_amd.utils import synth
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    eng, cfg = _engine()
    slide = np.full((600, 700, 3), 245, np.uint8)
    slide[64:480, 96:600] = synth.g_he(1, 416, 504, seed=3)[0]
    reader = ArrayWSIReader(slide, mpp=0.25, power=40)
    with tempfile.TemporaryDirectory() as tmp:
        paths = eng.run([reader], patch_mode=False, ioconfig=cfg, return_probabilities=True, save_dir=Path(tmp) / "out",
                        compute_dtype="float16")
        assert list(paths) == [0] and paths[0].name == "0.npz"
        with np.load(paths[0]) as res:
            pred, probs = res["predictions"], res["probabilities"]
    assert pred.shape == (600, 700) and pred.dtype == np.uint8 and np.isfinite(probs).all()


@halves
def test_engine_half_run_launches_the_hand_written_kernels_only(dtype):
    from torch.profiler import ProfilerActivity, profile

    from tiatoolbox_amd.utils import synth

    eng, cfg = _engine()
    x = synth.g_he(2, 128, 128, seed=4)
    name = str(dtype).replace("torch.", "")
    eng.run(x, patch_mode=True, ioconfig=cfg, return_probabilities=True, compute_dtype=name)  # builds the inference copy
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out = eng.run(x, patch_mode=True, ioconfig=cfg, return_probabilities=True, compute_dtype=name)
        torch.cuda.synchronize()
    assert np.isfinite(np.asarray(out["probabilities"])).all()
    names = {e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()}
    kernels = {n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()}
    for wanted in ("stem7x7_pool_convh_kernel", "conv_mfma_h_kernel", "upsample2x_add_h_kernel", "head1x1_h_kernel"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    banned = ("igemm", "naive_conv", "SubTensorOp", "ck::", "miopen", "MIOpen", "Im2Col", "gemm_conv", "grouped_conv_fwd")
    offenders = {k for k in kernels if any(b in k for b in banned)}
    assert not offenders, offenders

"""The half-precision ``FusedHoVerNet`` on the GPU (``-m gpu``): its four new kernels against the CPU references of
``_hovernet_half_ref.py``, the whole graph against the plain module, and what ``NucleusInstanceSegmentor`` runs for
``compute_dtype="float16" | "bfloat16"``.

* ``tia_conv2d_nhwc_h_ex``: float32 CPU convolution of the same half-rounded operands, ``eps |ref| + 1e-4 max |ref|`` (the second output:
  the same bound propagated through the affine); equality with ``tia_conv2d_nhwc_h`` where both apply; one hand-made case decided by
  EQUALITY that shows the second output comes from the unrounded sum;
* ``tia_grouped_conv_valid_nhwc_h``: float64 on the half operands, ``2 K 2^-24 sum |w x| + eps |ref|``; nothing outside the output view
  is written;
* ``tia_scale_shift_act_view_nhwc_h``: EQUALITY with the float32 sequence of separate torch ops followed by ``.to(dtype)``;
* ``tia_conv2d_thin_nhwc``: BIT-EQUAL to the float32 entry point's output through ``.to(dtype)``;
* graph: ``e_new <= 2 e_lib`` per head with ``e = max |logits - ref| / max(max |ref|, 1)``, ``ref`` the plain float32 CPU module, ``e_lib``
  the error of the torch module cast to the dtype (what the option ran before).
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
import _hovernet_half_ref as R  # noqa: E402, N812

pytestmark = pytest.mark.gpu

DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
halves = pytest.mark.parametrize("dtype", R.HALVES, ids=[R.IDS[d] for d in R.HALVES])
EINVAL, ESIZE = -1, -3


def _nhwc(t):  # NCHW values -> the same tensor stored channels-last on the device
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _pack(w_half_oihw, dtype):
    """Pack on the device from the float32 image of already-rounded weights (the second rounding is the identity)."""
    from tiatoolbox_amd.models.architecture.fused import pack_conv_weights_h

    conv = torch.nn.Conv2d(w_half_oihw.shape[1], w_half_oihw.shape[0], w_half_oihw.shape[2], bias=False)
    conv.weight.data = w_half_oihw.float()
    wp = pack_conv_weights_h(conv.cuda(), dtype)
    assert torch.equal(wp.cpu(), R.pack_h(w_half_oihw.float(), dtype))
    return wp


def _within(got, ref, bound, what):
    err = (got.double() - ref.double()).abs()
    print(f"{what}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert float((err - bound).max()) <= 0.0, what


# ------------------------------------------------------------------------------------------- convolution, extended epilogue
@halves
@pytest.mark.parametrize(("shape", "cin", "cout"), [((2, 10, 12), 32, 64), ((2, 10, 12), 64, 128), ((1, 9, 13), 32, 128), ((1, 9, 13), 64, 64)],
                         ids=["2x10x12-32-64", "2x10x12-64-128", "1x9x13-32-128", "1x9x13-64-64"])
def test_conv_ex_strided_3x3_with_tf_same_padding(dtype, shape, cin, cout):
    """3x3 / stride 2 with TensorFlow "same" pads: (0, 1) on the even map, (1, 1) on the odd one (``_same_pads`` of the HEIGHT); bias and
    ReLU; 32- and 64-channel inputs (one and two slices per tap), 64- and 128-wide tiles.  On the odd map the pads are symmetric: the
    plain entry point applies too and must agree bit for bit."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv2d_h, hip_conv2d_h_ex
    from tiatoolbox_amd.models.architecture.hovernet_fused import _same_pads

    n, h, w = shape
    g = torch.Generator().manual_seed(h * 100 + cin + cout)
    x = torch.randn((n, cin, h, w), generator=g).to(dtype)
    wgt = (torch.randn((cout, cin, 3, 3), generator=g) * 0.1).to(dtype)
    bias = torch.randn(cout, generator=g) * 0.5
    lo, hi = _same_pads(h, 3, 2)
    assert (lo, hi) == ((0, 1) if h % 2 == 0 else (1, 1))
    ref, _ = R.conv_ex_ref(x, wgt, bias, None, stride=2, pad_lo=lo, pad_hi=hi, relu=True)
    assert (ref == 0).any() and (ref > 0).any()
    wp = _pack(wgt, dtype)
    got = hip_conv2d_h_ex(_nhwc(x), wp, bias.cuda(), None, cout=cout, kernel=3, stride=2, pad_lo=lo, pad_hi=hi, relu=True)
    assert got.dtype == dtype and got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
    _within(got.cpu(), ref, R.conv_bound(ref, dtype), f"conv_ex 3x3/2 {R.IDS[dtype]} {shape} {cin}->{cout} pads {(lo, hi)}")
    if lo == hi:
        plain = hip_conv2d_h(_nhwc(x), wp, bias.cuda(), None, cout=cout, kernel=3, stride=2, padding=lo, relu=True)
        assert torch.equal(got, plain)


@halves
@pytest.mark.parametrize(("shape", "cin", "cout"), [((2, 9, 7), 64, 128), ((3, 12, 12), 32, 64)], ids=["2x9x7-64-128", "3x12x12-32-64"])
def test_conv_ex_1x1_with_residual_and_second_output(dtype, shape, cin, cout):
    """conv3 + shortcut of a residual unit: 126 pixels (one partial 128-pixel tile) and 432 (several tiles, the last partial); raw sum
    and activated copy from one launch, with and without ``d_y``; the raw sum equals the plain entry point's bit for bit."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv2d_h, hip_conv2d_h_ex

    n, h, w = shape
    g = torch.Generator().manual_seed(h + cin)
    x = torch.randn((n, cin, h, w), generator=g).to(dtype)
    wgt = (torch.randn((cout, cin, 1, 1), generator=g) * 0.2).to(dtype)
    res = torch.randn((n, cout, h, w), generator=g).to(dtype)
    bias = torch.randn(cout, generator=g) * 0.3
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.5
    v_ref, y2_ref = R.conv_ex_ref(x, wgt, bias, res, stride=1, pad_lo=0, pad_hi=0, relu=False, post_scale=sc, post_shift=sh)
    assert (y2_ref == 0).any() and (y2_ref > 0).any()
    wp = _pack(wgt, dtype)
    args = (_nhwc(x), wp, bias.cuda(), _nhwc(res))
    kw = {"cout": cout, "kernel": 1, "stride": 1, "pad_lo": 0, "pad_hi": 0, "relu": False, "post_scale": sc.cuda(), "post_shift": sh.cuda()}
    y, y2 = hip_conv2d_h_ex(*args, **kw)
    what = f"conv_ex 1x1 {R.IDS[dtype]} {shape} {cin}->{cout}"
    _within(y.cpu(), v_ref, R.conv_bound(v_ref, dtype), what + " y")
    _within(y2.cpu(), y2_ref, R.post_bound(y2_ref, v_ref, sc, dtype), what + " y2")
    none, y2_only = hip_conv2d_h_ex(*args, **kw, want_raw=False)
    assert none is None and torch.equal(y2_only, y2)
    plain = hip_conv2d_h(*args, cout=cout, kernel=1, stride=1, padding=0, relu=False)
    assert torch.equal(y, plain)
    assert torch.equal(hip_conv2d_h_ex(*args, cout=cout, kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False), plain)


@halves
def test_conv_ex_second_output_comes_from_the_unrounded_sum(dtype):
    """The hand-made pixel of ``post_hand_example``: v = 1 + half-ulp rounds to 1 for ``y``; ``y2`` = 1 from the unrounded v, where the
    affine applied to the rounded value would give 0.  Decided by equality."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv2d_h_ex

    x, wgt, res, sc, sh, want_y, want_y2 = R.post_hand_example(dtype)
    y, y2 = hip_conv2d_h_ex(_nhwc(x), _pack(wgt, dtype), None, _nhwc(res), cout=64, kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False,
                            post_scale=sc.cuda(), post_shift=sh.cuda())
    assert torch.equal(y.cpu().double(), want_y)
    assert torch.equal(y2.cpu().double(), want_y2), y2.flatten()[:4]


@halves
def test_conv_ex_refuses_what_it_cannot_take(dtype):
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_conv2d_h_ex

    lib, stream = _lib.load(), _lib.current_stream()
    x = _nhwc(torch.zeros((1, 32, 4, 4), dtype=dtype))
    wp = torch.zeros((1, 1, 4, 64, 8), dtype=dtype, device="cuda")
    sc32 = torch.ones(64, device="cuda")
    with pytest.raises(ValueError, match="float32 CUDA tensors"):
        hip_conv2d_h_ex(x, wp, None, None, cout=64, kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False, post_scale=sc32.to(dtype),
                        post_shift=sc32.to(dtype))
    with pytest.raises(ValueError, match="both or neither"):
        hip_conv2d_h_ex(x, wp, None, None, cout=64, kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False, post_scale=sc32)
    with pytest.raises(ValueError, match="beside a"):
        hip_conv2d_h_ex(x, wp.float(), None, None, cout=64, kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False)
    with pytest.raises(ValueError, match="dtype and shape"):
        hip_conv2d_h_ex(x, wp, None, _nhwc(torch.zeros((1, 64, 4, 4))), cout=64, kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False)
    y = torch.zeros((1, 64, 4, 4), dtype=dtype, device="cuda")
    y2 = torch.zeros_like(y)

    def call(xp, cin, cout, yp, scp, shp, y2p, dt=DT[dtype]):
        return lib.tia_conv2d_nhwc_h_ex(xp, wp.data_ptr(), 0, 0, yp, 1, 4, 4, cin, cout, 1, 1, 1, 0, 0, 4, 4, dt, 0, scp, shp, y2p, stream)

    p = (x.data_ptr(), y.data_ptr(), sc32.data_ptr(), y2.data_ptr())
    assert call(p[0], 32, 64, p[1], p[2], p[2], p[3]) == 0
    y.zero_(), y2.zero_()
    assert call(p[0], 16, 64, p[1], 0, 0, 0) == ESIZE and call(p[0], 32, 48, p[1], 0, 0, 0) == ESIZE
    assert call(p[0] + 8, 32, 64, p[1], 0, 0, 0) == EINVAL and call(p[0], 32, 64, p[1], p[2] + 4, p[2], p[3]) == EINVAL
    assert call(p[0], 32, 64, p[1], p[2], p[2], p[3] + 8) == EINVAL
    assert call(p[0], 32, 64, 0, 0, 0, 0) == EINVAL            # no output at all
    assert call(p[0], 32, 64, p[1], p[2], p[2], 0) == EINVAL   # an affine without a second output
    assert call(p[0], 32, 64, p[1], p[2], 0, p[3]) == EINVAL   # a second output without its shift
    assert call(p[0], 32, 64, p[1], 0, 0, 0, dt=0) == EINVAL   # float32 dtype code
    torch.cuda.synchronize()
    assert not y.any() and not y2.any()  # nothing was launched


# ------------------------------------------------------------------------------------------------------------ grouped valid
def _grouped_case(dtype, k, h, w):
    g = torch.Generator().manual_seed(10 * k + h)
    x = torch.randn((2, 128, h, w), generator=g).to(dtype)
    wgt = torch.randn((32, 32, k, k), generator=g) * 0.1
    return x, wgt


@halves
@pytest.mark.parametrize("k", [3, 5])
def test_grouped_valid_within_the_float32_summation_bound(dtype, k):
    """groups = 4, n = 2; h x w = k x k (one output pixel per image), 7 x 9, 20 x 21 (more than one 64-pixel workgroup, the last wave
    tile partial); dense output and a 32-channel slice at channel 64 inside a window of a wider, sentinel-filled buffer -- every element
    outside the slice bit-unchanged.  The bound is also >= 20 x below the output range, so it cannot pass vacuously."""
    from tiatoolbox_amd.models.architecture.fused import hip_grouped_conv_valid_h, pack_grouped_conv_valid_weights_h

    for h, w in ((k, k), (7, 9), (20, 21)):
        x, wgt = _grouped_case(dtype, k, h, w)
        wp = pack_grouped_conv_valid_weights_h(wgt.cuda(), 4, dtype)
        assert wp.dtype == dtype and torch.equal(wp.cpu(), R.pack_grouped_h(wgt, 4, dtype))  # one rounding of the float32 weights
        ref, bound = R.grouped_ref(x, wgt.to(dtype), 4)
        ho, wo = h - k + 1, w - k + 1
        got = hip_grouped_conv_valid_h(_nhwc(x), wp, groups=4, kernel=k)
        assert got.dtype == dtype and got.shape == (2, 32, ho, wo) and got.is_contiguous(memory_format=torch.channels_last)
        _within(got.cpu(), ref, bound, f"grouped {R.IDS[dtype]} k {k} {h}x{w} dense")
        if h > k:
            assert float(bound.max()) * 20 <= float(ref.max() - ref.min())
        sentinel = -7.0
        big = torch.full((2, 160, ho + 3, wo + 4), sentinel, dtype=dtype, device="cuda").contiguous(memory_format=torch.channels_last)
        view = big[:, 64:96, 1:1 + ho, 2:2 + wo]
        out = hip_grouped_conv_valid_h(_nhwc(x), wp, groups=4, kernel=k, out=view)
        assert out.data_ptr() == view.data_ptr()
        assert torch.equal(view, got)  # the same values through the strides
        outside = big.clone()
        outside[:, 64:96, 1:1 + ho, 2:2 + wo] = sentinel
        assert (outside == sentinel).all()


@halves
def test_grouped_valid_refuses_what_it_cannot_take(dtype):
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_grouped_conv_valid_h

    lib, stream = _lib.load(), _lib.current_stream()
    x = _nhwc(torch.zeros((1, 128, 5, 5), dtype=dtype))
    wp = torch.zeros((4, 3, 3, 4, 8, 8), dtype=dtype, device="cuda")
    flat = torch.zeros(8 + 3 * 3 * 40 + 64, dtype=dtype, device="cuda")
    y = torch.zeros((1, 32, 3, 3), dtype=dtype, device="cuda").contiguous(memory_format=torch.channels_last)

    def call(yp, sb, sy, sp, cpg=32, opg=8, k=3, dt=DT[dtype]):
        return lib.tia_grouped_conv_valid_nhwc_h(x.data_ptr(), wp.data_ptr(), yp, sb, sy, sp, 1, 5, 5, 4, cpg, opg, k, dt, stream)

    assert call(y.data_ptr(), 288, 96, 32) == 0
    y.zero_()
    assert call(y.data_ptr(), 288, 96, 32, cpg=16) == ESIZE and call(y.data_ptr(), 288, 96, 32, opg=16) == ESIZE
    assert call(y.data_ptr(), 288, 96, 32, k=4) == ESIZE
    assert call(y.data_ptr(), 360, 120, 36) == EINVAL          # strides that are no multiple of 8
    assert call(y.data_ptr(), 288, 96, 24) == EINVAL           # pixels narrower than the output channels
    assert call(flat.data_ptr() + 8, 360, 120, 40) == EINVAL   # a base 8 bytes into a 16-byte unit
    assert call(y.data_ptr(), 288, 96, 32, dt=0) == EINVAL
    off = torch.as_strided(flat, (1, 32, 3, 3), (360, 1, 120, 40), storage_offset=4)
    assert off.data_ptr() % 16 == 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip_grouped_conv_valid_h(x, wp, groups=4, kernel=3, out=off)
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip_grouped_conv_valid_h(x, wp, groups=4, kernel=3, out=torch.as_strided(flat, (1, 32, 3, 3), (324, 1, 108, 36)))
    with pytest.raises(ValueError, match="do not match"):
        hip_grouped_conv_valid_h(x, wp.float(), groups=4, kernel=3)
    with pytest.raises(ValueError, match="fp16 / bf16 channels-last"):
        hip_grouped_conv_valid_h(x.float(), wp, groups=4, kernel=3)
    torch.cuda.synchronize()
    assert not y.any() and not flat.any()  # nothing was launched


# ---------------------------------------------------------------------------------------------------------- view activation
@halves
def test_view_activation_equals_the_float32_op_sequence(dtype):
    """n = 2; h x w in {1 x 1, 3 x 5, 9 x 8}; c in {8, 160} (one vector; the dense block's widest odd multiple); the input a channel
    prefix of a wider buffer and a cropped window of it; values of both signs, so the ReLU cuts about half."""
    from tiatoolbox_amd.models.architecture.fused import hip_scale_shift_act_view

    g = torch.Generator().manual_seed(21)
    for h, w in ((1, 1), (3, 5), (9, 8)):
        for c in (8, 160):
            buf = torch.randn((2, c + 32, h + 2, w + 3), generator=g).to(dtype)
            sc, sh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5
            view = buf[:, :c, 1:1 + h, 2:2 + w]
            want = R.view_act_ref(view, sc, sh)
            dev = _nhwc(buf)[:, :c, 1:1 + h, 2:2 + w]
            assert dev.stride(3) == c + 32 and dev.stride(2) == (w + 3) * (c + 32)
            got = hip_scale_shift_act_view(dev, sc.cuda(), sh.cuda())
            assert got.dtype == dtype and got.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(got.cpu(), want), (h, w, c, float((got.cpu().float() - want.float()).abs().max()))
            assert (want == 0).any() and (want > 0).any()
            plain = hip_scale_shift_act_view(dev, sc.cuda(), sh.cuda(), relu=False)
            assert torch.equal(plain.cpu(), R.view_act_ref(view, sc, sh, relu=False))


@halves
def test_view_activation_refuses_what_it_cannot_take(dtype):
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_scale_shift_act_view

    lib, stream = _lib.load(), _lib.current_stream()
    sc = torch.ones(8, device="cuda")
    flat = torch.ones(4 + 2 * 2 * 12 + 64, dtype=dtype, device="cuda")
    out = torch.zeros((1, 8, 2, 2), dtype=dtype, device="cuda")

    def call(xp, sb, sy, sp, c=8, dt=DT[dtype]):
        return lib.tia_scale_shift_act_view_nhwc_h(xp, sb, sy, sp, sc.data_ptr(), sc.data_ptr(), out.data_ptr(), 1, 2, 2, c, 1, dt, stream)

    assert call(flat.data_ptr(), 32, 16, 8) == 0
    out.zero_()
    assert call(flat.data_ptr(), 32, 16, 8, c=4) == ESIZE
    assert call(flat.data_ptr(), 48, 24, 12) == EINVAL and call(flat.data_ptr() + 8, 32, 16, 8) == EINVAL
    assert call(flat.data_ptr(), 32, 16, 8, dt=0) == EINVAL
    x4 = _nhwc(torch.zeros((1, 4, 2, 2), dtype=dtype))
    with pytest.raises(ValueError, match="c % 8"):
        hip_scale_shift_act_view(x4, sc[:4], sc[:4])
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip_scale_shift_act_view(torch.as_strided(flat, (1, 8, 2, 2), (32, 1, 16, 8), storage_offset=4), sc, sc)
    with pytest.raises(ValueError, match="16-byte aligned"):
        hip_scale_shift_act_view(torch.as_strided(flat, (1, 8, 2, 2), (48, 1, 24, 12)), sc, sc)
    x8 = _nhwc(torch.zeros((1, 8, 2, 2), dtype=dtype))
    with pytest.raises(ValueError, match="as float32 CUDA"):
        hip_scale_shift_act_view(x8, sc.to(dtype), sc.to(dtype))
    with pytest.raises(ValueError, match="as float32 CUDA"):
        hip_scale_shift_act_view(x8, sc.cpu(), sc.cpu())
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- thin stem
@halves
@pytest.mark.parametrize(("shape", "pad"), [((2, 20, 24), 3), ((1, 17, 19), 0)], ids=["2x20x24-same", "1x17x19-valid"])
def test_thin_stem_half_output_is_the_float32_output_rounded_once(dtype, shape, pad):
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import hip_conv2d_thin, pack_thin_conv_weights

    n, h, w = shape
    torch.manual_seed(7)
    conv = torch.nn.Conv2d(3, 64, 7)
    with torch.no_grad():
        conv.bias.normal_(0, 0.3)  # about half of the outputs are cut by the ReLU
    conv = conv.cuda()
    wp, bias = pack_thin_conv_weights(conv.weight), conv.bias.detach()
    x = (torch.randint(0, 256, (n, 3, h, w), generator=torch.Generator().manual_seed(h)).float() / 255.0).cuda()
    kw = {"kernel": 7, "stride": 1, "pad_lo": pad, "pad_hi": pad, "relu": True}
    y32 = hip_conv2d_thin(x, wp, bias, **kw)
    assert y32.dtype == torch.float32 and (y32 == 0).any() and (y32 > 0).any()
    cut = float((y32 == 0).float().mean())
    assert 0.2 <= cut <= 0.8, cut
    yh = hip_conv2d_thin(x, wp, bias, **kw, out_dtype=dtype)
    assert yh.dtype == dtype and yh.shape == y32.shape and yh.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(yh, y32.to(dtype))
    assert torch.equal(hip_conv2d_thin(x, wp, bias, **kw, out_dtype=torch.float32), y32)  # the old symbol's output is unchanged
    with pytest.raises(ValueError, match="computes in float32"):
        hip_conv2d_thin(x, wp, bias.to(dtype), **kw, out_dtype=dtype)
    # the new entry point with the float32 code is the old one; a misaligned half output is refused
    lib, stream = _lib.load(), _lib.current_stream()
    ho, wo = y32.shape[2], y32.shape[3]
    need = (wo - 1) + 11
    wpad = max(w + 2 * pad, need)
    xp = torch.zeros((n, h, wpad, 3), device="cuda")
    xp[:, :, pad:pad + w] = x.permute(0, 2, 3, 1)
    y_new = torch.full_like(y32, -1.0)
    assert lib.tia_conv2d_thin_nhwc(xp.data_ptr(), wp.data_ptr(), bias.data_ptr(), y_new.data_ptr(), 0, n, h, wpad, 3, 64, 7, 7, 1, pad, ho, wo, 1,
                                    stream) == 0
    assert torch.equal(y_new, y32)
    assert lib.tia_conv2d_thin_nhwc(xp.data_ptr(), wp.data_ptr(), bias.data_ptr(), y_new.data_ptr() + 8, DT[dtype], n, h, wpad, 3, 64, 7, 7, 1, pad,
                                    ho, wo, 1, stream) == EINVAL


# -------------------------------------------------------------------------------------------------------------------- graph
def _half_fused(model, dtype):
    from tiatoolbox_amd.models.architecture.hovernet_fused import FusedHoVerNet

    fused = FusedHoVerNet(copy.deepcopy(model).cuda())
    fused.prepare(dtype)
    return fused.to(dtype).to(memory_format=torch.channels_last).eval()


@halves
@pytest.mark.parametrize("kind", ["fast", "original", "plus"])
def test_half_graph_is_as_close_to_float32_as_the_cast_module(dtype, kind):
    """``fast`` 256^2 (n = 1 and n = 2), ``original`` 270^2, ``HoVerNetPlus`` 256^2; per head e_new <= 2 e_lib."""
    model, x_all, ref_all = R.graph_case(kind)
    fused = _half_fused(model, dtype)
    x_half = x_all.to(dtype)  # 0 .. 255 are half numbers
    yard = "the cast torch module on the GPU"
    try:  # ONE library forward per case, on the whole batch (its images are independent: the n = 1 yardstick is its first image)
        cast = copy.deepcopy(model).cuda().to(dtype).to(memory_format=torch.channels_last).eval()
        with torch.inference_mode():
            lib_all = {k: v.float().cpu() for k, v in cast(_nhwc(x_half)).items()}
    except RuntimeError as exc:  # the library has no kernel for this dtype here: the CPU module cast to it is the yardstick
        yard = f"the cast torch module on the CPU (the GPU library refused {dtype}: {exc})"
        with torch.inference_mode():
            lib_all = {k: v.float() for k, v in copy.deepcopy(model).to(dtype).eval()(x_half).items()}
    for n in ((1, 2) if kind == "fast" else (1,)):
        ref = {k: v[:n] for k, v in ref_all.items()}
        with torch.inference_mode():
            got = fused(_nhwc(x_half[:n]))
        assert list(got) == list(ref)
        for name in ref:
            assert got[name].dtype == torch.float32 and got[name].shape == ref[name].shape and torch.isfinite(got[name]).all()
            e_new, e_lib = R.rel_err(got[name].cpu(), ref[name]), R.rel_err(lib_all[name][:n], ref[name])
            print(f"graph {kind} {R.IDS[dtype]} n {n} head {name}: e_new {e_new:.3e}  e_lib {e_lib:.3e}  ({yard})")
            assert e_new <= 2 * e_lib, f"{name}: e_new {e_new:.3e} > 2 x e_lib {e_lib:.3e}; yardstick: {yard}"


def test_prepare_raises_for_a_layer_without_a_half_kernel():
    from tiatoolbox_amd.models.architecture.hovernet_fused import FusedHoVerNet

    model, _, _ = R.graph_case("fast")
    m = copy.deepcopy(model)
    m.decoder["np"][2].conva = torch.nn.Conv2d(256, 48, 5, bias=False)  # cout % 64 != 0 (float32 runs it as a torch convolution)
    with pytest.raises(TypeError, match="no torch.float16 kernel"):
        FusedHoVerNet(m.cuda()).prepare(torch.float16)


# ------------------------------------------------------------------------------------------------------------------- engine
def _engine():
    import warnings

    from tiatoolbox_amd.models.engine.nucleus_instance_segmentor import NucleusInstanceSegmentor

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)  # (the class name the issue and the bench use)
        return NucleusInstanceSegmentor("hovernet_fast-pannuke", batch_size=2, device="cuda", verbose=False)


def _tiles():
    from tiatoolbox_amd.utils import synth

    return synth.g_he(3, 256, 256, seed=4)


INSTANCE_KEYS = ("box", "centroid", "contours", "prob", "type")


@halves
def test_engine_builds_the_fused_hovernet_for_half(dtype):
    eng = _engine()
    m = eng._inference_model(dtype)  # noqa: SLF001
    assert type(m).__name__ == "FusedHoVerNet" and m.half_dtype == dtype and next(m.parameters()).dtype == dtype
    m32 = eng._inference_model(torch.float32)  # noqa: SLF001
    assert type(m32).__name__ == "FusedHoVerNet" and m32.half_dtype is None and next(m32.parameters()).dtype == torch.float32


def test_engine_patch_mode_float16_and_float32_unchanged_around_it():
    from tiatoolbox_amd.models.architecture.hovernet import HoVerNet

    eng, tiles = _engine(), _tiles()
    before = eng.run(tiles, patch_mode=True, return_probabilities=True, compute_dtype="float32")
    out = eng.run(tiles, patch_mode=True, return_probabilities=True, compute_dtype="float16")
    assert set(out) == set(before) and out["predictions"].shape == before["predictions"].shape == (3, 164, 164)
    assert all(np.isfinite(p).all() and p.dtype == np.float32 for p in out["probabilities"])
    copy_h = eng._inference_model(torch.float16)  # noqa: SLF001  (the cached copy the run used)
    assert type(copy_h).__name__ == "FusedHoVerNet" and copy_h.half_dtype == torch.float16
    # the instance dictionaries are the post-processing of the maps that copy's own `infer_batch` gives for the same tiles
    parts = [HoVerNet.infer_batch(copy_h, torch.from_numpy(tiles[i:i + 2]).cuda(), device="cuda") for i in (0, 2)]  # the run's batches
    heads = [torch.cat(h) for h in zip(*parts)]
    for j, (got_p, want_p) in enumerate(zip(out["probabilities"], heads)):
        assert np.array_equal(got_p, want_p.cpu().numpy()), j
    want = eng.model.postproc_batch(*heads)
    assert len(want) == 3 and sum(len(t["info_dict"]["box"]) for t in want) > 0
    for i, item in enumerate(want):
        assert np.array_equal(out["predictions"][i], item["predictions"])
        for key in INSTANCE_KEYS:
            got_k, want_k = out[key][i], item["info_dict"][key]
            assert len(got_k) == len(want_k), (i, key)
            assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got_k, want_k)), (i, key)
    after = eng.run(tiles, patch_mode=True, return_probabilities=True, compute_dtype="float32")
    for a, b in zip(before["probabilities"], after["probabilities"]):  # the cache key separates the copies
        assert np.array_equal(a, b)
    assert np.array_equal(before["predictions"], after["predictions"])


KERNELS = {
    torch.float32: ("conv_mfma_f32_kernel", "grouped_conv_valid_kernel", "scale_shift_act_view_kernel", "upsample2x_add_kernel", "head1x1_kernel"),
    "half": ("conv_mfma_f32_kernel", "conv_mfma_h_kernel", "grouped_conv_valid_h_kernel", "scale_shift_act_view_h_kernel",
             "upsample2x_add_h_kernel", "head1x1_h_kernel"),
}
BANNED = ("igemm", "naive_conv", "SubTensorOp", "ck::", "miopen", "MIOpen", "Im2Col", "gemm_conv", "grouped_conv_fwd")  # test_unet_half_gpu's


@pytest.mark.parametrize("dtype", [torch.float32, *R.HALVES], ids=["fp32", "fp16", "bf16"])
def test_engine_run_launches_the_hand_written_kernels_only(dtype):
    """float32 included: the stem (the thin form of ``conv_mfma_f32_kernel``, float32 arithmetic in every dtype), the MFMA convolutions,
    the grouped and view kernels, the up-sampling and the heads -- and no library convolution."""
    from torch.profiler import ProfilerActivity, profile

    eng, tiles = _engine(), _tiles()[:2]
    name = str(dtype).replace("torch.", "")
    eng.run(tiles, patch_mode=True, compute_dtype=name)  # builds the inference copy
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out = eng.run(tiles, patch_mode=True, return_probabilities=True, compute_dtype=name)
        torch.cuda.synchronize()
    assert all(np.isfinite(p).all() for p in out["probabilities"])
    names = {e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()}
    kernels = {n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()}
    for wanted in KERNELS[dtype if dtype == torch.float32 else "half"]:
        assert any(wanted in k for k in kernels), (wanted, kernels)
    offenders = {k for k in kernels if any(b in k for b in BANNED)}
    assert not offenders, offenders


def test_engine_wsi_mode_float16_completes():
    from tiatoolbox_amd.utils import synth
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    eng = _engine()
    slide = np.full((600, 700, 3), 245, np.uint8)
    slide[64:480, 96:600] = synth.g_he(1, 416, 504, seed=3)[0]
    reader = ArrayWSIReader(slide, mpp=0.25, power=40)
    with tempfile.TemporaryDirectory() as tmp:
        paths = eng.run([reader], patch_mode=False, return_probabilities=True, return_predictions=(True,), save_dir=Path(tmp) / "out",
                        compute_dtype="float16")
        assert list(paths) == [0] and paths[0].name == "0.npz"
        with np.load(paths[0], allow_pickle=True) as res:
            pred = res["predictions"]
            probs = [res[f"probabilities/{j}"] for j in range(3)]
    assert type(eng._inference_model(torch.float16)).__name__ == "FusedHoVerNet"  # noqa: SLF001
    assert pred.shape == (600, 700) and all(p.shape[:2] == (600, 700) and np.isfinite(p).all() for p in probs)

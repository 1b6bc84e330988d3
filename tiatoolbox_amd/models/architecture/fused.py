"""Inference-time graph surgery for the CNN backbones (eval mode only).

* ``fold_conv_bn``: BatchNorm folded into the preceding convolution (weights scaled, bias added), removing one full
  read+write of every activation tensor per BN layer.
* ``MfmaResNet``: float32 ResNet trunk on hand-written kernels only -- the stem (``csrc/stem_mfma.hip``: uint8 or float32
  patches -> conv7x7 + bias + ReLU + max-pool, one kernel) and every block convolution (``csrc/conv_mfma.hip``: implicit GEMM
  on the matrix cores with bias / residual / ReLU in the epilogue).
  In fp16 / bf16 the same module runs on ``tia_stem_conv7x7_pool_nhwc_h`` / ``tia_conv2d_nhwc_h`` (no library convolution).
  A float32 trunk in ``"winograd"`` mode given uint8 patches runs the stem on the bf16 matrix cores with exactly split weights
  (``split_stem_weights`` / ``tia_stem_conv7x7_pool_nhwc_u8x3``: float32 in, float32 accumulate).

State-dict compatibility is untouched: these are derived copies built from a loaded ``CNNModel`` (reference parameter
names), never the object that loads weights.  Every wrapper raises on tensors it cannot take (host tensors, wrong layout):
there is no silent torch fallback.
"""

from __future__ import annotations

import copy
import functools

import torch
import torch.nn.functional as F  # noqa: N812
from torch import nn
from torch.nn.utils.fusion import fuse_conv_bn_eval

from tiatoolbox_amd import logger
from tiatoolbox_amd.models.architecture.resnet import BasicBlock, Bottleneck


def fold_conv_bn(model: nn.Module) -> nn.Module:
    """Deep-copied eval model with every (Conv2d, BatchNorm2d) pair fused."""
    model = copy.deepcopy(model).eval()

    def visit(mod: nn.Module) -> None:
        prev_name, prev = None, None
        for name, child in list(mod.named_children()):
            if isinstance(child, nn.BatchNorm2d) and isinstance(prev, nn.Conv2d):
                setattr(mod, prev_name, fuse_conv_bn_eval(prev, child))
                setattr(mod, name, nn.Identity())
                prev_name, prev = None, None
                continue
            visit(child)
            prev_name, prev = name, child

    visit(model)
    return model


# ------------------------------------------------------------------------------------------------
# HIP epilogues: conv (MIOpen, no bias) -> one fused bias (+ residual) + ReLU pass (cnn_epilogue.hip)
# ------------------------------------------------------------------------------------------------
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _nhwc_ptr_ok(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last) and t.dtype in _DT


def _ptr(t: torch.Tensor | None) -> int:
    """The address the C entry points take for an optional tensor: 0 stands for "none"."""
    return t.data_ptr() if t is not None else 0


def _conv_out_shape(name: str, x: torch.Tensor, cout: int, residual: torch.Tensor | None, *, kernel: int, stride: int, pad_lo: int,
                    pad_hi: int) -> tuple[int, int, int, int]:
    """``(n, cout, ho, wo)`` of a dense convolution of ``x`` with ``pad_lo`` zero rows / columns in front and ``pad_hi`` behind, for the
    wrapper ``name``; a ``residual`` must be a channels-last CUDA tensor of ``x``'s dtype and exactly that shape."""
    n, _, h, w = x.shape
    shape = (n, cout, (h + pad_lo + pad_hi - kernel) // stride + 1, (w + pad_lo + pad_hi - kernel) // stride + 1)
    if residual is not None and not (_nhwc_ptr_ok(residual) and residual.dtype == x.dtype and residual.shape == shape):
        msg = (f"{name}: residual must be a channels-last CUDA tensor of the output's dtype and shape ({x.dtype}, {shape}); got "
               f"{residual.dtype}, {tuple(residual.shape)}.")
        raise ValueError(msg)
    return shape


def hip_bias_act_(x: torch.Tensor, bias: torch.Tensor, residual: torch.Tensor | None = None, *, relu: bool = True) -> torch.Tensor:
    """In place ``x = relu(x + bias[c] (+ residual))`` on an NCHW tensor stored channels-last."""
    from tiatoolbox_amd import _lib

    if not _nhwc_ptr_ok(x) or (residual is not None and not _nhwc_ptr_ok(residual)):
        msg = "hip_bias_act_ expects channels-last CUDA tensors (fp32/fp16/bf16)."
        raise ValueError(msg)
    n, c, h, w = x.shape
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_bias_act_nhwc(x.data_ptr(), bias.data_ptr(), _ptr(residual), n * h * w, c, _DT[x.dtype], int(relu),
                                           _lib.current_stream())
    _lib.check(rc, "tia_bias_act_nhwc")
    return x


def hip_bias_relu_maxpool(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``maxpool3x3/s2/p1(relu(x + bias))`` of a channels-last tensor, one pass."""
    from tiatoolbox_amd import _lib

    if not _nhwc_ptr_ok(x):
        msg = "hip_bias_relu_maxpool expects a channels-last CUDA tensor (fp32/fp16/bf16)."
        raise ValueError(msg)
    n, c, h, w = x.shape
    out = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_bias_relu_maxpool_nhwc(x.data_ptr(), bias.data_ptr(), n, h, w, c, _DT[x.dtype], out.data_ptr(),
                                                    _lib.current_stream())
    _lib.check(rc, "tia_bias_relu_maxpool_nhwc")
    return out


CAM_MAX_CHANNELS = 8192  # (cnn_cam.hip: at least one class of the weights per workgroup's LDS tile)


def hip_cam(feat: torch.Tensor, weight: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Class activation maps ``cam[n, k, y, x] = sum_c weight[k, c] * feat[n, c, y, x]`` (``models/engine/_cam.py``), float32
    ``[N, K, h, w]``, in one launch of ``tia_cam_nhwc_f32`` / ``tia_cam_nhwc_h``.  ``feat``: the NCHW view of a channels-last CUDA
    tensor, float32 / fp16 / bf16 (any other layout is copied to channels-last first); ``weight``: float32 ``[K, C]`` on the same
    device; ``out``: a contiguous float32 ``[N, K, h, w]`` tensor there to write into instead of a new one (the engines' buffer of a
    whole run).  ``C`` is a multiple of 64 up to 8192."""
    from tiatoolbox_amd import _lib

    if not (isinstance(feat, torch.Tensor) and isinstance(weight, torch.Tensor) and feat.is_cuda and weight.is_cuda):
        msg = "hip_cam expects CUDA tensors (there is no CPU fallback: models/engine/_cam.py has the torch form)."
        raise ValueError(msg)
    if feat.dim() != 4 or feat.dtype not in _DT:  # noqa: PLR2004
        msg = f"hip_cam expects a feature map [N, C, h, w] in float32, float16 or bfloat16; got {tuple(feat.shape)} {feat.dtype}."
        raise ValueError(msg)
    if weight.dtype != torch.float32 or weight.dim() != 2 or weight.device != feat.device:  # noqa: PLR2004
        msg = f"hip_cam expects float32 weights [K, C] on the feature map's device; got {tuple(weight.shape)} {weight.dtype} on {weight.device}."
        raise ValueError(msg)
    n, c, h, w = feat.shape
    k = weight.shape[0]
    if weight.shape[1] != c:
        msg = f"hip_cam: the feature map has {c} channels and the weights {weight.shape[1]}."
        raise ValueError(msg)
    if min(n, c, h, w, k) <= 0:
        msg = f"hip_cam: empty feature map {tuple(feat.shape)} or weights {tuple(weight.shape)}."
        raise ValueError(msg)
    if not feat.is_contiguous(memory_format=torch.channels_last):
        feat = feat.contiguous(memory_format=torch.channels_last)
    weight = weight.detach().contiguous()
    if out is None:
        out = torch.empty((n, k, h, w), dtype=torch.float32, device=feat.device)
    elif not (out.dtype == torch.float32 and out.device == feat.device and tuple(out.shape) == (n, k, h, w) and out.is_contiguous()):
        msg = f"hip_cam: `out` must be a contiguous float32 tensor {(n, k, h, w)} on {feat.device}; got {tuple(out.shape)} {out.dtype} on {out.device}."
        raise ValueError(msg)
    with torch.cuda.device(feat.device):
        if feat.dtype == torch.float32:
            name = "tia_cam_nhwc_f32"
            rc = _lib.load().tia_cam_nhwc_f32(feat.data_ptr(), weight.data_ptr(), out.data_ptr(), n, h * w, c, k, _lib.current_stream())
        else:
            name = "tia_cam_nhwc_h"
            rc = _lib.load().tia_cam_nhwc_h(feat.data_ptr(), weight.data_ptr(), out.data_ptr(), n, h * w, c, k, _DT[feat.dtype],
                                            _lib.current_stream())
    if rc == _lib.TIA_ESIZE:
        msg = (f"hip_cam: {name} takes channel counts that are multiples of 64 up to {CAM_MAX_CHANNELS} (and fewer than 2^31 patches "
               f"and h * w * K entries per patch); got C = {c}, N = {n}, h * w * K = {h * w * k}.")
        raise ValueError(msg)
    _lib.check(rc, name)
    return out


# ------------------------------------------------------------------------------------------------
# Hand-written MFMA convolutions (conv_mfma.hip): float32 implicit GEMM with the epilogue fused in
# ------------------------------------------------------------------------------------------------
def hip_conv2d(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None, *,
               kernel: int, stride: int, padding: int, relu: bool) -> torch.Tensor:
    """``relu(conv2d(x, w) + bias + residual)`` on a float32 channels-last CUDA tensor (``tia_conv2d_nhwc_f32``)."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_conv2d expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    cout = w_packed.shape[-1]
    shape = _conv_out_shape("hip_conv2d", x, cout, residual, kernel=kernel, stride=stride, pad_lo=padding, pad_hi=padding)
    y = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv2d_nhwc_f32(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), n, h, w, cin,
                                             cout, kernel, kernel, stride, padding, int(relu), _lib.current_stream())
    _lib.check(rc, "tia_conv2d_nhwc_f32")
    return y


def hip_conv2d_ex(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None, *,
                  kernel: int, stride: int, pad_lo: int, pad_hi: int, relu: bool) -> torch.Tensor:
    """Like :func:`hip_conv2d` with ``pad_lo`` zero rows / columns in front and ``pad_hi`` behind (``tia_conv2d_nhwc_f32_ex``):
    TensorFlow-style "same" padding of strided convolutions, and valid convolutions (0 / 0)."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_conv2d_ex expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    cout = w_packed.shape[-1]
    shape = _conv_out_shape("hip_conv2d_ex", x, cout, residual, kernel=kernel, stride=stride, pad_lo=pad_lo, pad_hi=pad_hi)
    y = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv2d_nhwc_f32_ex(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), n, h, w, cin,
                                                cout, kernel, kernel, stride, pad_lo, pad_lo, shape[2], shape[3], int(relu),
                                                _lib.current_stream())
    _lib.check(rc, "tia_conv2d_nhwc_f32_ex")
    return y


def pack_thin_conv_weights(weight: torch.Tensor) -> torch.Tensor:
    """OIHW ``[cout, c, kh, kw]`` with ``c * kw <= 32`` -> ``[kh][32][cout]`` (row ``kx * c + ch``; zero rows behind): the
    row-packed form :func:`hip_conv2d_thin` multiplies with."""
    cout, c, kh, kw = weight.shape
    if c * kw > 32 or cout % 64 != 0:  # noqa: PLR2004
        msg = f"thin-input convolution needs c * kw <= 32 and cout % 64 == 0; got weight {tuple(weight.shape)}."
        raise ValueError(msg)
    rows = weight.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(kh, kw * c, cout)
    packed = torch.zeros((kh, 32, cout), dtype=torch.float32, device=weight.device)
    packed[:, :kw * c] = rows
    return packed.contiguous()


def hip_conv2d_thin(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, *, kernel: int, stride: int, pad_lo: int,
                    pad_hi: int, relu: bool, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Convolution of a few-channel image (``c * kernel <= 32``: HoVer-Net's RGB 7x7 stem) on the MFMA kernel
    (``tia_conv2d_thin_nhwc_f32``): the ``kernel * c`` values under a row of taps are contiguous in NHWC, so they are read
    as one 32-wide slice.  ``x``: float32 channels-last ``[n, c, h, w]``; the horizontal padding (``pad_lo`` / ``pad_hi`` zero
    columns, plus the few that keep the last slice inside its row) is materialised here, the vertical one is the kernel's.
    ``out_dtype`` fp16 / bf16 (``tia_conv2d_thin_nhwc``): the same float32 arithmetic on float32 inputs, weights and bias, the
    result rounded once on the way out -- the stem of the half-precision HoVer-Net."""
    from tiatoolbox_amd import _lib

    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):  # noqa: PLR2004
        msg = "hip_conv2d_thin expects a float32 CUDA tensor [n, c, h, w]."
        raise ValueError(msg)
    if out_dtype not in _DT or w_packed.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        msg = (f"hip_conv2d_thin computes in float32 (float32 packed weights and bias) and returns float32 / fp16 / bf16; got weights "
               f"{w_packed.dtype}, bias {bias.dtype if bias is not None else None}, out_dtype {out_dtype}.")
        raise ValueError(msg)
    n, c, h, w = x.shape
    cout = w_packed.shape[-1]
    ho = (h + pad_lo + pad_hi - kernel) // stride + 1
    wo = (w + pad_lo + pad_hi - kernel) // stride + 1
    need = (wo - 1) * stride + -(-32 // c)  # columns the last output's 32-float read covers
    extra = max(need - (w + pad_lo + pad_hi), 0)
    rows = x.permute(0, 2, 3, 1)  # NHWC
    wp = w + pad_lo + pad_hi + extra
    xp = torch.zeros((n, h, wp, c), dtype=torch.float32, device=x.device)
    xp[:, :, pad_lo:pad_lo + w] = rows
    y = torch.empty((n, cout, ho, wo), dtype=out_dtype, device=x.device, memory_format=torch.channels_last)
    name = "tia_conv2d_thin_nhwc_f32" if out_dtype == torch.float32 else "tia_conv2d_thin_nhwc"
    args = (n, h, wp, c, cout, kernel, kernel, stride, pad_lo, ho, wo, int(relu), _lib.current_stream())
    with torch.cuda.device(x.device):
        if out_dtype == torch.float32:
            rc = _lib.load().tia_conv2d_thin_nhwc_f32(xp.data_ptr(), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), *args)
        else:
            rc = _lib.load().tia_conv2d_thin_nhwc(xp.data_ptr(), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), _DT[out_dtype], *args)
    _lib.check(rc, name)
    return y


def hip_conv1x1_head(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, *, pre_scale: torch.Tensor | None = None,
                     pre_shift: torch.Tensor | None = None) -> torch.Tensor:
    """A class head: 1x1 convolution ``64 -> cout <= 8`` (``tia_conv1x1_head_nhwc_f32``; fp16 / bf16 ``x``:
    ``tia_conv1x1_head_nhwc_h``), optionally of ``relu(x * pre_scale[c] + pre_shift[c])`` (the BatchNorm + ReLU in front of
    HoVer-Net's ``u0/conv``) without writing that intermediate.  ``x``: channels-last ``[n, 64, h, w]``; ``weight``: ``[cout, 64]``
    (or OIHW 1x1).  Weights, bias and ``pre_*`` are float32 whatever ``x`` is, and so are the returned logits."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.shape[1] == 64):  # noqa: PLR2004
        msg = "hip_conv1x1_head expects a float32 / fp16 / bf16 channels-last CUDA tensor with 64 channels."
        raise ValueError(msg)
    half = x.dtype != torch.float32
    if half and any(t is not None and t.dtype != torch.float32 for t in (weight, bias, pre_scale, pre_shift)):
        msg = f"hip_conv1x1_head takes weight, bias and pre_scale / pre_shift in float32 beside a {x.dtype} input."
        raise ValueError(msg)
    n, _, h, w = x.shape
    cout = weight.shape[0]
    wmat = weight.detach().reshape(cout, 64).to(torch.float32).contiguous()
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    ptrs = (wmat.data_ptr(), _ptr(bias), _ptr(pre_scale), _ptr(pre_shift))
    name = "tia_conv1x1_head_nhwc_h" if half else "tia_conv1x1_head_nhwc_f32"
    with torch.cuda.device(x.device):
        if half:
            rc = _lib.load().tia_conv1x1_head_nhwc_h(x.data_ptr(), n * h * w, *ptrs, cout, _DT[x.dtype], y.data_ptr(), _lib.current_stream())
        else:
            rc = _lib.load().tia_conv1x1_head_nhwc_f32(x.data_ptr(), n * h * w, *ptrs, cout, y.data_ptr(), _lib.current_stream())
    _lib.check(rc, name)
    return y


def hip_conv2d_post(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None, *,
                    kernel: int, stride: int, pad_lo: int, pad_hi: int, relu: bool, post_scale: torch.Tensor,
                    post_shift: torch.Tensor, want_raw: bool = True) -> tuple[torch.Tensor | None, torch.Tensor]:
    """:func:`hip_conv2d_ex` plus ``relu(v * post_scale[c] + post_shift[c])`` of its result ``v`` from the same epilogue
    (``tia_conv2d_post_nhwc_f32``); returns ``(v or None, activated)``."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_conv2d_post expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    cout = w_packed.shape[-1]
    shape = _conv_out_shape("hip_conv2d_post", x, cout, residual, kernel=kernel, stride=stride, pad_lo=pad_lo, pad_hi=pad_hi)
    y = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last) if want_raw else None
    y2 = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv2d_post_nhwc_f32(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), _ptr(y), n, h, w, cin,
                                                  cout, kernel, kernel, stride, pad_lo, pad_lo, shape[2], shape[3], int(relu),
                                                  post_scale.data_ptr(), post_shift.data_ptr(), y2.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_conv2d_post_nhwc_f32")
    return y, y2


def hip_conv1x1_pre(x: torch.Tensor, pre_scale: torch.Tensor, pre_shift: torch.Tensor, w_packed: torch.Tensor,
                    bias: torch.Tensor | None, residual: torch.Tensor | None = None, *, stride: int = 1,
                    relu: bool = False) -> torch.Tensor:
    """``act(conv1x1(relu(x * pre_scale[c] + pre_shift[c])) + bias [+ residual])`` with the activation applied on load
    (``tia_conv1x1_pre_nhwc_f32``): the pre-activation in front of a residual unit without an activated copy in memory."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_conv1x1_pre expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    cout = w_packed.shape[-1]
    shape = _conv_out_shape("hip_conv1x1_pre", x, cout, residual, kernel=1, stride=stride, pad_lo=0, pad_hi=0)
    y = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv1x1_pre_nhwc_f32(x.data_ptr(), pre_scale.data_ptr(), pre_shift.data_ptr(), w_packed.data_ptr(),
                                                  _ptr(bias), _ptr(residual), y.data_ptr(), n, h, w, cin, cout, stride, int(relu),
                                                  _lib.current_stream())
    _lib.check(rc, "tia_conv1x1_pre_nhwc_f32")
    return y


def hip_scale_shift_act(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, *, relu: bool = True,
                        inplace: bool = False) -> torch.Tensor:
    """``relu(x * scale[c] + shift[c])`` on a float32 channels-last CUDA tensor (``tia_scale_shift_act_nhwc_f32``)."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_scale_shift_act expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    n, c, h, w = x.shape
    y = x if inplace else torch.empty_like(x, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_scale_shift_act_nhwc_f32(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), n * h * w, c,
                                                      int(relu), _lib.current_stream())
    _lib.check(rc, "tia_scale_shift_act_nhwc_f32")
    return y


def hip_scale_shift_act_view(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, *, relu: bool = True) -> torch.Tensor:
    """``relu(x * scale[c] + shift[c])`` of a channel-prefix / spatial-window VIEW of a channels-last CUDA tensor, written to a
    dense channels-last tensor (``tia_scale_shift_act_view_nhwc_f32``; an fp16 / bf16 ``x``: ``tia_scale_shift_act_view_nhwc_h``,
    float32 ``scale`` / ``shift`` and arithmetic, one rounding)."""
    from tiatoolbox_amd import _lib

    if not x.is_cuda:
        msg = "hip_scale_shift_act_view expects a CUDA tensor."
        raise ValueError(msg)
    n, c, h, w = x.shape
    half = x.dtype in (torch.float16, torch.bfloat16)
    vec = 8 if half else 4  # elements per 16-byte access
    ok = (x.dtype in _DT and x.stride(1) == 1 and c % vec == 0 and x.data_ptr() % 16 == 0
          and all(x.stride(d) % vec == 0 for d in (0, 2, 3)) and x.stride(3) >= c)
    if not ok:
        msg = ("hip_scale_shift_act_view expects a float32 / fp16 / bf16 view with contiguous channels, c % 4 == 0 (fp16 / bf16: c % 8 "
               "== 0), a 16-byte aligned base and strides that are multiples of 4 (8) elements; "
               f"got shape {tuple(x.shape)} strides {tuple(x.stride())} {x.dtype}.")
        raise ValueError(msg)
    if any(not t.is_cuda or t.dtype != torch.float32 for t in (scale, shift)):
        msg = f"hip_scale_shift_act_view takes scale / shift as float32 CUDA tensors; got {scale.dtype} / {shift.dtype} on {scale.device}."
        raise ValueError(msg)
    y = torch.empty((n, c, h, w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    args = (x.data_ptr(), x.stride(0), x.stride(2), x.stride(3), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), n, h, w, c, int(relu))
    name = "tia_scale_shift_act_view_nhwc_h" if half else "tia_scale_shift_act_view_nhwc_f32"
    with torch.cuda.device(x.device):
        if half:
            rc = _lib.load().tia_scale_shift_act_view_nhwc_h(*args, _DT[x.dtype], _lib.current_stream())
        else:
            rc = _lib.load().tia_scale_shift_act_view_nhwc_f32(*args, _lib.current_stream())
    _lib.check(rc, name)
    return y


def hip_grouped_conv_valid(x: torch.Tensor, w_packed: torch.Tensor, *, groups: int, kernel: int,
                           out: torch.Tensor | None = None) -> torch.Tensor:
    """Grouped valid ``kernel x kernel`` convolution, 32 -> 8 channels per group (``tia_grouped_conv_valid_nhwc_f32``); ``out``
    may be a channel slice / window view of a wider channels-last buffer.  ``w_packed``: ``[groups, k, k, 32, 8]``."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_grouped_conv_valid expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    ho, wo = h - kernel + 1, w - kernel + 1
    if out is None:
        out = torch.empty((n, groups * 8, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    if (out.shape != (n, groups * 8, ho, wo) or out.stride(1) != 1 or out.dtype != torch.float32 or out.data_ptr() % 16
            or any(out.stride(d) % 4 for d in (0, 2, 3))):
        msg = "hip_grouped_conv_valid: `out` must be a float32 channels-last (view of a) tensor of the output shape."
        raise ValueError(msg)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_grouped_conv_valid_nhwc_f32(x.data_ptr(), w_packed.data_ptr(), out.data_ptr(), out.stride(0),
                                                         out.stride(2), out.stride(3), n, h, w, groups, cin // groups, 8, kernel,
                                                         _lib.current_stream())
    _lib.check(rc, "tia_grouped_conv_valid_nhwc_f32")
    return out


def pack_grouped_conv_valid_weights_h(weight: torch.Tensor, groups: int, dtype: torch.dtype) -> torch.Tensor:
    """Grouped OIHW float32 ``[groups * 8, 32, k, k]`` -> ``[groups, k, k, 4, 8, 8]`` halves of ``dtype`` (8-channel chunk, output,
    channel within the chunk), rounded once: the operand layout of :func:`hip_grouped_conv_valid_h`
    (``tia_grouped_conv_pack_weights_h``)."""
    from tiatoolbox_amd import _lib

    w = weight.detach()
    if (not w.is_cuda or w.dtype != torch.float32 or dtype not in (torch.float16, torch.bfloat16) or w.dim() != 4  # noqa: PLR2004
            or w.shape[0] != groups * 8 or w.shape[1] != 32 or w.shape[2] != w.shape[3]):  # noqa: PLR2004
        msg = (f"pack_grouped_conv_valid_weights_h packs a float32 CUDA weight [groups * 8, 32, k, k] for fp16 / bf16; got "
               f"{tuple(w.shape)} {w.dtype} on {w.device}, groups {groups}, {dtype}.")
        raise ValueError(msg)
    w = w.contiguous()
    k = w.shape[2]
    out = torch.empty((groups, k, k, 4, 8, 8), dtype=dtype, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_grouped_conv_pack_weights_h(w.data_ptr(), groups, k, _DT[dtype], out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_grouped_conv_pack_weights_h")
    return out


def hip_grouped_conv_valid_h(x: torch.Tensor, w_packed: torch.Tensor, *, groups: int, kernel: int,
                             out: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`hip_grouped_conv_valid` on fp16 / bf16 activations (``tia_grouped_conv_valid_nhwc_h``: the 16x16x32 MFMA, float32
    accumulation, one rounding); ``w_packed`` from :func:`pack_grouped_conv_valid_weights_h` in ``x``'s dtype; ``out`` may be a
    channel slice / window view of a wider channels-last buffer of that dtype."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype in (torch.float16, torch.bfloat16)):
        msg = "hip_grouped_conv_valid_h expects an fp16 / bf16 channels-last CUDA tensor."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    if (w_packed.dtype != x.dtype or tuple(w_packed.shape) != (groups, kernel, kernel, 4, 8, 8) or not w_packed.is_contiguous()
            or w_packed.device != x.device):
        msg = (f"hip_grouped_conv_valid_h: packed weights {tuple(w_packed.shape)} {w_packed.dtype} on {w_packed.device} do not match "
               f"{groups} groups, kernel {kernel}, {x.dtype} on {x.device} (expected pack_grouped_conv_valid_weights_h's layout).")
        raise ValueError(msg)
    ho, wo = h - kernel + 1, w - kernel + 1
    if out is None:
        out = torch.empty((n, groups * 8, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if (out.shape != (n, groups * 8, ho, wo) or out.stride(1) != 1 or out.dtype != x.dtype or not out.is_cuda or out.data_ptr() % 16
            or any(out.stride(d) % 8 for d in (0, 2, 3))):
        msg = (f"hip_grouped_conv_valid_h: `out` must be a channels-last (view of a) {x.dtype} CUDA tensor of the output shape on a "
               "16-byte aligned base with strides that are multiples of 8 elements.")
        raise ValueError(msg)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_grouped_conv_valid_nhwc_h(x.data_ptr(), w_packed.data_ptr(), out.data_ptr(), out.stride(0), out.stride(2),
                                                       out.stride(3), n, h, w, groups, cin // groups, 8, kernel, _DT[x.dtype],
                                                       _lib.current_stream())
    _lib.check(rc, "tia_grouped_conv_valid_nhwc_h")
    return out


def pack_grouped_conv_weights(conv: nn.Conv2d) -> torch.Tensor:
    """Grouped OIHW 3x3 ``[groups * cg, cg, 3, 3]`` -> ``[groups, 3, 3, cg (input), cg (output)]`` float32, the layout of
    ``tia_conv3x3_grouped_nhwc_f32`` (a group's weights of one tap and input channel are contiguous over its outputs)."""
    w = conv.weight.detach().to(torch.float32)
    cout, cg, kh, kw = w.shape
    groups = conv.groups
    if (kh, kw) != (3, 3) or cout != groups * cg or conv.in_channels != cout or cg not in (4, 8, 16, 32, 64):  # noqa: PLR2004
        msg = f"the grouped 3x3 kernel takes cin == cout, 4 to 64 channels per group; got weight {tuple(w.shape)}, groups {groups}."
        raise ValueError(msg)
    return w.reshape(groups, cg, cg, 3, 3).permute(0, 3, 4, 2, 1).contiguous()


def hip_conv3x3_grouped(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, *, stride: int,
                        relu: bool) -> torch.Tensor:
    """``relu(conv3x3(x, w, groups, stride, padding=1) + bias)`` on a float32 channels-last CUDA tensor
    (``tia_conv3x3_grouped_nhwc_f32``, the ResNeXt conv2); ``w_packed`` from :func:`pack_grouped_conv_weights`."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_conv3x3_grouped expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    n, c, h, w = x.shape
    groups, cg = w_packed.shape[0], w_packed.shape[-1]
    if (tuple(w_packed.shape) != (groups, 3, 3, cg, cg) or groups * cg != c or w_packed.dtype != torch.float32
            or not w_packed.is_contiguous() or w_packed.device != x.device):
        msg = (f"hip_conv3x3_grouped: packed weights {tuple(w_packed.shape)} {w_packed.dtype} on {w_packed.device} do not match an "
               f"input with {c} channels on {x.device} (expected pack_grouped_conv_weights' [groups, 3, 3, cg, cg] float32).")
        raise ValueError(msg)
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.numel() == c and bias.is_contiguous()):
        msg = "hip_conv3x3_grouped takes a contiguous float32 CUDA bias of one value per channel."
        raise ValueError(msg)
    y = torch.empty((n, c, (h - 1) // stride + 1, (w - 1) // stride + 1), dtype=torch.float32, device=x.device,
                    memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv3x3_grouped_nhwc_f32(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), y.data_ptr(), n, h, w, groups, cg, stride,
                                                      int(relu), _lib.current_stream())
    _lib.check(rc, "tia_conv3x3_grouped_nhwc_f32")
    return y


def hip_upsample2x_add(x: torch.Tensor, y: torch.Tensor, scale: torch.Tensor | None = None,
                       shift: torch.Tensor | None = None) -> torch.Tensor:
    """``x.repeat_interleave(2, 2).repeat_interleave(2, 3) + y`` in one pass (``tia_upsample2x_add_act_nhwc_f32``; fp16 / bf16
    ``x`` and ``y``: ``tia_upsample2x_add_act_nhwc_h``, float32 arithmetic and one rounding); ``y`` may be a centre-cropped view
    of a channels-last tensor.  With ``scale`` / ``shift`` (float32): followed by ``relu(. * scale + shift)``."""
    from tiatoolbox_amd import _lib

    if not (x.is_cuda and y.is_cuda):
        msg = "hip_upsample2x_add expects CUDA tensors."
        raise ValueError(msg)
    n, c, h, w = x.shape
    half = x.dtype in (torch.float16, torch.bfloat16)
    vec = 8 if half else 4  # elements per 16-byte access
    ok_y = (y.is_cuda and y.dtype == x.dtype and y.shape == (n, c, 2 * h, 2 * w) and y.stride(1) == 1 and y.stride(3) == c
            and y.stride(2) % vec == 0 and y.stride(0) % vec == 0 and y.data_ptr() % 16 == 0)
    if not (_nhwc_ptr_ok(x) and ok_y and c % vec == 0):
        msg = ("hip_upsample2x_add expects channels-last tensors of one dtype (float32: c % 4 == 0; fp16 / bf16: c % 8 == 0), `y` a "
               "(cropped) view with contiguous channels of shape [n, c, 2h, 2w] on a 16-byte aligned base and strides; "
               f"got x {tuple(x.shape)} {x.dtype}, y {tuple(y.shape)} {y.dtype} strides {tuple(y.stride())}.")
        raise ValueError(msg)
    if half and any(t is not None and t.dtype != torch.float32 for t in (scale, shift)):
        msg = f"hip_upsample2x_add takes scale / shift in float32 beside {x.dtype} tensors."
        raise ValueError(msg)
    out = torch.empty((n, c, 2 * h, 2 * w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    args = (x.data_ptr(), y.data_ptr(), y.stride(0), y.stride(2), _ptr(scale), _ptr(shift), out.data_ptr(), n, h, w, c)
    name = "tia_upsample2x_add_act_nhwc_h" if half else "tia_upsample2x_add_act_nhwc_f32"
    with torch.cuda.device(x.device):
        if half:
            rc = _lib.load().tia_upsample2x_add_act_nhwc_h(*args, _DT[x.dtype], _lib.current_stream())
        else:
            rc = _lib.load().tia_upsample2x_add_act_nhwc_f32(*args, _lib.current_stream())
    _lib.check(rc, name)
    return out


def hip_avgpool2x2(x: torch.Tensor) -> torch.Tensor:
    """``F.avg_pool2d(x, 2, 2)`` in one pass (``tia_avgpool2x2_nhwc_f32``; fp16 / bf16 ``x``: ``tia_avgpool2x2_nhwc_h``, float32
    arithmetic and one rounding): the sums in torch's order, ``((x00 + x01) + x10) + x11``, times 0.25; a last odd row or column
    is dropped."""
    from tiatoolbox_amd import _lib

    if not x.is_cuda:
        msg = "hip_avgpool2x2 expects a CUDA tensor."
        raise ValueError(msg)
    half = x.dtype in (torch.float16, torch.bfloat16)
    vec = 8 if half else 4  # elements per 16-byte access
    if not (_nhwc_ptr_ok(x) and x.shape[1] % vec == 0 and x.shape[2] >= 2 and x.shape[3] >= 2 and x.data_ptr() % 16 == 0):  # noqa: PLR2004
        msg = ("hip_avgpool2x2 expects a channels-last tensor [n, c, h, w] with h >= 2, w >= 2 (float32: c % 4 == 0; fp16 / bf16: "
               f"c % 8 == 0) on a 16-byte aligned base; got x {tuple(x.shape)} {x.dtype} strides {tuple(x.stride())}.")
        raise ValueError(msg)
    n, c, h, w = x.shape
    out = torch.empty((n, c, h // 2, w // 2), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    name = "tia_avgpool2x2_nhwc_h" if half else "tia_avgpool2x2_nhwc_f32"
    with torch.cuda.device(x.device):
        if half:
            rc = _lib.load().tia_avgpool2x2_nhwc_h(x.data_ptr(), out.data_ptr(), n, h, w, c, _DT[x.dtype], _lib.current_stream())
        else:
            rc = _lib.load().tia_avgpool2x2_nhwc_f32(x.data_ptr(), out.data_ptr(), n, h, w, c, _lib.current_stream())
    _lib.check(rc, name)
    return out


def hip_upsample2x_concat(x: torch.Tensor, y: torch.Tensor, scale: torch.Tensor | None = None,
                          shift: torch.Tensor | None = None) -> torch.Tensor:
    """``torch.cat([x.repeat_interleave(2, 2).repeat_interleave(2, 3), y], 1)`` in one pass (``tia_upsample2x_concat_act_nhwc_f32``;
    fp16 / bf16 ``x`` and ``y``: ``tia_upsample2x_concat_act_nhwc_h``): a pure copy, bit for bit.  With ``scale`` / ``shift``
    (float32, ``cx + cy`` channels): followed by ``relu(. * scale + shift)``, product and sum rounded separately in float32 and --
    for halves -- one rounding at the end."""
    from tiatoolbox_amd import _lib

    if not (x.is_cuda and y.is_cuda):
        msg = "hip_upsample2x_concat expects CUDA tensors."
        raise ValueError(msg)
    half = x.dtype in (torch.float16, torch.bfloat16)
    vec = 8 if half else 4  # elements per 16-byte access
    ok = (_nhwc_ptr_ok(x) and _nhwc_ptr_ok(y) and y.dtype == x.dtype and y.shape[0] == x.shape[0]
          and tuple(y.shape[2:]) == (2 * x.shape[2], 2 * x.shape[3]) and x.shape[1] % vec == 0 and y.shape[1] % vec == 0
          and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)
    if not ok:
        msg = ("hip_upsample2x_concat expects channels-last tensors of one dtype, x [n, cx, h, w] and y [n, cy, 2h, 2w] (float32: "
               "cx % 4 == 0 and cy % 4 == 0; fp16 / bf16: cx % 8 == 0 and cy % 8 == 0), dense on 16-byte aligned bases; "
               f"got x {tuple(x.shape)} {x.dtype} strides {tuple(x.stride())}, y {tuple(y.shape)} {y.dtype} strides {tuple(y.stride())}.")
        raise ValueError(msg)
    n, cx, h, w = x.shape
    cy = y.shape[1]
    if (scale is None) != (shift is None) or any(
            t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.shape == (cx + cy,) and t.is_contiguous())
            for t in (scale, shift)):
        msg = (f"hip_upsample2x_concat takes scale / shift in float32 ([cx + cy] = [{cx + cy}] each, both or neither) beside {x.dtype} "
               f"tensors; got {None if scale is None else (tuple(scale.shape), scale.dtype)}, "
               f"{None if shift is None else (tuple(shift.shape), shift.dtype)}.")
        raise ValueError(msg)
    out = torch.empty((n, cx + cy, 2 * h, 2 * w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    args = (x.data_ptr(), y.data_ptr(), _ptr(scale), _ptr(shift), out.data_ptr(), n, h, w, cx, cy)
    name = "tia_upsample2x_concat_act_nhwc_h" if half else "tia_upsample2x_concat_act_nhwc_f32"
    with torch.cuda.device(x.device):
        if half:
            rc = _lib.load().tia_upsample2x_concat_act_nhwc_h(*args, _DT[x.dtype], _lib.current_stream())
        else:
            rc = _lib.load().tia_upsample2x_concat_act_nhwc_f32(*args, _lib.current_stream())
    _lib.check(rc, name)
    return out


def hip_conv2d_h(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None, *,
                 cout: int, kernel: int, stride: int, padding: int, relu: bool) -> torch.Tensor:
    """``relu(conv2d(x, w) + bias + residual)`` on an fp16 / bf16 channels-last CUDA tensor (``tia_conv2d_nhwc_h``: MFMA with
    float32 accumulation; ``bias`` float32; one rounding to half at the end)."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype in (torch.float16, torch.bfloat16)):
        msg = "hip_conv2d_h expects an fp16 / bf16 channels-last CUDA tensor."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    shape = _conv_out_shape("hip_conv2d_h", x, cout, residual, kernel=kernel, stride=stride, pad_lo=padding, pad_hi=padding)
    if bias is not None and bias.dtype != torch.float32:
        msg = "hip_conv2d_h takes the bias in float32."
        raise ValueError(msg)
    y = torch.empty(shape, dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv2d_nhwc_h(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), n, h, w, cin, cout,
                                           kernel, kernel, stride, padding, _DT[x.dtype], int(relu), _lib.current_stream())
    _lib.check(rc, "tia_conv2d_nhwc_h")
    return y


def hip_conv2d_h_ex(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None, *, cout: int,
                    kernel: int, stride: int, pad_lo: int, pad_hi: int, relu: bool, post_scale: torch.Tensor | None = None,
                    post_shift: torch.Tensor | None = None, want_raw: bool = True):
    """:func:`hip_conv2d_h` with ``pad_lo`` zero rows / columns in front and ``pad_hi`` behind (``tia_conv2d_nhwc_h_ex``) and, with
    ``post_scale`` / ``post_shift`` (float32), a second output ``relu(v * post_scale[c] + post_shift[c])`` of the float32 result
    ``v`` BEFORE its rounding.  Returns ``y``, or ``(y or None, activated)`` with a second output (``want_raw=False``: no ``y``)."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype in (torch.float16, torch.bfloat16)):
        msg = "hip_conv2d_h_ex expects an fp16 / bf16 channels-last CUDA tensor."
        raise ValueError(msg)
    with_post = post_scale is not None or post_shift is not None
    if any(t is not None and (t.dtype != torch.float32 or not t.is_cuda) for t in (bias, post_scale, post_shift)) or (
            with_post and (post_scale is None or post_shift is None)):
        msg = "hip_conv2d_h_ex takes the bias and post_scale / post_shift (both or neither) as float32 CUDA tensors."
        raise ValueError(msg)
    if w_packed.dtype != x.dtype:
        msg = f"hip_conv2d_h_ex: weights packed for {w_packed.dtype} beside a {x.dtype} input."
        raise ValueError(msg)
    if not with_post and not want_raw:
        msg = "hip_conv2d_h_ex: want_raw=False needs a second output."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    shape = _conv_out_shape("hip_conv2d_h_ex", x, cout, residual, kernel=kernel, stride=stride, pad_lo=pad_lo, pad_hi=pad_hi)
    y = torch.empty(shape, dtype=x.dtype, device=x.device, memory_format=torch.channels_last) if want_raw else None
    y2 = torch.empty(shape, dtype=x.dtype, device=x.device, memory_format=torch.channels_last) if with_post else None
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv2d_nhwc_h_ex(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), _ptr(y), n, h, w, cin, cout,
                                              kernel, kernel, stride, pad_lo, pad_lo, shape[2], shape[3], _DT[x.dtype], int(relu),
                                              _ptr(post_scale), _ptr(post_shift), _ptr(y2), _lib.current_stream())
    _lib.check(rc, "tia_conv2d_nhwc_h_ex")
    return (y, y2) if with_post else y


def pack_conv_weights_h(conv: nn.Conv2d, dtype: torch.dtype) -> torch.Tensor:
    """OIHW -> ``[kh, kw, cin/8, cout, 8]`` halves of ``dtype`` on the convolution's device (``tia_conv_pack_weights_h``)."""
    from tiatoolbox_amd import _lib

    w = conv.weight.detach().to(torch.float32).contiguous()
    cout, cin, kh, kw = w.shape
    if not w.is_cuda or dtype not in (torch.float16, torch.bfloat16):
        msg = f"pack_conv_weights_h packs CUDA weights for fp16 / bf16; got weights on {w.device} for {dtype}."
        raise ValueError(msg)
    out = torch.empty((kh, kw, cin // 8, cout, 8), dtype=dtype, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_conv_pack_weights_h(w.data_ptr(), cout, cin, kh, kw, _DT[dtype], out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_conv_pack_weights_h")
    return out


def pack_conv_weights(conv: nn.Conv2d) -> torch.Tensor:
    """OIHW -> ``[kh, kw, cin, cout]`` float32 on the convolution's device (``tia_conv_pack_weights_f32``)."""
    from tiatoolbox_amd import _lib

    w = conv.weight.detach().to(torch.float32).contiguous()
    cout, cin, kh, kw = w.shape
    out = torch.empty((kh, kw, cin, cout), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_conv_pack_weights_f32(w.data_ptr(), cout, cin, kh, kw, out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_conv_pack_weights_f32")
    return out


def _pack_conv_weights_wino(conv: nn.Conv2d, positions: int, entry: str, form: str) -> torch.Tensor:
    """The Winograd-domain weights of a 3x3 convolution, ``[positions, cin/16, 2, cout/64, 2, 64, 4]``, packed by `entry`."""
    from tiatoolbox_amd import _lib

    w = conv.weight.detach().to(torch.float32).contiguous()
    cout, cin, kh, kw = w.shape
    if (kh, kw) != (3, 3) or cin % 16 or cout % 64:
        msg = f"Winograd {form} needs a 3x3 kernel, cin % 16 == 0 and cout % 64 == 0; got weight {tuple(w.shape)}."
        raise ValueError(msg)
    out = torch.empty((positions, cin // 16, 2, cout // 64, 2, 64, 4), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = getattr(_lib.load(), entry)(w.data_ptr(), cout, cin, out.data_ptr(), _lib.current_stream())
    _lib.check(rc, entry)
    return out


def pack_conv_weights_wino(conv: nn.Conv2d) -> torch.Tensor:
    """OIHW 3x3 float32 -> the Winograd-domain weights ``U = G g G^T`` in the stage layout of ``tia_conv3x3_wino_nhwc_f32``
    (``tia_conv_pack_weights_wino_f32``: float64 transform, one rounding), ``[16, cin/16, 2, cout/64, 2, 64, 4]``
    (position, 16-channel slice, 8-channel half, 64-column block, 4-channel group, column, channel)."""
    return _pack_conv_weights_wino(conv, 16, "tia_conv_pack_weights_wino_f32", "F(2x2, 3x3)")


def pack_conv_weights_wino42(conv: nn.Conv2d) -> torch.Tensor:
    """OIHW 3x3 float32 -> the F(4x2, 3x3) Winograd-domain weights ``U = G4 g G2^T`` in the stage layout of
    ``tia_conv3x3_wino42_nhwc_f32`` (``tia_conv_pack_weights_wino42_f32``: float64 transform, one rounding),
    ``[24, cin/16, 2, cout/64, 2, 64, 4]`` (position 4 i + j, then as :func:`pack_conv_weights_wino`)."""
    return _pack_conv_weights_wino(conv, 24, "tia_conv_pack_weights_wino42_f32", "F(4x2, 3x3)")


def wino_weights_f32(weight: torch.Tensor) -> torch.Tensor:
    """OIHW 3x3 weights -> ``U = G g G^T`` as ``[cout, cin, 4, 4]`` float32: transformed in float64 in the operation order of
    ``tia_conv_pack_weights_wino_f32`` and rounded once, so the values are bit for bit that packing's.  Device-agnostic."""
    g = weight.detach().to(torch.float64)

    def rows(t: torch.Tensor, dim: int) -> torch.Tensor:  # G t along `dim` (G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1])
        t0, t1, t2 = t.unbind(dim)
        return torch.stack((t0, 0.5 * (t0 + t1 + t2), 0.5 * (t0 - t1 + t2), t2), dim)

    return rows(rows(g, 2), 3).to(torch.float32)


def pack_conv_weights_wino_split(conv: nn.Conv2d) -> torch.Tensor | None:
    """OIHW 3x3 float32 -> the three bf16 planes of the Winograd-domain weights in the stage layout of
    ``tia_conv3x3_wino_bf16x3_nhwc_f32``, ``[cin/16, 2, cout/64, 8, 3, 2, 64, 8]`` bf16 (slice, column pair of the position grid,
    64-column block, position ``2 i + jl``, plane, k-chunk, column, channel): ``U`` from :func:`wino_weights_f32` (what the float32
    form multiplies by), split by :func:`split_stem_weights`, laid out by ``tia_conv_pack_weights_wino_bf16x3``.  ``None`` when ``U``
    has no usable exact split (one ``info`` line): the layer then keeps the float32 Winograd form."""
    from tiatoolbox_amd import _lib

    w = conv.weight.detach().to(torch.float32).contiguous()
    cout, cin, kh, kw = w.shape
    if (kh, kw) != (3, 3) or cin % 16 or cout % 64 or conv.groups != 1:
        msg = f"the split Winograd form needs a 3x3 kernel, cin % 16 == 0, cout % 64 == 0 and groups == 1; got weight {tuple(w.shape)}."
        raise ValueError(msg)
    parts, usable = split_stem_weights(wino_weights_f32(w))
    if not usable:
        logger.info("a %s convolution's Winograd-domain weights have no exact three-part bf16 split (non-finite or extreme "
                    "exponents); the layer keeps the float32 Winograd form.", tuple(w.shape))
        return None
    parts = parts.contiguous()
    out = torch.empty((cin // 16, 2, cout // 64, 8, 3, 2, 64, 8), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_conv_pack_weights_wino_bf16x3(parts.data_ptr(), cout, cin, out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_conv_pack_weights_wino_bf16x3")
    return out


@functools.lru_cache(maxsize=256)
def wino_split_serves(n: int, h: int, w: int, cin: int, cout: int, pad: int) -> bool:
    """Whether the fused resnet blocks run this "same"-padded 3x3 / stride-1 layer on the split-operand Winograd form under
    ``conv_algo="auto"``: :func:`wino_split_form` answers 1 (16 x 16 blocks) or 2 (four images of at most 8 x 8 per block)."""
    return wino_split_form(n, h, w, cin, cout, pad) > 0


@functools.lru_cache(maxsize=256)
def wino_split_form(n: int, h: int, w: int, cin: int, cout: int, pad: int) -> int:
    """The route query of the split-operand Winograd form (``tia_conv3x3_wino_bf16x3_form``, host-only): 0 not taken, 1 a layer class
    on 16 x 16 blocks, 2 the class on blocks of four images (the kernel picks the geometry by the map size); negative for shapes no
    Winograd form serves."""
    from tiatoolbox_amd import _lib

    return int(_lib.load().tia_conv3x3_wino_bf16x3_form(n, h, w, cin, cout, pad))


@functools.lru_cache(maxsize=256)
def wino_form(n: int, h: int, w: int, cin: int, cout: int, pad: int) -> int:
    """Which Winograd form the fused resnet blocks take for a "same"-padded 3x3 / stride-1 layer (``tia_conv3x3_wino_form``, a
    host-only query): 1 F(4x2, 3x3), 0 F(2x2, 3x3); negative for shapes no Winograd form serves."""
    from tiatoolbox_amd import _lib

    return int(_lib.load().tia_conv3x3_wino_form(n, h, w, cin, cout, pad))


def hip_conv3x3_wino(x: torch.Tensor, u_packed: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None, *,
                     padding: int, relu: bool, pad_hi: int | None = None) -> torch.Tensor:
    """``relu(conv3x3(x, w) + bias + residual)``, stride 1, through a Winograd kernel: F(2x2, 3x3) (``tia_conv3x3_wino_nhwc_f32``) for
    weights from :func:`pack_conv_weights_wino` (leading dimension 16), F(4x2, 3x3) (``tia_conv3x3_wino42_nhwc_f32``) for weights from
    :func:`pack_conv_weights_wino42` (24), F(2x2, 3x3) on the bf16 matrix cores with both operands split
    (``tia_conv3x3_wino_bf16x3_nhwc_f32``) for the bf16 planes from :func:`pack_conv_weights_wino_split`.  float32 in / float32
    accumulate like :func:`hip_conv2d`, 2.25 x / 3 x fewer multiplies, results within ~1e-5 (relative) of it."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_conv3x3_wino expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    if residual is not None and not (_nhwc_ptr_ok(residual) and residual.dtype == torch.float32):
        msg = "hip_conv3x3_wino expects a float32 channels-last CUDA residual."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    split = u_packed.dtype == torch.bfloat16
    if split:
        ok = u_packed.dim() == 8 and tuple(u_packed.shape) == (cin // 16, 2, u_packed.shape[2], 8, 3, 2, 64, 8)  # noqa: PLR2004
        npos, n_cb = 16, u_packed.shape[2] if ok else 0
    else:
        npos = u_packed.shape[0] if u_packed.dim() == 7 else 0  # noqa: PLR2004
        ok = (npos in (16, 24) and tuple(u_packed.shape) == (npos, cin // 16, 2, u_packed.shape[3], 2, 64, 4)
              and u_packed.dtype == torch.float32)
        n_cb = u_packed.shape[3] if ok else 0
    if not ok or cin % 16 or not u_packed.is_contiguous() or u_packed.device != x.device:
        msg = (f"hip_conv3x3_wino: packed weights {tuple(u_packed.shape)} {u_packed.dtype} on {u_packed.device} do not match an input with "
               f"{cin} channels on {x.device} (expected pack_conv_weights_wino's [16, cin/16, 2, cout/64, 2, 64, 4] or "
               f"pack_conv_weights_wino42's [24, ...] float32, or pack_conv_weights_wino_split's [cin/16, 2, cout/64, 8, 3, 2, 64, 8] "
               f"bf16, contiguous).")
        raise ValueError(msg)
    cout = n_cb * 64
    behind = padding if pad_hi is None else pad_hi  # zero rows / columns behind the image (`padding` in front): "same", valid, TF-same
    ho, wo = h + padding + behind - 2, w + padding + behind - 2
    y = torch.empty((n, cout, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    if residual is not None and residual.shape != y.shape:
        msg = f"residual shape {tuple(residual.shape)} != output shape {tuple(y.shape)}"
        raise ValueError(msg)
    name = "tia_conv3x3_wino_nhwc_f32" if npos == 16 else "tia_conv3x3_wino42_nhwc_f32"  # noqa: PLR2004
    if split:
        name = "tia_conv3x3_wino_bf16x3_nhwc_f32"
    with torch.cuda.device(x.device):
        rc = getattr(_lib.load(), name)(x.data_ptr(), u_packed.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), n, h, w, cin, cout,
                                        padding, padding, ho, wo, int(relu), _lib.current_stream())
    _lib.check(rc, name)
    return y


class _MfmaBlock(nn.Module):
    """Shared machinery of the hand-written blocks: per-convolution packed weights (float32: ``[kh, kw, cin, cout]``; fp16 /
    bf16: ``[kh, kw, cin/8, cout, 8]``), float32 biases, and one launch per convolution with its epilogue fused."""

    # "winograd": float32 3x3 / stride-1 layers through tia_conv3x3_wino_nhwc_f32, large stride-2 launches through
    # tia_conv2d_bf16x3_nhwc_f32 (MfmaResNet.set_conv_algo)
    conv_algo = "direct"

    def __init__(self) -> None:
        super().__init__()
        self._packed: dict[tuple[str, torch.dtype | str], torch.Tensor | None] = {}  # (None: a split form without a usable split)
        self._bias32: dict[str, torch.Tensor] = {}

    def _wino(self, name: str, x: torch.Tensor | None = None) -> torch.Tensor | None:
        """The layer's Winograd-domain weights if it is to run on that kernel (float32 3x3 / stride 1, cin % 16, cout % 64): F(4x2, 3x3)
        where the route query :func:`wino_form` takes it for the input ``x``, F(2x2, 3x3) otherwise (and without an input); the bf16
        planes of the split-operand F(2x2, 3x3) where :func:`wino_split_serves` says so for ``x`` and ``U`` has a usable split."""
        conv = getattr(self, name)
        if (self.conv_algo != "winograd" or conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.dilation != (1, 1)
                or conv.groups != 1 or conv.in_channels % 16 or conv.out_channels % 64 or conv.padding[0] != conv.padding[1]
                or conv.padding[0] > 2):  # noqa: PLR2004
            return None
        # the split form where the route query takes the input; like F(4x2) its planes are packed by the first forward that is routed
        # to them (without an input -- `prepare` -- nothing says which shapes will come, and the table lives in the library alone)
        if x is not None and wino_split_serves(x.shape[0], x.shape[2], x.shape[3], conv.in_channels, conv.out_channels, conv.padding[0]):
            key = (name, "wino_split")
            if key not in self._packed or (self._packed[key] is not None and self._packed[key].device != conv.weight.device):
                self._packed[key] = pack_conv_weights_wino_split(conv)  # None: no usable split (remembered: asked once per device)
            if self._packed[key] is not None:
                return self._packed[key]
        key, pack = (name, "wino"), pack_conv_weights_wino
        if x is not None and wino_form(x.shape[0], x.shape[2], x.shape[3], conv.in_channels, conv.out_channels, conv.padding[0]) == 1:
            key, pack = (name, "wino42"), pack_conv_weights_wino42
        cached = self._packed.get(key)
        if cached is None or cached.device != conv.weight.device:
            cached = self._packed[key] = pack(conv)
        return cached

    def _w(self, name: str, dtype: torch.dtype) -> torch.Tensor:
        conv = getattr(self, name)
        cached = self._packed.get((name, dtype))
        if cached is None or cached.device != conv.weight.device:
            if conv.groups != 1 and dtype != torch.float32:
                msg = f"grouped convolutions run in float32 only (tia_conv3x3_grouped_nhwc_f32); got {dtype}."
                raise ValueError(msg)
            if conv.groups != 1:
                cached = pack_grouped_conv_weights(conv)
            else:
                cached = pack_conv_weights(conv) if dtype == torch.float32 else pack_conv_weights_h(conv, dtype)
            self._packed[(name, dtype)] = cached
        return cached

    def _split(self, name: str, x: torch.Tensor | None = None) -> torch.Tensor | None:
        """The layer's three-plane bf16 weights if it is to run on the split-operand kernel (``conv_algo="winograd"``, i.e. the engines'
        ``"auto"``; float32, ``groups == 1``, square kernel and stride, symmetric padding, cin % 16, cout % 128, a usable exact split)
        and, for an input ``x``, the route query :func:`conv_split_serves` takes it; ``None`` otherwise."""
        conv = getattr(self, name)
        if (self.conv_algo != "winograd" or conv.groups != 1 or conv.dilation != (1, 1) or conv.in_channels % 16 or conv.out_channels % 128
                or conv.kernel_size[0] != conv.kernel_size[1] or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]
                or conv.padding[0] >= conv.kernel_size[0] or conv.kernel_size[0] > 16 or conv.padding_mode != "zeros"):  # noqa: PLR2004
            return None
        if x is not None and not conv_split_serves(x.shape[0], x.shape[2], x.shape[3], conv.in_channels, conv.out_channels,
                                                   conv.kernel_size[0], conv.stride[0], conv.padding[0]):
            return None
        key = (name, "split")
        if key not in self._packed or (self._packed[key] is not None and self._packed[key].device != conv.weight.device):
            self._packed[key] = pack_conv_weights_split(conv)  # None: no usable split (remembered: asked once per device)
        return self._packed[key]

    def _b(self, name: str) -> torch.Tensor | None:
        conv = getattr(self, name)
        if conv.bias is None:
            return None
        cached = self._bias32.get(name)  # kept from before a cast to half (`prepare`): the kernels add the bias in float32
        if cached is not None and cached.device == conv.bias.device:
            return cached
        if conv.bias.dtype == torch.float32:
            return conv.bias
        cached = self._bias32[name] = conv.bias.detach().float().contiguous()
        return cached

    def prepare(self, dtype: torch.dtype) -> None:
        """Pack the weights for ``dtype`` and keep float32 biases NOW, from the float32 parameters (call before the module is
        cast to half: packing afterwards would start from weights and biases already rounded to half)."""
        for name in ("conv1", "conv2", "conv3", "down"):
            conv = getattr(self, name, None)
            if conv is None:
                continue
            self._w(name, dtype)
            if dtype == torch.float32 and self._wino(name) is None:
                # the split-operand kernel's weights, if conv_algo is already "winograd" (the engines set it before they prepare);
                # otherwise, as with _wino, the layer packs them in its first forward after set_conv_algo
                self._split(name)
            if conv.bias is not None:
                self._bias32[name] = conv.bias.detach().float().clone().contiguous()

    def _conv(self, name: str, x: torch.Tensor, residual: torch.Tensor | None, *, relu: bool) -> torch.Tensor:
        conv = getattr(self, name)
        k, st, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        if conv.groups != 1:  # ResNeXt's grouped 3x3 (float32 only: _w refuses half); conv_algo does not apply
            if x.dtype != torch.float32:
                msg = f"grouped convolutions run in float32 only (tia_conv3x3_grouped_nhwc_f32); got {x.dtype}."
                raise ValueError(msg)
            if residual is not None or k != 3 or pad != 1:  # noqa: PLR2004
                msg = "the grouped kernel is a 3x3 / padding 1 convolution without residual."
                raise ValueError(msg)
            return hip_conv3x3_grouped(x, self._w(name, x.dtype), self._b(name), stride=st, relu=relu)
        if x.dtype == torch.float32:
            u = self._wino(name, x)
            if u is not None:
                return hip_conv3x3_wino(x, u, self._b(name), residual, padding=pad, relu=relu)
            w3 = self._split(name, x)
            if w3 is not None:
                return hip_conv2d_split(x, w3, self._b(name), residual, kernel=k, stride=st, padding=pad, relu=relu)
            return hip_conv2d(x, self._w(name, x.dtype), self._b(name), residual, kernel=k, stride=st, padding=pad, relu=relu)
        return hip_conv2d_h(x, self._w(name, x.dtype), self._b(name), residual, cout=conv.out_channels, kernel=k, stride=st,
                            padding=pad, relu=relu)


class _MfmaBasic(_MfmaBlock):
    """BasicBlock as three launches: (downsample) / conv1+bias+ReLU / conv2+bias+residual+ReLU."""

    def __init__(self, blk: BasicBlock) -> None:
        super().__init__()
        self.conv1, self.conv2 = blk.conv1, blk.conv2
        self.down = blk.downsample[0] if blk.downsample is not None else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = x if self.down is None else self._conv("down", x, None, relu=False)
        out = self._conv("conv1", x, None, relu=True)
        return self._conv("conv2", out, identity, relu=True)


class _MfmaBottleneck(_MfmaBlock):
    """Bottleneck as (downsample) / 1x1+bias+ReLU / 3x3+bias+ReLU / 1x1+bias+residual+ReLU launches; a grouped 3x3 (ResNeXt)
    runs on ``tia_conv3x3_grouped_nhwc_f32``."""

    def __init__(self, blk: Bottleneck) -> None:
        super().__init__()
        self.conv1, self.conv2, self.conv3 = blk.conv1, blk.conv2, blk.conv3
        self.down = blk.downsample[0] if blk.downsample is not None else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = x if self.down is None else self._conv("down", x, None, relu=False)
        out = self._conv("conv1", x, None, relu=True)
        out = self._conv("conv2", out, None, relu=True)
        return self._conv("conv3", out, identity, relu=True)


def pack_stem_weights(conv) -> torch.Tensor:
    """OIHW ``[64, 3, 7, 7]`` -> the stem GEMM's B matrix ``[148, 64]`` (``(ky, kx, c)`` rows + one zero row).  ``conv``: the
    ``nn.Conv2d`` (stride 2, padding 3 are checked) or its (BN-folded) weight tensor."""
    from tiatoolbox_amd import _lib

    weight = conv.weight if isinstance(conv, nn.Module) else conv
    w = weight.detach().to(torch.float32).contiguous()
    geometry_ok = not isinstance(conv, nn.Conv2d) or (conv.stride == (2, 2) and conv.padding == (3, 3))
    if tuple(w.shape) != (64, 3, 7, 7) or not geometry_ok:
        msg = f"the stem kernel is conv7x7 / stride 2 / pad 3, 3 -> 64 channels; got weight {tuple(w.shape)}."
        raise ValueError(msg)
    if not w.is_cuda:
        msg = f"pack_stem_weights packs on a CUDA device; got a weight on {w.device}."
        raise ValueError(msg)
    out = torch.empty((148, 64), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_stem_pack_weights_f32(w.data_ptr(), out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_stem_pack_weights_f32")
    return out


def pack_stem_weights_h(weight: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """OIHW float32 ``[64, 3, 7, 7]`` -> the half stem's B matrix ``[22, 64, 8]`` (k = 24 ky + 3 kx + c, zero padded to 176)."""
    from tiatoolbox_amd import _lib

    w = weight.detach().to(torch.float32).contiguous()
    if tuple(w.shape) != (64, 3, 7, 7) or dtype not in (torch.float16, torch.bfloat16) or not w.is_cuda:
        msg = f"pack_stem_weights_h expects a CUDA float32 weight [64, 3, 7, 7] and fp16 / bf16; got {tuple(w.shape)}, {dtype}."
        raise ValueError(msg)
    out = torch.empty((22, 64, 8), dtype=dtype, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_stem_pack_weights_h(w.data_ptr(), _DT[dtype], out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_stem_pack_weights_h")
    return out


def hip_stem_conv_pool_h(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, *, dtype: torch.dtype) -> torch.Tensor:
    """:func:`hip_stem_conv_pool` on the half matrix cores (``tia_stem_conv7x7_pool_nhwc_h``): ``x / 255`` and the weights
    rounded to ``dtype`` (what ``model.half()`` feeds its first convolution), float32 accumulation, bias + ReLU + max-pool in
    float32, ONE rounding of the pooled result to ``dtype``.  ``x``: NHWC uint8 or float32 CUDA batch."""
    from tiatoolbox_amd import _lib

    if not (x.is_cuda and x.dim() == 4 and x.shape[-1] == 3 and x.is_contiguous() and x.dtype in (torch.uint8, torch.float32)):  # noqa: PLR2004
        msg = "hip_stem_conv_pool_h expects a contiguous NHWC uint8 / float32 CUDA batch with 3 channels."
        raise ValueError(msg)
    if w_packed.dtype != dtype or tuple(w_packed.shape) != (22, 64, 8):
        msg = "hip_stem_conv_pool_h expects weights packed by pack_stem_weights_h for the same dtype."
        raise ValueError(msg)
    n, h, w, _ = x.shape
    hp, wp = ((h - 1) // 2) // 2 + 1, ((w - 1) // 2) // 2 + 1
    y = torch.empty((n, 64, hp, wp), dtype=dtype, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_stem_conv7x7_pool_nhwc_h(x.data_ptr(), int(x.dtype == torch.uint8), w_packed.data_ptr(), bias.data_ptr(),
                                                      y.data_ptr(), _DT[dtype], n, h, w, _lib.current_stream())
    _lib.check(rc, "tia_stem_conv7x7_pool_nhwc_h")
    return y


def hip_stem_conv_pool(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, *,
                       out_dtype: torch.dtype = torch.float32, return_conv: bool = False):
    """``maxpool3x3/2(relu(conv7x7/2(x) + bias))`` in one kernel (``tia_stem_conv7x7_pool_conv_nhwc``).

    ``x``: NHWC ``[n, h, w, 3]`` contiguous CUDA tensor, ``uint8`` (scaled by 1/255 on load: ``ToTensor``) or ``float32`` (as is).
    Returns the pooled activations as an NCHW tensor stored channels-last (``[n, 64, hp, wp]``) of ``out_dtype`` (float32
    arithmetic; fp16 / bf16 = one rounding at the end, for the half-precision trunk).  ``return_conv=True``: ``(pooled, conv)``
    with ``conv = relu(conv7x7(x) + bias)`` before the pooling (``[n, 64, ho, wo]`` of ``out_dtype`` too, the UNet's first skip)."""
    from tiatoolbox_amd import _lib

    if not (x.is_cuda and x.dim() == 4 and x.shape[-1] == 3 and x.is_contiguous() and x.dtype in (torch.uint8, torch.float32)):
        msg = f"hip_stem_conv_pool expects a contiguous NHWC uint8 / float32 CUDA batch with 3 channels, got {tuple(x.shape)} {x.dtype}."
        raise ValueError(msg)
    if out_dtype not in _DT or w_packed.dtype != torch.float32 or bias.dtype != torch.float32:
        msg = (f"hip_stem_conv_pool computes in float32 (weights from pack_stem_weights, float32 bias) and returns float32 / fp16 / bf16; "
               f"got weights {w_packed.dtype}, bias {bias.dtype}, out_dtype {out_dtype}.")
        raise ValueError(msg)
    n, h, w, _ = x.shape
    hp, wp = ((h - 1) // 2) // 2 + 1, ((w - 1) // 2) // 2 + 1
    y = torch.empty((n, 64, hp, wp), dtype=out_dtype, device=x.device, memory_format=torch.channels_last)
    conv = None
    if return_conv:
        conv = torch.empty((n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=out_dtype, device=x.device,
                           memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_stem_conv7x7_pool_conv_nhwc(x.data_ptr(), int(x.dtype == torch.uint8), w_packed.data_ptr(), bias.data_ptr(),
                                                         y.data_ptr(), _DT[out_dtype], _ptr(conv), n, h, w, _lib.current_stream())
    _lib.check(rc, "tia_stem_conv7x7_pool_conv_nhwc")
    return (y, conv) if return_conv else y


def split_stem_weights(weight: torch.Tensor) -> tuple[torch.Tensor, bool]:
    """Float32 weights as the sum of three bf16 numbers: ``parts[0] = bf16(w)``, ``parts[1] = bf16(w - parts[0])``,
    ``parts[2] = bf16(w - parts[0] - parts[1])`` (round to nearest even; the subtractions are exact in float32), returned as a
    float32 tensor ``[3, *w.shape]`` whose values are bf16 numbers, and whether the split is USABLE by the bf16 matrix cores:
    ``parts.sum(0) == w`` exactly (compared in float64) and every non-zero part a finite, normal bf16 number.  Not usable:
    non-finite weights, weights next to overflow (``bf16(w)`` rounds to infinity), weights so small that a part falls below
    the normal range (``|w| < ~1e-33``, subnormals).  Device-agnostic: a few element-wise torch operations."""
    w = weight.detach().to(torch.float32)
    hi = w.to(torch.bfloat16).to(torch.float32)
    r1 = w - hi
    mid = r1.to(torch.bfloat16).to(torch.float32)
    lo = (r1 - mid).to(torch.bfloat16).to(torch.float32)
    parts = torch.stack((hi, mid, lo))
    tiny = torch.finfo(torch.bfloat16).tiny  # 2^-126, the smallest normal bf16 (= float32) number
    normal = (parts == 0) | (torch.isfinite(parts) & (parts.abs() >= tiny))
    exact = parts.to(torch.float64).sum(0) == w.to(torch.float64)  # NaN compares unequal
    return parts, bool(normal.all()) and bool(exact.all())


def pack_stem_weights_split(conv) -> torch.Tensor | None:
    """OIHW float32 ``[64, 3, 7, 7]`` -> ``[3, 22, 64, 8]`` bf16: the planes ``hi``, ``mid``, ``lo`` of
    :func:`split_stem_weights`, each in the half stem's layout (``tia_stem_pack_weights_bf16x3``).  ``None`` when the weights
    have no usable exact split: the caller then keeps the float32 stem."""
    from tiatoolbox_amd import _lib

    weight = conv.weight if isinstance(conv, nn.Module) else conv
    w = weight.detach().to(torch.float32).contiguous()
    geometry_ok = not isinstance(conv, nn.Conv2d) or (conv.stride == (2, 2) and conv.padding == (3, 3))
    if tuple(w.shape) != (64, 3, 7, 7) or not geometry_ok or not w.is_cuda:
        msg = f"the stem kernel is conv7x7 / stride 2 / pad 3, 3 -> 64 channels on a CUDA device; got weight {tuple(w.shape)} on {w.device}."
        raise ValueError(msg)
    parts, usable = split_stem_weights(w)
    if not usable:
        return None
    parts = parts.contiguous()
    out = torch.empty((3, 22, 64, 8), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_stem_pack_weights_bf16x3(parts.data_ptr(), out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_stem_pack_weights_bf16x3")
    return out


def hip_stem_conv_pool_split(x: torch.Tensor, w_packed3: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``maxpool3x3/2(relu(conv7x7/2(x / 255) + bias))`` of a uint8 NHWC batch on the bf16 matrix cores with exactly split
    float32 weights (``tia_stem_conv7x7_pool_nhwc_u8x3``): bytes and weight parts are bf16 numbers, their products exact, the
    accumulation float32; ``conv = fl(sum / 255) + bias``.  Float32 arithmetic in another summation order than
    :func:`hip_stem_conv_pool`.  Returns ``[n, 64, hp, wp]`` float32, channels-last."""
    from tiatoolbox_amd import _lib

    if not (x.is_cuda and x.dim() == 4 and x.shape[-1] == 3 and x.is_contiguous() and x.dtype == torch.uint8):  # noqa: PLR2004
        msg = f"hip_stem_conv_pool_split expects a contiguous NHWC uint8 CUDA batch with 3 channels, got {tuple(x.shape)} {x.dtype}."
        raise ValueError(msg)
    if w_packed3.dtype != torch.bfloat16 or tuple(w_packed3.shape) != (3, 22, 64, 8) or not w_packed3.is_contiguous():
        msg = "hip_stem_conv_pool_split expects weights packed by pack_stem_weights_split."
        raise ValueError(msg)
    n, h, w, _ = x.shape
    hp, wp = ((h - 1) // 2) // 2 + 1, ((w - 1) // 2) // 2 + 1
    y = torch.empty((n, 64, hp, wp), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_stem_conv7x7_pool_nhwc_u8x3(x.data_ptr(), w_packed3.data_ptr(), bias.data_ptr(), y.data_ptr(), n, h, w,
                                                         _lib.current_stream())
    _lib.check(rc, "tia_stem_conv7x7_pool_nhwc_u8x3")
    return y


def pack_conv_weights_split(conv: nn.Conv2d) -> torch.Tensor | None:
    """OIHW float32 -> ``[kh, kw, cin/16, cout/128, 3, 2, 128, 8]`` bf16: the planes ``hi``, ``mid``, ``lo`` of
    :func:`split_stem_weights` in the stage layout of ``tia_conv2d_bf16x3_nhwc_f32`` (``tia_conv_pack_weights_bf16x3``).  ``None``
    when the weights have no usable exact split (one ``info`` line): the layer then keeps the float32 kernel."""
    from tiatoolbox_amd import _lib

    w = conv.weight.detach().to(torch.float32).contiguous()
    cout, cin, kh, kw = w.shape
    if cin % 16 or cout % 128 or conv.groups != 1:
        msg = f"the split-operand kernel needs cin % 16 == 0, cout % 128 == 0 and groups == 1; got weight {tuple(w.shape)}."
        raise ValueError(msg)
    parts, usable = split_stem_weights(w)
    if not usable:
        logger.info("a %s convolution's weights have no exact three-part bf16 split (non-finite or extreme exponents); the "
                    "layer keeps the float32 kernel.", tuple(w.shape))
        return None
    parts = parts.contiguous()
    out = torch.empty((kh, kw, cin // 16, cout // 128, 3, 2, 128, 8), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_conv_pack_weights_bf16x3(parts.data_ptr(), cout, cin, kh, kw, out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_conv_pack_weights_bf16x3")
    return out


@functools.lru_cache(maxsize=256)
def conv_split_serves(n: int, h: int, w: int, cin: int, cout: int, kernel: int, stride: int, padding: int) -> bool:
    """Whether the fused resnet blocks run this symmetric-padded convolution on the split-operand kernel under ``conv_algo="auto"``
    (``tia_conv2d_bf16x3_serves``, a host-only query)."""
    from tiatoolbox_amd import _lib

    ho, wo = (h + 2 * padding - kernel) // stride + 1, (w + 2 * padding - kernel) // stride + 1
    return _lib.load().tia_conv2d_bf16x3_serves(n, h, w, cin, cout, kernel, kernel, stride, padding, padding, ho, wo) == 1


def hip_conv2d_split(x: torch.Tensor, w_packed3: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None, *,
                     kernel: int, stride: int, padding: int, relu: bool) -> torch.Tensor:
    """``relu(conv2d(x, w) + bias + residual)`` on a float32 channels-last CUDA tensor on the bf16 matrix cores with both operands
    split into three bf16 numbers (``tia_conv2d_bf16x3_nhwc_f32``; weights from :func:`pack_conv_weights_split`): float32 in,
    float32 accumulate, another summation order than :func:`hip_conv2d`."""
    from tiatoolbox_amd import _lib

    if not (_nhwc_ptr_ok(x) and x.dtype == torch.float32):
        msg = "hip_conv2d_split expects a float32 channels-last CUDA tensor."
        raise ValueError(msg)
    n, cin, h, w = x.shape
    if (w_packed3.dim() != 8 or w_packed3.dtype != torch.bfloat16 or not w_packed3.is_contiguous() or w_packed3.device != x.device  # noqa: PLR2004
            or tuple(w_packed3.shape) != (kernel, kernel, cin // 16, w_packed3.shape[3], 3, 2, 128, 8) or cin % 16):
        msg = (f"hip_conv2d_split: weights {tuple(w_packed3.shape)} {w_packed3.dtype} on {w_packed3.device} are not "
               f"pack_conv_weights_split's [k, k, cin/16, cout/128, 3, 2, 128, 8] bf16 for a {kernel}x{kernel} kernel over {cin} channels on {x.device}.")
        raise ValueError(msg)
    cout = w_packed3.shape[3] * 128
    shape = _conv_out_shape("hip_conv2d_split", x, cout, residual, kernel=kernel, stride=stride, pad_lo=padding, pad_hi=padding)
    y = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv2d_bf16x3_nhwc_f32(x.data_ptr(), w_packed3.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), n, h, w,
                                                    cin, cout, kernel, kernel, stride, padding, padding, int(relu),
                                                    _lib.current_stream())
    _lib.check(rc, "tia_conv2d_bf16x3_nhwc_f32")
    return y


class MfmaResNet(nn.Module):
    """ResNet trunk on hand-written kernels only: the stem (7x7 / 3 input channels + bias + ReLU + max-pool, one float32 MFMA
    kernel reading uint8 or float32 patches) and every block convolution (BasicBlock: resnet18/34; Bottleneck: resnet50/101,
    wide_resnet50_2/101_2, resnext50_32x4d/101_32x8d) as an MFMA implicit GEMM with its epilogue fused (BN folded, channels-last;
    the grouped 3x3 of ResNeXt: ``tia_conv3x3_grouped_nhwc_f32``, float32 only) -- ``tia_conv2d_nhwc_f32`` for float32 (the
    reference's arithmetic), ``tia_conv2d_nhwc_h`` once the module has been cast to fp16 / bf16 (float32 accumulation; the stem
    is then ``tia_stem_conv7x7_pool_nhwc_h``: half inputs and weights on the half matrix cores, one rounding of the result).  A ``uint8`` input means ``ToTensor`` has been deferred into the stem: the
    kernel divides by 255 while it loads.  In ``"winograd"`` mode (``set_conv_algo``; the engines' ``conv_algo="auto"``) a float32
    trunk runs the stem of a uint8 batch on the bf16 matrix cores with exactly split weights (:func:`hip_stem_conv_pool_split`:
    float32 arithmetic, another summation order); ``"direct"``, float32 input, half trunks and weights without an exact split
    (one ``info`` line) keep the kernels above."""

    accepts_uint8 = True

    def __init__(self, trunk: nn.Sequential) -> None:
        super().__init__()
        folded = fold_conv_bn(trunk)
        self.stem = folded[0]
        self._stem_packed: torch.Tensor | None = None
        self._stem_packed_dtype: torch.dtype | None = None
        self._stem_split: torch.Tensor | None = None  # [3, 22, 64, 8] bf16 planes; None: not packed, or no exact split
        self.conv_algo = "direct"
        blocks = []
        for layer in list(folded)[4:]:
            for blk in layer:
                if not isinstance(blk, (BasicBlock, Bottleneck)):
                    msg = "MfmaResNet covers BasicBlock / Bottleneck trunks."
                    raise TypeError(msg)
                blocks.append(_MfmaBasic(blk) if isinstance(blk, BasicBlock) else _MfmaBottleneck(blk))
        self.blocks = nn.Sequential(*blocks)

    def stem_forward(self, x: torch.Tensor) -> torch.Tensor:
        """``x``: NCHW view of an NHWC batch (what ``infer_batch`` passes) or the NHWC batch itself."""
        if x.shape[-1] != 3:  # NCHW view -> the NHWC memory underneath (a copy only if it was not channels-last)
            x = x.permute(0, 2, 3, 1)
        x = x.contiguous()
        if x.dtype not in (torch.uint8, torch.float32):
            x = x.to(torch.float32)
        dtype = self.stem.weight.dtype
        w = self._stem_packed
        if w is None or w.device != self.stem.weight.device or self._stem_packed_dtype != dtype:
            self.prepare_stem(dtype)
            w = self._stem_packed
        if dtype == torch.float32:
            if self.conv_algo == "winograd" and x.dtype == torch.uint8 and self._stem_split is not None:
                return hip_stem_conv_pool_split(x, self._stem_split, self._stem_bias)
            return hip_stem_conv_pool(x, w, self._stem_bias)
        return hip_stem_conv_pool_h(x, w, self._stem_bias, dtype=dtype)  # half matrix cores, float32 accumulate

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.blocks(self.stem_forward(x))

    def set_conv_algo(self, algo: str) -> None:
        """``"direct"`` (the module's own default: float32 implicit GEMM, the reference's operation class AND order of accumulation over
        taps) or ``"winograd"``: the float32 3x3 / stride-1 block convolutions through F(2x2, 3x3) -- float32 in, float32 accumulate,
        2.25 x fewer multiplies, log-probabilities within the engine's smoke tolerance of the direct path (the class of arithmetic
        of the vendor libraries' own solvers for these layers).  The ENGINES choose: their default ``conv_algo="auto"`` sets
        ``"winograd"`` here, ``conv_algo="direct"`` is the audit mode (``EngineABC._inference_model``)."""
        if algo not in ("direct", "winograd"):
            msg = f"conv_algo must be 'direct' or 'winograd', got {algo!r}."
            raise ValueError(msg)
        self.conv_algo = algo  # the stem of a uint8 batch: "winograd" = exactly split weights on the bf16 matrix cores
        for blk in self.blocks:
            blk.conv_algo = algo

    def prepare(self, dtype: torch.dtype) -> None:
        """Pack every convolution for ``dtype`` from the float32 parameters (the engine calls this on the device, before it
        casts the inference copy to half)."""
        self.prepare_stem(dtype)
        for blk in self.blocks:
            blk.prepare(dtype)

    def prepare_stem(self, dtype: torch.dtype) -> None:
        weight = self.stem.weight.detach().float()
        self._stem_packed = pack_stem_weights(weight) if dtype == torch.float32 else pack_stem_weights_h(weight, dtype)
        self._stem_packed_dtype = dtype
        self._stem_bias = self.stem.bias.detach().float().clone().contiguous()
        self._stem_split = None
        if dtype == torch.float32:  # both packings side by side (38 KB + 68 KB): set_conv_algo switches without repacking
            self._stem_split = pack_stem_weights_split(weight)
            if self._stem_split is None:
                logger.info("MfmaResNet: the stem weights have no exact three-part bf16 split (non-finite or extreme "
                            "exponents); uint8 batches keep the float32 stem kernel.")


def fuse_cnn_model(model: nn.Module, *, epilogue_fusion: bool | str = False) -> nn.Module:
    """Derived inference copy of a ``CNNModel``/``CNNBackbone`` with BN folded into the convolutions.

    ``epilogue_fusion="mfma"`` (GPU, any dtype): stem and block convolutions on the hand-written kernels
    (:class:`MfmaResNet`); ``False``: BN folding only (CPU).
    """
    fused = copy.deepcopy(model).eval()
    trunk = fused.feat_extract
    if isinstance(trunk, nn.Sequential) and len(trunk) == 8 and isinstance(trunk[0], nn.Conv2d):
        if epilogue_fusion == "mfma":
            fused.feat_extract = MfmaResNet(trunk)
        elif epilogue_fusion:
            msg = f"unknown epilogue_fusion {epilogue_fusion!r}: 'mfma' or False."
            raise ValueError(msg)
        else:
            fused.feat_extract = fold_conv_bn(trunk)
    return fused

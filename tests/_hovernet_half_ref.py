"""References shared by ``test_hovernet_half.py`` (host) and ``test_hovernet_half_gpu.py`` (``-m gpu``): what the half-precision
kernels of ``FusedHoVerNet`` compute, stated with plain torch ops on the CPU, and the seeded networks the graph / engine tests use.

* convolution with the extended epilogue (``tia_conv2d_nhwc_h_ex``): a float32 CPU convolution of the SAME half-rounded inputs and
  weights; ``v = act(conv + bias [+ residual])`` in float32, ``y = half(v)``, ``y2 = half(relu(v * post_scale + post_shift))`` with
  product and sum rounded separately -- ``y2`` comes from the UNROUNDED ``v``.  Bound (the project's own for the half convolution,
  ``tests/test_engine.py::test_hip_mfma_conv_half_matches_torch_cpu_fp32``): ``eps |ref| + 1e-4 max |ref|`` with ``eps`` = 2^-10 /
  2^-7; for ``y2`` the same bound propagated: ``eps |y2_ref| + |post_scale| 1e-4 max |v_ref|``.
* grouped valid convolution (``tia_grouped_conv_valid_nhwc_h``): float64 on the half inputs and the half-rounded weights; bound per
  element ``2 K 2^-24 sum |w x| + eps |ref|`` with ``K = 32 k^2`` (half products are exact in float32, so ``K 2^-24 sum |w x|`` bounds
  any IEEE summation order of the K terms; the factor 2 is the allowance for the matrix unit's internal order).
* view activation (``tia_scale_shift_act_view_nhwc_h``): ``x.float() * scale``, ``+ shift``, ``relu``, ``.to(dtype)`` -- equality.
* the graphs: ``HoVerNet(num_types=6)`` in both modes and ``HoVerNetPlus(3, 5)`` with RANDOMISED BatchNorm statistics, their float32
  CPU logits computed once per session.
* ``install_torch_kernels``: the HIP wrappers of the half graph replaced by these definitions, with call counters (the host test).
"""

from __future__ import annotations

import functools

import torch
import torch.nn.functional as F  # noqa: N812
from _unet_half_ref import HALVES, MANTISSA, randomise_bn, rel_err  # noqa: F401

EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
IDS = {torch.float16: "fp16", torch.bfloat16: "bf16"}


# ---------------------------------------------------------------------------------------------------------------- convolution
def conv_ex_ref(x, w, bias, res, *, stride, pad_lo, pad_hi, relu, post_scale=None, post_shift=None):
    """``x`` [n, cin, h, w], ``w`` OIHW and ``res`` of one half dtype, ``bias`` / ``post_*`` float32.  Returns ``(v, y2)`` in FLOAT32:
    ``v`` the unrounded epilogue value, ``y2`` the unrounded activated copy (None without ``post_*``); the kernel's outputs are
    these through one ``.to(dtype)`` up to the accumulation order."""
    v = F.conv2d(F.pad(x.float(), (pad_lo, pad_hi, pad_lo, pad_hi)), w.float(), bias, stride)
    if res is not None:
        v = v + res.float()
    if relu:
        v = F.relu(v)
    if post_scale is None:
        return v, None
    p = v * post_scale[None, :, None, None]
    return v, F.relu(p + post_shift[None, :, None, None])


def conv_bound(ref, dtype):
    """``eps |ref| + 1e-4 max |ref|`` per element (float64)."""
    ref = ref.double()
    return EPS[dtype] * ref.abs() + 1e-4 * float(ref.abs().max())


def post_bound(y2_ref, v_ref, post_scale, dtype):
    """The same bound propagated through the affine: ``eps |y2_ref| + |post_scale| 1e-4 max |v_ref|``."""
    return EPS[dtype] * y2_ref.double().abs() + post_scale.double().abs()[None, :, None, None] * 1e-4 * float(v_ref.double().abs().max())


def pack_h(w_oihw, dtype):
    """OIHW float32 -> ``[kh, kw, cin/8, cout, 8]`` of ``dtype`` (what ``tia_conv_pack_weights_h`` writes)."""
    cout, cin, kh, kw = w_oihw.shape
    return w_oihw.to(dtype).reshape(cout, cin // 8, 8, kh, kw).permute(3, 4, 1, 0, 2).contiguous()


def unpack_h(wp):
    kh, kw, c8, cout, _ = wp.shape
    return wp.permute(3, 2, 4, 0, 1).reshape(cout, c8 * 8, kh, kw)


def post_hand_example(dtype):
    """One pixel, 32 -> 64 channels, one-hot 1x1 weights (output c reads input c % 32), x = 1, residual = u = the half type's half-ulp
    of 1 (2^-12 fp16, 2^-9 bf16): v = 1 + u exactly in float32, and 1 after rounding to half (a tie, to even).  post_scale = 1 / u,
    post_shift = -1 / u: from the unrounded v, y2 = (1 + u) / u - 1 / u = 1 exactly (every step exact in float32); from the rounded
    v it would be 0.  Returns ``(x, w_oihw, residual, post_scale, post_shift, want_y, want_y2)``, the wanted values as float64."""
    u = 2.0 ** -(MANTISSA[dtype] + 2)
    x = torch.ones((1, 32, 1, 1), dtype=dtype)
    w = torch.zeros((64, 32, 1, 1))
    w[torch.arange(64), torch.arange(64) % 32] = 1.0
    res = torch.full((1, 64, 1, 1), u, dtype=torch.float64).to(dtype)
    assert float(res.double().flatten()[0]) == u  # the half-ulp is a number of the half type
    scale, shift = torch.full((64,), 1.0 / u), torch.full((64,), -1.0 / u)
    return x, w.to(dtype), res, scale, shift, torch.ones((1, 64, 1, 1), dtype=torch.float64), torch.ones((1, 64, 1, 1), dtype=torch.float64)


# -------------------------------------------------------------------------------------------------------------- grouped valid
def grouped_ref(x, w, groups):
    """``x`` [n, groups * 32, h, w] half, ``w`` OIHW [groups * 8, 32, k, k] ALREADY rounded to that half type.  Returns ``(ref, bound)``
    in float64: ``bound = 2 K 2^-24 sum |w x| + eps |ref|``, K = 32 k^2."""
    k = w.shape[-1]
    ref = F.conv2d(x.double(), w.double(), None, 1, 0, 1, groups)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 0, 1, groups)
    return ref, 2 * (32 * k * k) * 2.0 ** -24 * mag + EPS[x.dtype] * ref.abs()


def pack_grouped_h(w_oihw, groups, dtype):
    """OIHW float32 [groups * 8, 32, k, k] -> ``[groups, k, k, 4, 8, 8]`` of ``dtype`` (what ``tia_grouped_conv_pack_weights_h`` writes)."""
    k = w_oihw.shape[-1]
    return w_oihw.to(dtype).reshape(groups, 8, 4, 8, k, k).permute(0, 4, 5, 2, 1, 3).contiguous()


def unpack_grouped_h(wp):
    groups, k = wp.shape[0], wp.shape[1]
    return wp.permute(0, 4, 3, 5, 1, 2).reshape(groups * 8, 32, k, k)


# ------------------------------------------------------------------------------------------------------------ view activation
def view_act_ref(x, scale, shift, *, relu=True):
    p = x.float() * scale[None, :, None, None]
    a = p + shift[None, :, None, None]
    return (F.relu(a) if relu else a).to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------------- graphs
GRAPHS = {"fast": ("fast", 256), "original": ("original", 270), "plus": ("fast", 256)}


@functools.lru_cache(maxsize=3)
def graph_case(kind: str):
    """``(model, x_float_nchw [2 or 1 images], ref)``: built and run on the CPU once per session; callers must not modify it.
    ``fast`` carries two images (the tests take ``x[:1]`` / ``ref[:1]`` for n = 1); seeds of ``test_fused_graphs.py``."""
    from tiatoolbox_amd.models.architecture.hovernet import HoVerNet
    from tiatoolbox_amd.models.architecture.hovernetplus import HoVerNetPlus

    mode, size = GRAPHS[kind]
    if kind == "plus":
        torch.manual_seed(2)
        model = HoVerNetPlus(num_types=3, num_layers=5).eval()
        g = randomise_bn(model, 7)
    else:
        torch.manual_seed(3)
        model = HoVerNet(num_types=6, mode=mode).eval()
        g = randomise_bn(model, 5)
    x = torch.randint(0, 256, (2 if kind == "fast" else 1, 3, size, size), generator=g).float()
    with torch.inference_mode():
        ref = model(x)
    return model, x, ref


# ------------------------------------------------------------------------------- the half graph on the CPU (host test fixture)
def install_torch_kernels(monkeypatch):
    """Replace the HIP wrappers ``hovernet_fused`` calls in half precision by what the header says they compute.  Returns
    ``(hovernet_fused module, calls, probes)``; ``probes["stem"]`` holds the last stem output."""
    import tiatoolbox_amd.models.architecture.hovernet_fused as hf

    calls = {"conv_h": 0, "conv_h_ex": 0, "post": 0, "grouped": 0, "thin": 0, "head": 0, "up": 0, "view": 0}
    probes = {}

    def pack_conv(conv, dtype):
        w = conv.weight.detach()
        assert w.dtype == torch.float32  # packed from the float32, BN-folded weights: one rounding
        return pack_h(w, dtype)

    def conv_h(x, wp, bias, res, *, cout, kernel, stride, padding, relu):
        calls["conv_h"] += 1
        assert x.dtype == wp.dtype and x.dtype in HALVES and (bias is None or bias.dtype == torch.float32)
        assert (res is None or res.dtype == x.dtype) and wp.shape[0] == kernel and wp.shape[3] == cout
        v, _ = conv_ex_ref(x, unpack_h(wp), bias, res, stride=stride, pad_lo=padding, pad_hi=padding, relu=relu)
        return v.to(x.dtype)

    def conv_h_ex(x, wp, bias, res, *, cout, kernel, stride, pad_lo, pad_hi, relu, post_scale=None, post_shift=None, want_raw=True):
        calls["conv_h_ex"] += 1
        assert x.dtype == wp.dtype and x.dtype in HALVES and (bias is None or bias.dtype == torch.float32)
        assert (res is None or res.dtype == x.dtype) and wp.shape[0] == kernel and wp.shape[3] == cout
        v, y2 = conv_ex_ref(x, unpack_h(wp), bias, res, stride=stride, pad_lo=pad_lo, pad_hi=pad_hi, relu=relu, post_scale=post_scale,
                            post_shift=post_shift)
        if post_scale is None:
            assert want_raw
            return v.to(x.dtype)
        calls["post"] += 1
        assert post_scale.dtype == post_shift.dtype == torch.float32 and kernel == 1  # the second output: 1x1 layers only
        return (v.to(x.dtype) if want_raw else None), y2.to(x.dtype)

    def pack_grouped(weight, groups, dtype):
        assert weight.dtype == torch.float32
        return pack_grouped_h(weight.detach(), groups, dtype)

    def grouped(x, wp, *, groups, kernel, out=None):
        calls["grouped"] += 1
        assert x.dtype == wp.dtype and x.dtype in HALVES and out is not None and out.dtype == x.dtype and wp.shape[1] == kernel
        y = F.conv2d(x.float(), unpack_grouped_h(wp).float(), None, 1, 0, 1, groups).to(x.dtype)
        out.copy_(y)
        return out

    def view(x, scale, shift, *, relu=True):
        calls["view"] += 1
        assert x.dtype in HALVES and scale.dtype == shift.dtype == torch.float32
        return view_act_ref(x, scale, shift, relu=relu)

    def pack_thin(weight):
        assert weight.dtype == torch.float32
        cout, c, kh, kw = weight.shape
        packed = torch.zeros((kh, 32, cout))
        packed[:, :kw * c] = weight.detach().permute(2, 3, 1, 0).reshape(kh, kw * c, cout)
        return packed

    def thin(x, wp, bias, *, kernel, stride, pad_lo, pad_hi, relu, out_dtype=torch.float32):
        calls["thin"] += 1
        assert x.dtype == wp.dtype == bias.dtype == torch.float32
        c = x.shape[1]
        w = wp[:, :kernel * c].reshape(kernel, kernel, c, -1).permute(3, 2, 0, 1)
        y = F.conv2d(F.pad(x, (pad_lo, pad_hi, pad_lo, pad_hi)), w, bias, stride)
        probes["stem"] = (F.relu(y) if relu else y).to(out_dtype)
        return probes["stem"]

    def head(x, weight, bias, *, pre_scale=None, pre_shift=None):
        calls["head"] += 1
        assert x.dtype in HALVES and weight.dtype == torch.float32 and bias.dtype == torch.float32
        assert pre_scale is not None and pre_scale.dtype == pre_shift.dtype == torch.float32
        a = F.relu(x.float() * pre_scale[None, :, None, None] + pre_shift[None, :, None, None])
        return F.conv2d(a, weight.reshape(weight.shape[0], 64, 1, 1), bias)

    def up(x, y, scale=None, shift=None):
        calls["up"] += 1
        assert x.dtype == y.dtype and x.dtype in HALVES and scale is None and shift is None
        return (x.float().repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) + y.float()).to(x.dtype)

    for name, fn in (("pack_conv_weights_h", pack_conv), ("hip_conv2d_h", conv_h), ("hip_conv2d_h_ex", conv_h_ex),
                     ("pack_grouped_conv_valid_weights_h", pack_grouped), ("hip_grouped_conv_valid_h", grouped),
                     ("hip_scale_shift_act_view", view), ("pack_thin_conv_weights", pack_thin), ("hip_conv2d_thin", thin),
                     ("hip_conv1x1_head", head), ("hip_upsample2x_add", up)):
        monkeypatch.setattr(hf, name, fn, raising=False)  # (raising=False: on a tree without the feature the tests fail at `prepare`)
    return hf, calls, probes

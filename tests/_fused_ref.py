"""Host-only helpers of ``tests/test_fused_kernel_reference.py``: references, case lists, bounds and comparisons for the kernels that
``FusedHoVerNet`` and ``FusedUNet`` launch between their plain convolutions -- the slice kernel's POST / PRE / thin forms, the class
head, the grouped valid convolution and the element-wise passes.  Nothing here touches a device.

A case is a ``_conv_ref.Case`` whose ``kernel`` is one of ``post / pre / thin / head / gvalid``:

* post   -- ``tia_conv2d_post_nhwc_f32``: any k, stride, ``pad_lo`` / ``pad_hi``;
* pre    -- ``tia_conv1x1_pre_nhwc_f32``: k = 1, no border, any stride;
* thin   -- ``tia_conv2d_thin_nhwc_f32``: ``cin`` = the image's few channels c, ``c * k <= 32``;
* head   -- ``tia_conv1x1_head_nhwc_f32``: cin = 64, cout <= 8, k = 1;
* gvalid -- ``tia_grouped_conv_valid_nhwc_f32``: ``groups`` groups of 32 -> 8 channels, no border, stride 1.
"""

from __future__ import annotations

import itertools

import numpy as np
import torch
import torch.nn.functional as F  # noqa: N812

import _conv_ref as R  # noqa: N812
from _conv_ref import Case

CONV_KERNELS = ("post", "pre", "thin", "head", "gvalid")
WHERE = "(image, channel, row, column)"

# ------------------------------------------------------------------------------------------------------------------------------------
# the grid caps of the grid-stride kernels, mirrored from tiatoolbox_amd/csrc/cnn_epilogue.hip (workgroups of 256 threads)
# ------------------------------------------------------------------------------------------------------------------------------------
THREADS = 256                              # `constexpr int ET = 256`
CAP_BIAS_ACT = 256 * 32 * THREADS          # `eblocks`: `if (b > 256L * 32) b = 256L * 32`   -- threads = 16-byte vectors per pass
CAP_POOL = CAP_BIAS_ACT                    # `launch_stem` sizes its grid with `eblocks` too (vectors of the OUTPUT)
CAP_SCALE_SHIFT = 256 * 64 * THREADS       # `tia_scale_shift_act_nhwc_f32`: `if (blocks > 256L * 64) blocks = 256L * 64`
CAP_SCALE_SHIFT_VIEW = 256 * 64 * THREADS  # `tia_scale_shift_act_view_nhwc_f32`: the same line
CAP_UPSAMPLE = 256 * 64 * THREADS          # `tia_upsample2x_add_act_nhwc_f32`: the same line (vectors of the output)
CAP_HEAD = 256 * 16 * 64                   # `launch_head`: `if (blocks > 256L * 16) blocks = 256L * 16`; 4 waves x U = 4 groups x 4 pixels

# one case per capped kernel with more than TWICE the cap, so that every thread runs the loop body more than once
# (shape [n, c, h, w]; for the pool the input shape)
BEYOND_CAP = {
    "bias_act": ((2, 64, 512, 520), "bfloat16"),
    "pool": ((2, 64, 727, 728), "float32"),
    "scale_shift": ((2, 256, 260, 256), "float32"),
    "scale_shift_view": ((2, 256, 260, 256), "float32"),   # a 256-channel prefix of 264, rows 1 .. 260 of 262
    "upsample": ((2, 256, 130, 128), "float32"),           # the low-resolution input; the output is [2, 256, 260, 256]
    "head": ((2, 64, 520, 512), "float32"),                # cout 3 with the activation on load
}


def work_items(kernel: str) -> tuple[int, int]:
    """(work items of the case in ``BEYOND_CAP``, the kernel's cap) in the kernel's own unit: 16-byte vectors, pixels for the head."""
    (n, c, h, w), dtype = BEYOND_CAP[kernel]
    per_vec = 4 if dtype == "float32" else 8
    if kernel == "pool":
        return n * ((h + 1) // 2) * ((w + 1) // 2) * c // per_vec, CAP_POOL
    if kernel == "upsample":
        return n * 2 * h * 2 * w * c // per_vec, CAP_UPSAMPLE
    if kernel == "head":
        return n * h * w, CAP_HEAD
    cap = {"bias_act": CAP_BIAS_ACT, "scale_shift": CAP_SCALE_SHIFT, "scale_shift_view": CAP_SCALE_SHIFT_VIEW}[kernel]
    return n * h * w * c // per_vec, cap


# ------------------------------------------------------------------------------------------------------------------------------------
# which instance of conv_mfma_f32_kernel a POST / PRE case runs on: the rule of conv2d_impl (csrc/conv_mfma.hip)
# ------------------------------------------------------------------------------------------------------------------------------------
def tile_width(case: Case) -> int:
    """``narrow = kh == 1 && kw == 1 && cin <= 256``; the 128-wide tile when ``cout % 128 == 0 && !narrow``, else the 64-wide one."""
    narrow = case.k == 1 and case.cin <= 256  # noqa: PLR2004
    return 128 if case.cout % 128 == 0 and not narrow else 64


def even_group(n: int, limit: int) -> int:
    """``tia::even_group``: ``ceil(n / k)`` images for the smallest ``k`` whose groups fit ``limit``."""
    if n <= limit:
        return n
    k = -(-n // limit)
    return -(-n // k)


def conv_group(case: Case) -> int:
    """Images per launch of ``conv2d_impl``: < 2 GiB of input (and < 2^30 output pixels), in equal groups."""
    limit = (2 ** 31 - 1) // (case.h * case.w * case.cin * 4)
    if limit * case.ho * case.wo > (2 ** 31 - 1) // 2:
        limit = (2 ** 31 - 1) // 2 // (case.ho * case.wo)
    return even_group(case.n, limit)


def thin_extra(case: Case) -> int:
    """Zero columns ``hip_conv2d_thin`` appends so that the last output column's 32-float read stays inside its row."""
    need = (case.wo - 1) * case.stride + -(-32 // case.cin)
    return max(need - (case.w + case.pad_lo + case.pad_hi), 0)


def epilogues(case: Case):
    """(bias, residual, ReLU) combinations the case's entry point has arguments for."""
    if case.kernel in ("post", "pre"):
        return list(itertools.product((False, True), repeat=3))
    if case.kernel == "thin":
        return [(b, False, a) for b in (False, True) for a in (False, True)]
    if case.kernel == "head":
        return [(b, False, False) for b in (False, True)]
    return [(False, False, False)]


# ------------------------------------------------------------------------------------------------------------------------------------
# references of the convolution forms
# ------------------------------------------------------------------------------------------------------------------------------------
def _per_channel(v: torch.Tensor) -> torch.Tensor:
    return v.view(1, -1, 1, 1)


def scale_shift_ref(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, relu: bool = True) -> torch.Tensor:
    """``relu(fl32(fl32(x * scale[c]) + shift[c]))``: the specified arithmetic of the PRE operand, the POST output and
    ``scale_shift_act`` (torch's CPU ``mul`` and ``add`` round separately)."""
    assert x.dtype == scale.dtype == shift.dtype == torch.float32
    v = torch.mul(x, _per_channel(scale))
    v = torch.add(v, _per_channel(shift))
    return torch.relu(v) if relu else v


def post_ref64(case: Case, x, weight, bias, res, relu, ps, pt):
    """(v, y2) in float64: ``v = act(conv + bias + residual)``, ``y2 = relu(v * ps + pt)``."""
    v = R.epilogue64(R.conv_ref64(case, x, weight), bias, res, relu)
    return v, torch.relu(v * _per_channel(ps.double()) + _per_channel(pt.double()))


def pre_ref64(case: Case, x, sc, sh, weight, bias, res, relu):
    """The operand in float32 as specified, the convolution (1x1, stride s, no border) and the epilogue in float64."""
    assert (case.k, case.pad_lo, case.pad_hi) == (1, 0, 0)
    return R.epilogue64(R.conv_ref64(case, scale_shift_ref(x, sc, sh), weight), bias, res, relu)


def head_ref64(x, weight, bias, sc=None, sh=None):
    """``bias[o] + sum_c w[o][c] * pre(x[p][c])`` in float64 (``weight`` [cout, 64]); ``pre`` in float32 as specified, or the identity."""
    a = scale_shift_ref(x, sc, sh) if sc is not None else x
    out = torch.einsum("oc,nchw->nohw", weight.double().reshape(weight.shape[0], 64), a.double())
    if bias is not None:
        out = out + _per_channel(bias.double())
    return out.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------------------------------------
# references of the element-wise kernels: the specified sequence of float32 operations on the CPU, then ONE rounding
# ------------------------------------------------------------------------------------------------------------------------------------
def bias_act_ref(x, bias, res, relu: bool, *, round_before_residual: bool = False):
    """``act((x + b) + r)`` on the widened values, one ``.to(dtype)``.  ``round_before_residual``: the WRONG form that rounds
    ``x + b`` to the tensor's type first (for the tests of the comparison itself)."""
    v = x.float() + _per_channel(bias.float())
    if round_before_residual:
        v = v.to(x.dtype).float()
    if res is not None:
        v = v + res.float()
    if relu:
        v = torch.relu(v)
    return v.to(x.dtype)


def pool_ref(x, bias, *, first_row: int = -1):
    """``maxpool3x3/s2/p1(relu(x + b))``: window rows ``2 oy + first_row .. + 2``, columns ``2 ox - 1 .. 2 ox + 1``, cut at the map's
    edges; float32, one rounding.  ``first_row = 0`` is the WRONG window of the comparison's own test."""
    n, c, h, w = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    v = torch.relu(x.float() + _per_channel(bias.float()))
    top = -first_row
    padded = F.pad(v, (1, 2, top, 3 - top), value=float("-inf"))
    out = torch.full((n, c, ho, wo), float("-inf"))
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, padded[:, :, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2])
    return out.to(x.dtype).contiguous(memory_format=torch.channels_last)


def upsample_add_ref(x, y, scale=None, shift=None, *, source_offset: int = 0):
    """``out[Y, X] = x[Y / 2, X / 2] + y[Y, X]``, then ``relu(. * s + t)`` when given; each operation rounds once.
    ``source_offset = 1`` is the WRONG source pixel ``(Y + 1) / 2`` of the comparison's own test."""
    h, w = x.shape[2:]
    iy = ((torch.arange(2 * h) + source_offset) // 2).clamp_(max=h - 1)
    ix = ((torch.arange(2 * w) + source_offset) // 2).clamp_(max=w - 1)
    v = x[:, :, iy][:, :, :, ix] + y
    if scale is not None:
        v = scale_shift_ref(v, scale, shift, relu=True)
    return v.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------------------------------------------
def _as_direct(case: Case) -> Case:
    return case._replace(kernel="direct")


def make_data(case: Case, seed: int):
    """``_conv_ref.make_data`` (normal inputs and residual, He-scaled weights -- for thin by ``(2 / (c k k))^0.5``, the same rule --
    bias of 0.1 sigma) plus the per-channel vectors: ``ps``, ``pt`` over the outputs (POST), ``sc``, ``sh`` over the inputs (PRE, head).
    ``sh`` is positive for most channels, so that ``relu(sh) != 0``: the operand of a pixel that does not exist is not zero."""
    x, weight, bias, res = R.make_data(_as_direct(case), seed)
    g = torch.Generator().manual_seed(seed + 77)
    ps = 1.0 + 0.5 * torch.randn(case.cout, generator=g)
    pt = 0.3 * torch.randn(case.cout, generator=g)
    sc = 1.0 + 0.5 * torch.randn(case.cin, generator=g)
    sh = 0.5 + 0.5 * torch.randn(case.cin, generator=g)
    return {"x": x, "w": weight, "bias": bias, "res": res, "ps": ps, "pt": pt, "sc": sc, "sh": sh}


X_MAX, W_MAX, B_MAX, R_MAX = R.EXACT_RANGES["direct"]
PS_MAX, PT_MAX, SC_MAX, SH_MAX = 3, 8, 3, 4


def make_exact_data(case: Case, seed: int):
    """Integer data: inputs, weights, bias and residual as ``_conv_ref.EXACT_RANGES["direct"]``; ``ps`` in {1, 2, 3}, ``pt`` in -8 .. 8,
    ``sc`` in {-2, -1, 1, 2, 3}, ``sh`` in -4 .. 4."""
    x, weight, bias, res = R.make_exact_data(_as_direct(case), seed)
    rng = np.random.default_rng([seed, 99])
    as_f32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32))  # noqa: E731
    return {"x": x, "w": weight, "bias": bias, "res": res,
            "ps": as_f32(rng.integers(1, PS_MAX + 1, case.cout)), "pt": as_f32(rng.integers(-PT_MAX, PT_MAX + 1, case.cout)),
            "sc": as_f32(rng.choice([-2, -1, 1, 2, 3], case.cin)), "sh": as_f32(rng.integers(-SH_MAX, SH_MAX + 1, case.cin))}


def fused_exact_bound(case: Case, *, pre: bool | None = None) -> float:
    """Largest magnitude any product, partial sum or result can take with ``make_exact_data``: below 2^24 every float32 operation of
    the kernel is exact in any order (the head's 64 products and the sums of its butterfly are bounded by the full sum)."""
    a_max = X_MAX * SC_MAX + SH_MAX  # the activated operand
    if case.kernel == "post":
        v_max = case.k * case.k * case.cin * X_MAX * W_MAX + B_MAX + R_MAX
        return v_max * PS_MAX + PT_MAX
    if case.kernel == "pre":
        return case.cin * a_max * W_MAX + B_MAX + R_MAX
    if case.kernel == "thin":
        return case.k * case.k * case.cin * X_MAX * W_MAX + B_MAX
    if case.kernel == "head":
        return 64 * (a_max if pre is not False else X_MAX) * W_MAX + B_MAX
    assert case.kernel == "gvalid"
    return case.k * case.k * 32 * X_MAX * W_MAX


# integer data for the fp16 / bf16 element-wise kernels: sums beyond the integers half holds exactly, so ties and a second
# rounding show.  (x_max, bias_max, residual_max); every value is rounded to the type first (representable integers only).
HALF_ELEMENTWISE_RANGES = {"bfloat16": (256, 700, 1024), "float16": (2048, 6000, 8192)}


def make_half_integer_data(shape, dtype: str, seed: int):
    """(x, bias, residual) of ``dtype`` holding integers: ``x`` up to ``HALF_INTEGER_LIMIT`` (all representable), bias and residual larger."""
    dt = getattr(torch, dtype)
    x_max, b_max, r_max = HALF_ELEMENTWISE_RANGES[dtype]
    rng = np.random.default_rng([seed, 7])
    draw = lambda top, size: torch.from_numpy(rng.integers(-top, top + 1, size).astype(np.float32)).to(dt)  # noqa: E731
    x, bias, res = draw(x_max, shape), draw(b_max, shape[1]), draw(r_max, shape)
    assert x_max == R.HALF_INTEGER_LIMIT[dtype] and torch.equal(x.float(), x.float().round())
    return x, bias, res


# ------------------------------------------------------------------------------------------------------------------------------------
# comparisons: each raises AssertionError naming the case and the worst element (image, channel, row, column)
# ------------------------------------------------------------------------------------------------------------------------------------
def gate_of(kernel: str) -> str:
    return "abs" if kernel in ("post", "pre", "thin") else "rel"


def close_ratio(kernel: str, got: torch.Tensor, ref: torch.Tensor, *, scale: float = 1.0, per_element: float = 0.0):
    """(worst error relative to the gate, its index).  post / pre / thin: ``GATE_ABS * scale + per_element * |ref|`` per element;
    head / gvalid: ``GATE_REL`` of the largest reference magnitude."""
    assert got.shape == ref.shape and ref.dtype == torch.float64, (tuple(got.shape), tuple(ref.shape), ref.dtype)
    err = got.double().sub_(ref).abs_()
    if gate_of(kernel) == "abs":
        err.div_(ref.abs().mul_(per_element).add_(R.GATE_ABS * scale))
    else:
        err.div_(max(R.GATE_REL * float(ref.abs().max()), 1e-300))
    idx = R.worst_element(err)
    return float(err[idx]), idx


def check_close(label, kernel: str, got, ref, **gate) -> float:
    ratio, idx = close_ratio(kernel, got, ref, **gate)
    assert ratio <= 1.0, (f"{label}: error {ratio:.3g} x the gate at {WHERE} {idx}: got {float(got[idx])!r}, "
                          f"reference {float(ref[idx])!r}")
    return ratio


def check_equal(label, got: torch.Tensor, exp: torch.Tensor) -> None:
    """Equality by value of two tensors of one type (-0.0 equals +0.0)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (label, tuple(got.shape), tuple(exp.shape), got.dtype, exp.dtype)
    if torch.equal(got, exp):
        return
    wrong = got != exp
    idx = R.worst_element((got.double() - exp.double()).abs().nan_to_num(nan=float("inf")))
    msg = (f"{label}: {int(wrong.sum())} of {wrong.numel()} elements differ; worst at {WHERE} {idx}: got {float(got[idx])!r}, "
           f"expected {float(exp[idx])!r}")
    raise AssertionError(msg)


def check_exact(label, got: torch.Tensor, ref: torch.Tensor) -> None:
    """Bit for bit against a float64 reference that holds exact integers below 2^24."""
    assert ref.dtype == torch.float64 and torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2 ** 24, label
    check_equal(label, got, ref.float())


def one_hot_weights(cout: int, cin: int) -> tuple[torch.Tensor, torch.Tensor]:
    """OIHW 1x1 weights with a single 1 per output, at input channel ``picked[o]`` (distinct, drawn over all channel quads and slices): the
    convolution then returns the picked operand channels EXACTLY (every other product is a zero), so a PRE or head output equals
    ``relu(fl32(fl32(x * sc) + sh))`` bit for bit -- a comparison without a tolerance of how the operand is rounded."""
    assert cout <= cin
    picked = torch.randperm(cin, generator=torch.Generator().manual_seed(cin + cout))[:cout]
    weight = torch.zeros((cout, cin, 1, 1))
    weight[torch.arange(cout), picked] = 1.0
    return weight, picked


def fused_scale_shift(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """The WRONG operand of the comparisons' own test: ``relu(fl32(x * scale + shift))``, one rounding (a fused multiply-add)."""
    return torch.relu(x.double() * _per_channel(scale.double()) + _per_channel(shift.double())).float()


def y2_gate(ps: torch.Tensor) -> dict:
    """The POST output against float64: the slice kernel's gate scaled by the largest ``|ps|``, plus the two extra roundings."""
    return {"scale": max(1.0, float(ps.abs().max())), "per_element": 2.0 ** -23}


def relu_fractions(ref: torch.Tensor) -> tuple[float, float]:
    """(share of a ReLU'd reference that is positive, share that is clamped to zero)."""
    pos = float((ref > 0).double().mean())
    return pos, 1.0 - pos


def evaluate(case: Case, data, epilogue, *, pre: bool = True):
    """The float64 reference(s) of one case and epilogue: a tuple ``(v, y2)`` for post, a tensor otherwise."""
    use_bias, use_res, relu = epilogue
    bias, res = data["bias"] if use_bias else None, data["res"] if use_res else None
    if case.kernel == "post":
        return post_ref64(case, data["x"], data["w"], bias, res, relu, data["ps"], data["pt"])
    if case.kernel == "pre":
        return pre_ref64(case, data["x"], data["sc"], data["sh"], data["w"], bias, res, relu)
    if case.kernel == "head":
        return head_ref64(data["x"], data["w"], bias, *((data["sc"], data["sh"]) if pre else (None, None)))
    return R.epilogue64(R.conv_ref64(case, data["x"], data["w"]), bias, None, relu)


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 1: fixed edge cases
# ------------------------------------------------------------------------------------------------------------------------------------
def _post(n, cin, cout, h, w, k=1, stride=1, pad=(0, 0)):
    return Case("post", n, cin, cout, h, w, k=k, stride=stride, pad_lo=pad[0], pad_hi=pad[1])


def _pre(n, cin, cout, h, w, stride=1):
    return Case("pre", n, cin, cout, h, w, k=1, stride=stride, pad_lo=0, pad_hi=0)


POST_CASES = [
    # <64, POST>: cout 64 / 192 with any k; cout 128 with k = 1 and cin <= 256 (the narrow rule)
    _post(1, 32, 64, 1, 1),                               # 1 output pixel
    _post(1, 96, 192, 127, 1),                            # 127
    _post(2, 64, 128, 8, 8),                              # 128, narrow
    _post(3, 256, 128, 43, 1),                            # 129, narrow at the limit cin == 256
    _post(1, 64, 64, 9, 6, k=3, pad=(1, 1)),
    _post(2, 32, 192, 15, 22, k=3, stride=2, pad=(0, 1)),
    _post(1, 32, 64, 16, 24, k=3, pad=(1, 1)),            # 384 = 3 * 128
    _post(2, 96, 64, 11, 7, k=3, pad=(0, 0)),
    _post(3, 128, 192, 13, 20, stride=2),                 # 1x1 at stride 2
    # <128, POST>: cout 128 / 256 with k = 1 and cin 288 / 512; cout 128 / 256 with k = 3
    _post(1, 288, 128, 1, 1),                             # 1
    _post(1, 512, 256, 1, 127),                           # 127
    _post(2, 288, 256, 8, 8),                             # 128
    _post(3, 512, 128, 1, 43),                            # 129
    _post(1, 32, 128, 3, 3, k=3),                         # 1, h == w == k
    _post(2, 32, 128, 9, 6, k=3, pad=(1, 1)),
    _post(1, 64, 128, 13, 20, k=3, stride=2, pad=(0, 1)),
    _post(2, 32, 128, 11, 7, k=3, pad=(0, 0)),
    _post(1, 32, 256, 18, 30, k=3, stride=2, pad=(1, 1)),
    _post(2, 288, 128, 13, 20, stride=2),
    _post(1, 64, 128, 16, 24, k=3, pad=(1, 1)),           # 384
    _post(1, 96, 128, 5, 127, k=3, pad=(0, 0)),           # 3 x 125 = 375: a partial last tile with k = 3
]

PRE_CASES = [
    # <64, PRE>: cin <= 256 (k is always 1), or cout 64 / 192 with any cin
    _pre(1, 32, 64, 1, 1),                                # 1
    _pre(1, 96, 128, 127, 1),                             # 127
    _pre(2, 256, 256, 8, 8),                              # 128
    _pre(3, 64, 192, 1, 43),                              # 129
    _pre(2, 512, 64, 11, 16, stride=2),                   # cin > 256, cout 64
    _pre(1, 288, 192, 16, 11, stride=3),                  # cin > 256, cout 192; 16 % 3 = 1, 11 % 3 = 2
    _pre(1, 64, 64, 10, 15, stride=3),                    # 10 % 3 = 1, 15 % 3 = 0
    _pre(3, 32, 128, 7, 12, stride=2),
    _pre(1, 128, 64, 16, 16),                             # 256 = 2 * 128
    # <128, PRE>: cin 288, 512, 1024 with cout % 128 == 0
    _pre(1, 288, 128, 1, 1),                              # 1
    _pre(1, 512, 256, 1, 127),                            # 127
    _pre(2, 1024, 128, 8, 8),                             # 128
    _pre(3, 288, 256, 43, 1),                             # 129
    _pre(2, 512, 128, 13, 20, stride=2),                  # 13 % 2 = 1, 20 % 2 = 0
    _pre(1, 1024, 128, 14, 22, stride=3),                 # 14 % 3 = 2, 22 % 3 = 1
    _pre(2, 288, 128, 9, 5, stride=3),                    # 9 % 3 = 0, 5 % 3 = 2
    _pre(1, 512, 128, 16, 24),                            # 384
]

THIN_CK = [(3, 7), (1, 3), (1, 16), (2, 16), (4, 8), (4, 5), (3, 10)]


def _thin_cases() -> list[Case]:
    """Every (c, k) x stride x border; n, cout and the map cycle.  A small map (the wrapper's extra columns are needed unless
    c * k == 32) and a larger one alternate."""
    cases, i = [], 0
    for c, k in THIN_CK:
        borders = [(k // 2, k // 2), (0, 0), (0, 1)] + ([(2, 3)] if k >= 5 else [])  # noqa: PLR2004
        for stride in (1, 2, 3):
            for lo, hi in borders:
                small = i % 2 == 0
                h = max(k - lo - hi, 1) + (i % 3 if small else 9 + i % 5)
                w = max(k - lo - hi, 1) + ((i // 2) % 4 if small else 17 + i % 7)
                cases.append(Case("thin", (1, 3)[i % 2], c, (64, 128, 192)[i % 3], h, w, k=k, stride=stride, pad_lo=lo, pad_hi=hi))
                i += 1
    return cases


HEAD_PIXELS = {1: (1, 1, 1), 2: (1, 1, 2), 3: (1, 3, 1), 4: (2, 2, 1), 5: (1, 1, 5), 15: (1, 3, 5), 16: (2, 2, 4), 17: (1, 17, 1),
               63: (1, 7, 9), 64: (2, 4, 8), 65: (1, 5, 13), 255: (3, 5, 17), 256: (2, 8, 16), 257: (1, 1, 257)}


def _head_cases() -> list[Case]:
    return [Case("head", n, 64, cout, h, w, k=1, pad_lo=0, pad_hi=0) for (n, h, w) in HEAD_PIXELS.values() for cout in range(1, 9)]


GVALID_GROUPS, GVALID_K = (1, 2, 3, 4, 7), (1, 3, 5, 7)


def _gvalid_shapes(k: int):
    """(n, h, w): 1 x 1, 1 x W and H x 1 outputs (h == k and / or w == k); 255, 256 and 257 output pixels; a plain rectangle."""
    return [(1, k, k), (3, k, k + 16), (2, k + 8, k), (3, k + 4, k + 16), (1, k + 15, k + 15), (1, k, k + 256), (2, k + 5, k + 8)]


def _gvalid_cases() -> list[Case]:
    cases = []
    for i, (groups, k) in enumerate(itertools.product(GVALID_GROUPS, GVALID_K)):
        shapes = _gvalid_shapes(k)
        for n, h, w in (shapes[i % 7], shapes[(i + 3) % 7], shapes[(i + 5) % 7]):
            cases.append(Case("gvalid", n, groups * 32, groups * 8, h, w, k=k, pad_lo=0, pad_hi=0, groups=groups))
    return cases


def fixed_cases(kernel: str) -> list[Case]:
    return {"post": lambda: POST_CASES, "pre": lambda: PRE_CASES, "thin": _thin_cases, "head": _head_cases,
            "gvalid": _gvalid_cases}[kernel]()


# element-wise kernels: (n, c, h, w)
SCALE_SHIFT_SHAPES = [(1, 4, 1, 1), (1, 8, 1, 1), (1, 96, 1, 1), (1, 2048, 1, 1), (2, 4, 5, 7), (3, 8, 7, 5), (2, 96, 9, 4), (1, 2048, 3, 2)]
# views of a wider buffer: (buffer [n, C, H, W], channels c of the prefix, first row, first column, rows, columns)
SCALE_SHIFT_VIEWS = [((2, 24, 6, 9), 8, 1, 2, 4, 5),      # prefix + crop with a base offset, n > 1, pixel stride 24 > 8
                     ((1, 96, 7, 5), 96, 2, 1, 3, 3),     # every channel, crop only
                     ((3, 16, 4, 6), 4, 0, 0, 4, 6),      # prefix only: pixel stride 16 > 4, no crop
                     ((2, 2052, 3, 4), 2048, 1, 1, 1, 2),  # 512 vectors per pixel, one row
                     ((2, 8, 5, 5), 4, 4, 4, 1, 1)]       # one pixel per image: the last of the buffer
# (n, c, h, w) of the low-resolution input; the cropped skip sits at (row 1, column 3) of a [2h + 3, 2w + 4] map
UPSAMPLE_SHAPES = [(1, 4, 1, 5), (2, 8, 5, 1), (1, 4, 1, 1), (3, 16, 3, 7), (2, 64, 6, 4), (3, 4, 2, 2)]
UPSAMPLE_CROP = (1, 3, 3, 4)  # first row, first column, extra rows, extra columns
BIAS_ACT_SHAPES = [(2, 8, 5, 7), (1, 8, 1, 1), (3, 24, 3, 2), (1, 24, 1, 9), (2, 64, 4, 5), (1, 64, 1, 1)]
POOL_HW = [(h, w) for h in (1, 2, 3, 4, 5) for w in (1, 2, 7, 8)]
POOL_CHANNELS = (8, 24, 64)
DTYPES = ("float32", "float16", "bfloat16")


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 2: seeded random cases (only what each entry point documents as served)
# ------------------------------------------------------------------------------------------------------------------------------------
RANDOM_SEED = 20261017
RANDOM_COUNT = {"post": 32, "pre": 32, "thin": 28, "head": 24, "gvalid": 28}
TILE_FLOOR = 4  # cases with h != w per tile width in the random draw of post and pre


def random_cases(kernel: str) -> list[Case]:
    rng = np.random.default_rng([RANDOM_SEED, CONV_KERNELS.index(kernel)])
    cases = []
    for i in range(RANDOM_COUNT[kernel]):
        n = int(rng.integers(1, 6))
        if kernel == "post":
            k = int(rng.choice([1, 3]))
            stride = int(rng.integers(1, 3))
            lo, hi = ((0, 0), (1, 1), (0, 1), (1, 0))[int(rng.integers(0, 4))] if k == 3 else (0, 0)  # noqa: PLR2004
            cin = 32 * int(rng.integers(1, 5)) if i % 2 else int(rng.choice([288, 320, 512]))
            cout = 64 * int(rng.integers(1, 5))
            h, w = int(rng.integers(k, 28)), int(rng.integers(k, 28))
            cases.append(_post(n, cin, cout, h, w, k=k, stride=stride, pad=(lo, hi)))
        elif kernel == "pre":
            cin = 32 * int(rng.integers(1, 9)) if i % 2 else int(rng.choice([288, 512, 1024]))
            cases.append(_pre(n, cin, 64 * int(rng.integers(1, 5)), int(rng.integers(1, 28)), int(rng.integers(1, 28)),
                              stride=int(rng.integers(1, 4))))
        elif kernel == "thin":
            c = int(rng.integers(1, 5))
            k = int(rng.integers(1, min(32 // c, 16) + 1))
            lo = int(rng.integers(0, min(k, 4)))
            hi = int(rng.integers(0, min(k, 4)))
            h, w = max(k - lo - hi, 1) + int(rng.integers(0, 24)), max(k - lo - hi, 1) + int(rng.integers(0, 40))
            cases.append(Case("thin", n, c, 64 * int(rng.integers(1, 4)), h, w, k=k, stride=int(rng.integers(1, 4)), pad_lo=lo, pad_hi=hi))
        elif kernel == "head":
            cases.append(Case("head", n, 64, i % 8 + 1, int(rng.integers(1, 60)), int(rng.integers(1, 60)), k=1, pad_lo=0, pad_hi=0))
        else:
            groups, k = int(rng.integers(1, 9)), int(rng.integers(1, 8))
            cases.append(Case("gvalid", n, groups * 32, groups * 8, k + int(rng.integers(0, 24)), k + int(rng.integers(0, 24)), k=k,
                              pad_lo=0, pad_hi=0, groups=groups))
    return cases


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 3: the exact tier's cases
# ------------------------------------------------------------------------------------------------------------------------------------
def exact_cases(kernel: str) -> list[Case]:
    cases = fixed_cases(kernel)
    if kernel in ("post", "pre"):
        return cases
    if kernel == "head":
        return [c for c in cases if c.n * c.h * c.w in (1, 3, 5, 17, 64, 255, 257)]
    return cases[::2] + cases[1::6]


def served(case: Case) -> bool:
    """What the case's entry point documents as served (shape conditions only)."""
    ok = case.n >= 1 and case.h >= 1 and case.w >= 1 and case.ho >= 1 and case.wo >= 1 and case.stride >= 1
    if case.kernel in ("post", "pre", "thin"):
        ok = ok and case.cout % 64 == 0 and case.k <= 16 and case.pad_lo < case.k and case.pad_hi < case.k  # noqa: PLR2004
        ok = ok and (case.ho - 1) * case.stride - case.pad_lo < case.h and (case.wo - 1) * case.stride - case.pad_lo < case.w
    if case.kernel in ("post", "pre"):
        ok = ok and case.cin % 32 == 0
    if case.kernel == "pre":
        ok = ok and (case.k, case.pad_lo, case.pad_hi) == (1, 0, 0)
    if case.kernel == "thin":
        ok = ok and case.cin * case.k <= 32  # noqa: PLR2004
    if case.kernel == "head":
        ok = ok and case.cin == 64 and 1 <= case.cout <= 8 and case.k == 1  # noqa: PLR2004
    if case.kernel == "gvalid":
        ok = ok and case.cin == 32 * case.groups and case.cout == 8 * case.groups and (case.stride, case.pad_lo, case.pad_hi) == (1, 0, 0)
        ok = ok and case.h >= case.k and case.w >= case.k
    return ok


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 4: the batch split of conv2d_impl for POST and PRE
# ------------------------------------------------------------------------------------------------------------------------------------
SPLIT_CASES = {"post": _post(129, 1024, 128, 64, 64), "pre": _pre(129, 1024, 64, 64, 64)}
SPLIT_CHUNK = 43  # three sub-batches that need no split

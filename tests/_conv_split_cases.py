"""Shared by ``test_conv_split.py`` (host) and ``test_conv_split_gpu.py``: a torch emulation of the arithmetic of
``conv_ring_bf16x3_kernel``, a restatement of the packed weight layout, and the builders of the EXACT cases -- inputs
whose result involves no rounded sum, so that kernel and emulation must both give it bit for bit.

The emulation: both operands split into three bf16 numbers (``split_stem_weights``: round to nearest even, exact float32
subtractions -- the kernel's instruction sequence on the activations), the reduction in the kernel's order (tap row, tap column,
16-channel slice), and per slice six matrix products into one accumulator in the kernel's order.  Every product of two parts is exact;
one product-sum step ``acc + sum_16 a_i w_j`` is evaluated in float64 and rounded to float32 once.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F  # noqa: N812

from tiatoolbox_amd.models.architecture.fused import split_stem_weights

# (activation part, weight part) of the six products of a slice, in the kernel's order: lo hi, hi lo, mid mid, mid hi, hi mid, hi hi
ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
DROPPED = ((1, 2), (2, 1), (2, 2))

# kernel / stride / padding of the GPU file's shapes
GEOMETRIES = ((1, 1, 0), (1, 2, 0), (3, 2, 1), (3, 1, 0), (3, 1, 1), (3, 1, 2), (5, 2, 2))


def emulate_gemm(a: torch.Tensor, w: torch.Tensor, *, terms=ORDER, fp64_accumulate: bool = False) -> torch.Tensor:
    """``a [M, K] @ w [K, N]`` (float32, K % 16 == 0) the kernel's way.  ``fp64_accumulate``: no rounding at all between the steps
    (what is left is the error of the terms that are not in ``terms``)."""
    ap, wp = split_stem_weights(a)[0].double(), split_stem_weights(w)[0].double()
    acc = torch.zeros((a.shape[0], w.shape[1]), dtype=torch.float64)
    for k0 in range(0, a.shape[1], 16):
        for i, j in terms:
            acc = acc + ap[i][:, k0:k0 + 16] @ wp[j][k0:k0 + 16]  # 16 exact products, summed in float64
            if not fp64_accumulate:
                acc = acc.float().double()
    return acc if fp64_accumulate else acc.float()


def im2col(x: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    """NCHW ``x`` -> ``[n * ho * wo, k * k * cin]`` with the reduction index ordered (tap row, tap column, channel): a 16-channel slice of
    a tap is 16 consecutive columns, as in the kernel."""
    n, c, h, w = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    cols = [xp[:, :, ty:ty + (ho - 1) * stride + 1:stride, tx:tx + (wo - 1) * stride + 1:stride] for ty in range(k) for tx in range(k)]
    return torch.stack(cols, 1).permute(0, 3, 4, 1, 2).reshape(n * ho * wo, k * k * c)


def emulate_conv(x: torch.Tensor, weight: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    """The kernel's arithmetic for ``conv2d(x, weight)`` (no bias), NCHW float32."""
    n, _, h, w = x.shape
    cout = weight.shape[0]
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    b = weight.permute(2, 3, 1, 0).reshape(-1, cout)  # (tap row, tap column, channel) x cout
    return emulate_gemm(im2col(x, k, stride, pad), b).reshape(n, ho, wo, cout).permute(0, 3, 1, 2).contiguous()


def packed_index(cout: int, cin: int, kh: int, kw: int) -> torch.Tensor:
    """For every element of the packed tensor ``[kh, kw, cin/16, cout/128, 3, 2, 128, 8]`` (tap row, tap column, 16-channel slice,
    128-column tile, plane, 8-channel k-chunk, column, channel) the flat index of its source in ``parts [3, cout, cin, kh, kw]``."""
    ty, tx, cs, ct, p, q, c, e = torch.meshgrid(*(torch.arange(s) for s in (kh, kw, cin // 16, cout // 128, 3, 2, 128, 8)), indexing="ij")
    o, ch = 128 * ct + c, 16 * cs + 8 * q + e
    return (((p * cout + o) * cin + ch) * kh + ty) * kw + tx


def full_mantissa(shape, gen: torch.Generator, *, exp_lo: int = 120, exp_hi: int = 134) -> torch.Tensor:
    """Float32 values with 23 random mantissa bits, a random sign and a biased exponent in ``[exp_lo, exp_hi]``."""
    mant = torch.randint(0, 1 << 23, shape, generator=gen, dtype=torch.int32)
    expo = torch.randint(exp_lo, exp_hi + 1, shape, generator=gen, dtype=torch.int32)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int32)
    return (mant | (expo << 23) | (sign * -(1 << 31))).view(torch.float32)


def _reference(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """float64 convolution; for the exact cases it IS the result (every sum it forms is exact), so its float32 value is the expected one."""
    y = F.conv2d(x.double(), w.double(), None, stride, pad)
    assert torch.equal(y.float().double(), y), "not an exact case: the reference itself needs more than float32"
    return y.float()


def case_single_tap(k: int, stride: int, pad: int, *, n: int = 5, cin: int = 48, cout: int = 128, seed: int = 0):
    """(i) One non-zero weight +-2^e per output channel (channel ``o`` takes tap ``o % k^2`` and input channel ``(7 o) % cin``),
    activations with random full 24-bit significands: the output is the shifted input value."""
    g = torch.Generator().manual_seed(1000 + seed + 10 * k + stride + 3 * pad)
    x = full_mantissa((n, cin, 19, 13), g)
    w = torch.zeros((cout, cin, k, k))
    for o in range(cout):
        tap = o % (k * k)
        w[o, (7 * o) % cin, tap // k, tap % k] = (-1.0) ** o * 2.0 ** ((o % 13) - 6)
    return x, w, _reference(x, w, stride, pad)


def case_power_of_two_activations(k: int, stride: int, pad: int, *, n: int = 3, cin: int = 48, cout: int = 128, seed: int = 0):
    """(ii) Activations zero except isolated pixels (a grid of pitch max(k, 2): no output window holds two) with a power of two in one
    channel, weights with random full significands: every output is one scaled weight (or zero)."""
    g = torch.Generator().manual_seed(2000 + seed + 10 * k + stride + 3 * pad)
    x = torch.zeros((n, cin, 19, 13))
    pitch = max(k, 2)
    for b in range(n):
        for yy in range(b % pitch, 19, pitch):
            for xx in range((b + 1) % pitch, 13, pitch):
                c = int(torch.randint(0, cin, (1,), generator=g))
                e = int(torch.randint(-8, 9, (1,), generator=g))
                x[b, c, yy, xx] = (-1.0) ** (yy + xx) * 2.0 ** e
    w = full_mantissa((cout, cin, k, k), g, exp_lo=115, exp_hi=125)
    return x, w, _reference(x, w, stride, pad)


def case_mid_mid(k: int, stride: int, pad: int, *, n: int = 3, cin: int = 16, cout: int = 128):
    """(iii) a = 1 + 2^-10 in isolated pixels of one channel, w = 1 + 2^-10 at every tap of that channel: hi = 1, mid = 2^-10, and the
    output 1 + 2^-9 + 2^-20 needs hi hi, hi mid, mid hi AND mid mid."""
    v = 1.0 + 2.0 ** -10
    x = torch.zeros((n, cin, 19, 13))
    pitch = max(k, 2)
    x[:, 5, 0::pitch, 0::pitch] = v
    w = torch.zeros((cout, cin, k, k))
    w[:, 5] = v
    ref = _reference(x, w, stride, pad)
    assert set(ref.unique().tolist()) <= {0.0, 1.0 + 2.0 ** -9 + 2.0 ** -20} and ref.max() > 1
    return x, w, ref


def case_integers(k: int = 3, stride: int = 2, pad: int = 1, *, n: int = 5, cin: int = 48, cout: int = 256, seed: int = 0):
    """(iv) Integer activations in [-2048, 2047] (about one in twelve non-zero, like a sparse ReLU map), integer weights in
    [-400, 400]; K = k^2 cin = 432 is chosen with that density so that sum |a| |w| < 2^24 for every output: every partial sum in
    ANY order is an integer below 2^24, i.e. exact.  Accumulation across taps, slices and padding."""
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.randint(-2048, 2048, (n, cin, 19, 13), generator=g).float()
    x = x * (torch.rand((n, cin, 19, 13), generator=g) < 1.0 / 12).float()
    w = torch.randint(-400, 401, (cout, cin, k, k), generator=g).float()
    bound = F.conv2d(x.abs().double(), w.abs().double(), None, stride, pad).max().item()
    assert bound < 2 ** 24, bound
    return x, w, _reference(x, w, stride, pad)

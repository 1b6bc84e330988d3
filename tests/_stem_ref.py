"""Host-only helpers of ``tests/test_stem_reference.py``: the float64 reference of the ResNet stem (``csrc/stem_mfma.hip``) on exactly
the operands each variant multiplies, the any-order float32 summation bound, the launch geometry of ``stem_impl`` restated in Python
(strips, row chunks, batch groups, V-tile path per wave), the case lists, and the deliberately wrong references of the sensitivity
test.  Nothing here touches a device, so all of it is exercised on a CPU-only checkout."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F  # noqa: N812

from _conv_ref import HALF_EPS, worst_element

# ------------------------------------------------------------------------------------------------------------------------------------
# variants: the grid of the device tests
# ------------------------------------------------------------------------------------------------------------------------------------
ARITHMETICS = ("f32", "float16", "bfloat16", "split")


class Variant(NamedTuple):
    """``arith``: f32 (float32 MFMA) / float16 / bfloat16 (half MFMA) / split (bf16 x 3); ``x_u8``: uint8 or float32 input; ``out``: type
    of the pooled output; ``conv``: a pre-pool output (of type ``out``) is wanted too."""

    arith: str
    x_u8: bool
    out: str
    conv: bool

    @property
    def name(self) -> str:
        return f"{self.arith}/{'u8' if self.x_u8 else 'f32'}->{self.out}{'+conv' if self.conv else ''}"


def variant_grid() -> list[Variant]:
    grid = [Variant("f32", u8, out, conv) for u8 in (True, False) for out in ("float32", "float16", "bfloat16") for conv in (False, True)]
    grid += [Variant(dt, u8, dt, False) for dt in ("float16", "bfloat16") for u8 in (True, False)]
    return [*grid, Variant("split", True, "float32", False)]


# accumulated terms per output: 147 taps + the zero row; 7 * 24 = 168 padded to 176; three planes of 176
K_TERMS = {"f32": 148, "float16": 176, "bfloat16": 176, "split": 3 * 176}
U = 2.0 ** -24  # unit roundoff of float32


# ------------------------------------------------------------------------------------------------------------------------------------
# reference and bound
# ------------------------------------------------------------------------------------------------------------------------------------
def _arith(variant) -> str:
    return variant.arith if isinstance(variant, Variant) else variant


def stem_operands(x: torch.Tensor, weight: torch.Tensor, variant):
    """(input NCHW float64, weight float64, divisor): exactly the values the kernel multiplies, widened.  ``x``: NHWC uint8 (scaled by
    1 / 255 on load) or float32 (as is)."""
    arith = _arith(variant)
    assert x.dtype in (torch.uint8, torch.float32) and x.dim() == 4 and x.shape[-1] == 3, (x.dtype, tuple(x.shape))  # noqa: PLR2004
    w32 = weight.detach().float()
    if arith == "split":  # the bytes themselves and the float32 weights: conv = S / 255 + bias
        assert x.dtype == torch.uint8
        return x.double().permute(0, 3, 1, 2), w32.double(), 255.0
    xv = x.float().div(255) if x.dtype == torch.uint8 else x
    if arith != "f32":  # rounded ONCE to the half type, inputs and weights
        dt = getattr(torch, arith)
        xv, w32 = xv.to(dt), w32.to(dt)
    return xv.double().permute(0, 3, 1, 2), w32.double(), 1.0


def stem_ref64(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, variant):
    """``(conv64, pooled64)``: convolution 7x7 / stride 2 / padding 3 in float64 + bias + ReLU, and its 3x3 / stride 2 / padding 1
    maximum."""
    x64, w64, div = stem_operands(x, weight, variant)
    lin = F.conv2d(x64, w64, None, 2, 3)
    if div != 1.0:
        lin = lin / div
    conv64 = torch.relu_(lin + bias.detach().double().view(1, -1, 1, 1))
    return conv64, F.max_pool2d(conv64, 3, 2, 1)


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def stem_bound(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, variant, conv64: torch.Tensor | None = None):
    """``(B_conv, B_pooled)`` in float64 for a FLOAT32 output: ``gamma(K + 1) * (conv64(|x|, |w|) + |bias|)``, the bound of a float32 sum
    of K terms taken in any order plus the addition of the bias; the split variant adds ``2 u |ref|`` for its rounded quotient
    (``conv64`` is then required).  ReLU and the maximum are 1-Lipschitz: the pooled bound is the maximum of the window's bounds."""
    arith = _arith(variant)
    x64, w64, div = stem_operands(x, weight, variant)
    mag = F.conv2d(x64.abs_(), w64.abs_(), None, 2, 3)
    if div != 1.0:
        mag = mag / div
    b = (mag + bias.detach().double().abs().view(1, -1, 1, 1)).mul_(gamma(K_TERMS[arith] + 1))
    if arith == "split":
        assert conv64 is not None
        b = b + 2.0 * U * conv64.abs()
    return b, F.max_pool2d(b, 3, 2, 1)


def output_bound(b: torch.Tensor, ref: torch.Tensor, out: str) -> torch.Tensor:
    """The bound of an output of type ``out``: a half output adds half an ulp of the reference, fp16 below its normal range the
    half spacing of its subnormals."""
    if out == "float32":
        return b
    tot = b + 0.5 * HALF_EPS[out] * ref.abs()
    if out == "float16":
        tot = tot + (ref.abs() < 2.0 ** -14).double() * 2.0 ** -25
    return tot


def bound_ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor):
    """(max err / bound, index of that element); a NaN is the worst element."""
    assert got.shape == ref.shape == bound.shape, (tuple(got.shape), tuple(ref.shape), tuple(bound.shape))
    ratio = got.double().sub_(ref).abs_().div_(bound.clamp_min(1e-300))
    idx = worst_element(ratio)
    r = float(ratio[idx])
    return (float("inf") if r != r else r), idx  # noqa: PLR0124


def make_data(n: int, h: int, w: int, seed: int, bias_shift: float = 0.0):
    """Random bytes, weights N(0, 0.05), bias N(0, 0.1) (the data of ``test_stem_gpu._stem_parts``) + ``bias_shift``."""
    g = torch.Generator().manual_seed(seed)
    weight = torch.randn((64, 3, 7, 7), generator=g) * 0.05
    bias = torch.randn(64, generator=g) * 0.1 + bias_shift
    x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    return x, weight, bias


def make_exact_data(n: int, h: int, w: int, seed: int):
    """Integer tier: float32 inputs 0 .. 15, weights -8 .. 8, bias -64 .. 64: |any partial sum| <= 147 * 15 * 8 + 64 < 2^24."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(0, 16, (n, h, w, 3)).astype(np.float32))
    weight = torch.from_numpy(rng.integers(-8, 9, (64, 3, 7, 7)).astype(np.float32))
    bias = torch.from_numpy(rng.integers(-64, 65, 64).astype(np.float32))
    return x, weight, bias


def make_onehot_data(n: int, h: int, w: int, seed: int):
    """One tap ``(c, ky, kx)`` per output channel with weight +-2^k (k in -4 .. 3), no bias, random bytes: every convolution value is
    ONE exact product ``fl(b / 255) * w`` (half stems: of the operand rounded to half)."""
    rng = np.random.default_rng(seed)
    weight = torch.zeros((64, 3, 7, 7))
    for o in range(64):
        c, ky, kx = int(rng.integers(0, 3)), int(rng.integers(0, 7)), int(rng.integers(0, 7))
        weight[o, c, ky, kx] = float(rng.choice([-1.0, 1.0])) * 2.0 ** int(rng.integers(-4, 4))
    x = torch.from_numpy(rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8))
    return x, weight, torch.zeros(64)


def onehot_expected(x_u8: torch.Tensor, weight: torch.Tensor, variant: Variant, *, reciprocal: bool = False):
    """(conv, pooled) of the one-hot tier in the OUTPUT type, bit for bit: float64 holds the single product exactly, one rounding to
    a half output.  ``reciprocal=True`` is the wrong staging ``x * fl(1 / 255)`` of the sensitivity test."""
    if reciprocal:
        x = x_u8.float() * torch.tensor(1.0, dtype=torch.float32).div(255)
    else:
        x = x_u8.float().div(255)
    conv64, pooled64 = stem_ref64(x, weight, torch.zeros(64), variant.arith)
    assert torch.equal(conv64.float().double(), conv64)  # one product of a 24-bit and a 1-bit mantissa
    dt = getattr(torch, variant.out)
    return conv64.float().to(dt), pooled64.float().to(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# launch geometry of stem_impl / stem7x7_pool_body
# ------------------------------------------------------------------------------------------------------------------------------------
INT_MAX = 0x7FFFFFFF


class Strip(NamedTuple):
    p0: int       # pooled columns [p0, p1)
    p1: int
    c_start: int  # conv columns [c_start, c_start + ncols)
    ncols: int

    def wave_columns(self) -> list[int]:
        """Valid conv columns of each of the four waves (32 columns each)."""
        return [min(32, max(0, self.ncols - 32 * wv)) for wv in range(4)]


class Launch(NamedTuple):
    first: int           # first image of the group
    nb: int              # images of the group
    chunks: int          # row chunks per image
    rows_per_chunk: int  # pooled rows per chunk
    x_shift: int         # uint8: bytes between the dword-aligned buffer base and the group's first image


class Geometry(NamedTuple):
    n: int
    h: int
    w: int
    ho: int
    wo: int
    hp: int
    wp: int
    strips: tuple[Strip, ...]
    group: int
    launches: tuple[Launch, ...]


def even_group(n: int, max_group: int) -> int:
    """``tia::even_group``: equal groups of at most ``max_group`` images."""
    if max_group < 1 or n <= max_group:
        return max_group
    k = (n + max_group - 1) // max_group
    return (n + k - 1) // k


def stem_geometry(n: int, h: int, w: int, *, x_u8: bool = True, base: int = 0) -> Geometry:
    """What ``stem_impl`` launches for ``n`` images of ``h x w`` whose first byte is at address ``base``."""
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    image_bytes = h * w * 3 * (1 if x_u8 else 4)
    assert image_bytes <= INT_MAX
    group = even_group(n, min(INT_MAX // image_bytes, INT_MAX // (h * w * 3)))
    nstrips = 1 if wp <= 64 else 1 + (wp - 64 + 62) // 63  # noqa: PLR2004
    strips = []
    for s in range(nstrips):
        p0 = 0 if s == 0 else 64 + 63 * (s - 1)
        p1 = min(wp, 64 if s == 0 else p0 + 63)
        c_start = max(0, 2 * p0 - 1)
        strips.append(Strip(p0, p1, c_start, min(wo, 2 * p1) - c_start))
    launches = []
    for first in range(0, n, group):
        nb = min(group, n - first)
        chunks = (1024 + nb * nstrips - 1) // (nb * nstrips)
        chunks = max(1, min(chunks, hp // 8 if hp >= 8 else 1))  # noqa: PLR2004
        rows = (hp + chunks - 1) // chunks
        chunks = (hp + rows - 1) // rows
        launches.append(Launch(first, nb, chunks, rows, (base + first * image_bytes) % 4 if x_u8 else 0))
    return Geometry(n, h, w, ho, wo, hp, wp, tuple(strips), group, tuple(launches))


def chunk_rows(geom: Geometry, launch: Launch) -> list[tuple[int, int]]:
    """Pooled rows [q0, q1) of each chunk of a launch."""
    return [(c * launch.rows_per_chunk, min(geom.hp, (c + 1) * launch.rows_per_chunk)) for c in range(launch.chunks)]


def vtile_paths(geom: Geometry, *, conv_out: bool, split: bool = False) -> set[str]:
    """Which V-tile paths the waves of the launches take: ``fast`` when both conv rows of the iteration and all 32 columns of the wave
    are on the map and no pre-pool output is wanted (the split variant never has one), else ``slow`` -- per (strip, wave, iteration,
    warm-up iterations included)."""
    paths = set()
    for launch in geom.launches:
        for q0, q1 in chunk_rows(geom, launch):
            for py in range(max(q0 - 1, 0), q1):
                both_rows = 2 * py + 1 < geom.ho
                for strip in geom.strips:
                    for cols in strip.wave_columns():
                        paths.add("fast" if both_rows and cols == 32 and (split or not conv_out) else "slow")  # noqa: PLR2004
    return paths


# ------------------------------------------------------------------------------------------------------------------------------------
# case lists: (n, h, w)
# ------------------------------------------------------------------------------------------------------------------------------------
SEAM_WIDTHS = [*range(253, 263), *range(505, 519), *range(757, 763)]
TINY_WIDTHS = [1, 2, 3, 5, 6, 7, 8, 9, 13]
TINY_HEIGHTS = [1, 2, 7, 9]
SWEEP_HEIGHTS = [*range(1, 9), *range(57, 73), *range(125, 137)]

WIDTH_CASES = [(2, 10, w) for w in SEAM_WIDTHS] + [(2, h, w) for w in TINY_WIDTHS for h in TINY_HEIGHTS]
HEIGHT_CASES = [(n, h, w) for h in SWEEP_HEIGHTS for w in (9, 66) for n in (1, 3)]
COMBINATION_CASES = [(1024, 57, 9), (1100, 64, 8), (1, 131, 258), (1, 70, 600)]
ALL_CASES = WIDTH_CASES + HEIGHT_CASES + COMBINATION_CASES

ALIGN_CASES = [(2, 10, w, off) for w in (257, 259, 509) for off in (0, 1, 2, 3)]  # uint8 batches `off` bytes off a dword
WINDOW_CASES = [(1, 70, 600), (1, 131, 258), (3, 66, 509)]
BIG_F32 = (171, 1024, 1024)   # float32 input: 2.15 GB, two groups of 86 / 85 images
BIG_U8 = (11009, 255, 255)    # uint8 input with odd image bytes: two groups of 5505 / 5504 images, the second 3 bytes off a dword


def case_seed(n: int, h: int, w: int) -> int:
    return 100_000 * (n % 97) + 1000 * h + w


# ------------------------------------------------------------------------------------------------------------------------------------
# window-position codes (every conv pixel of every window reaches the pooled output)
# ------------------------------------------------------------------------------------------------------------------------------------
def window_code_map(n: int, h: int, w: int, phase: tuple[int, int], axis: int):
    """(conv map [n, ho, wo] float32, expected pooled map [n, hp, wp], mask of the pooled pixels whose own conv pixel exists).  Only conv
    pixels ``(2 p + a, 2 q + b)`` are non-zero; they carry a code of ``p`` (``axis == 0``) or of ``q`` (``axis == 1``): increasing for
    phase 0 / +1 and decreasing for phase -1, so that a window's own pixel beats the neighbour's on the row or column they share."""
    a, b = phase
    geom = stem_geometry(n, h, w)
    p = torch.arange(geom.hp).view(-1, 1).expand(geom.hp, geom.wp)
    q = torch.arange(geom.wp).view(1, -1).expand(geom.hp, geom.wp)
    idx, ph = (p, a) if axis == 0 else (q, b)
    code = (250 - idx if ph < 0 else 1 + idx).float()
    cy, cx = 2 * p + a, 2 * q + b
    ok = (cy >= 0) & (cy < geom.ho) & (cx >= 0) & (cx < geom.wo)
    conv = torch.zeros((geom.ho, geom.wo))
    conv[cy[ok], cx[ok]] = code[ok]
    pooled = F.max_pool2d(conv[None, None], 3, 2, 1)[0, 0]
    assert float(code.min()) >= 1 and float(code.max()) <= 250  # noqa: PLR2004  (bf16 holds every integer up to 256)
    return conv.expand(n, -1, -1), pooled.expand(n, -1, -1), ok


def window_input(conv_map: torch.Tensor, h: int, w: int, *, as_bytes: bool) -> torch.Tensor:
    """NHWC input under a unit centre tap on channel 0: conv pixel ``(cy, cx)`` is input sample ``(2 cy, 2 cx)``."""
    n = conv_map.shape[0]
    x = torch.zeros((n, h, w, 3))
    x[:, ::2, ::2, 0] = conv_map
    return x.to(torch.uint8) if as_bytes else x


def window_weight(value: float) -> torch.Tensor:
    weight = torch.zeros((64, 3, 7, 7))
    weight[:, 0, 3, 3] = value
    return weight


# ------------------------------------------------------------------------------------------------------------------------------------
# wrong references (sensitivity): each must fail the comparison that guards it
# ------------------------------------------------------------------------------------------------------------------------------------
def wrong_tap_dropped(x, weight, bias, variant, tap=(5, 2, 1)):
    ky, kx, c = tap
    w2 = weight.clone()
    w2[:, c, ky, kx] = 0.0
    return stem_ref64(x, w2, bias, variant)


def wrong_taps_transposed(x, weight, bias, variant):
    return stem_ref64(x, weight.transpose(2, 3).contiguous(), bias, variant)


def wrong_carried_row_missing(conv64: torch.Tensor, geom: Geometry) -> torch.Tensor:
    """The pooled map with conv row ``2 p - 1`` left out of the window at the first pooled row ``p`` of every chunk but the first."""
    pooled = F.max_pool2d(conv64, 3, 2, 1)
    firsts = {q0 for launch in geom.launches for q0, _ in chunk_rows(geom, launch) if q0 > 0}
    assert firsts
    for p in firsts:
        rows = conv64[:, :, 2 * p:2 * p + 2]
        pooled[:, :, p] = F.max_pool2d(rows, (rows.shape[2], 3), (2, 2), (0, 1))[:, :, 0]
    return pooled


def wrong_strip_column_zeroed(conv64: torch.Tensor, geom: Geometry, *, last: bool) -> torch.Tensor:
    """The pooled map after zeroing the first (``c_start``) or the last (``c_start + ncols - 1``) conv column of every non-first strip."""
    assert len(geom.strips) > 1
    c2 = conv64.clone()
    for strip in geom.strips[1:]:
        c2[..., strip.c_start + strip.ncols - 1 if last else strip.c_start] = 0.0
    return F.max_pool2d(c2, 3, 2, 1)


def wrong_bias_after_half_rounding(x, weight, bias, variant, out: str) -> torch.Tensor:
    """A half pooled output whose convolution was rounded to half BEFORE the bias: two roundings instead of one."""
    dt = getattr(torch, out)
    x64, w64, div = stem_operands(x, weight, variant)
    lin = (F.conv2d(x64, w64, None, 2, 3) / div).float().to(dt).double()
    conv = torch.relu_(lin + bias.double().view(1, -1, 1, 1)).float().to(dt)
    return F.max_pool2d(conv.float(), 3, 2, 1).to(dt)

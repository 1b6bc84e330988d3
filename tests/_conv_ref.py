"""Host-only helpers of ``tests/test_conv_reference_sweep.py``: the float64 reference of a convolution case, the comparisons at each
kernel's gate, the fixed and the seeded random cases, and the magnitude bounds of the exact (integer) tier.  Nothing here touches a
device, so all of it is exercised on a CPU-only checkout."""

from __future__ import annotations

import itertools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F  # noqa: N812


class Case(NamedTuple):
    """One convolution: ``kernel`` in direct / half / wino22 / wino42 / grouped; ``pad_lo`` zero rows and columns in front of the map,
    ``pad_hi`` behind; ``groups`` > 1 only for the grouped kernel (``cin == cout == groups * channels per group``)."""

    kernel: str
    n: int
    cin: int
    cout: int
    h: int
    w: int
    k: int = 3
    stride: int = 1
    pad_lo: int = 1
    pad_hi: int = 1
    groups: int = 1
    dtype: str = "float32"

    @property
    def ho(self) -> int:
        return (self.h + self.pad_lo + self.pad_hi - self.k) // self.stride + 1

    @property
    def wo(self) -> int:
        return (self.w + self.pad_lo + self.pad_hi - self.k) // self.stride + 1


def epilogues(case: Case):
    """(bias, residual, ReLU) combinations the case's entry point has arguments for: the grouped kernel takes no residual."""
    return [(b, r, a) for b, r, a in itertools.product((False, True), repeat=3) if not (r and case.kernel == "grouped")]


# ------------------------------------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------------------------------------
def conv_ref64(case: Case, x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """``conv2d`` of exactly the given values on the CPU in float64 (OIHW weights; explicit zero border)."""
    xp = F.pad(x.double(), (case.pad_lo, case.pad_hi, case.pad_lo, case.pad_hi))
    out = F.conv2d(xp, weight.double(), None, stride=case.stride, padding=0, groups=case.groups)
    assert out.shape == (case.n, case.cout, case.ho, case.wo), (case, out.shape)
    return out.contiguous(memory_format=torch.channels_last)  # the kernels' outputs are channels-last: equal strides in every comparison


def epilogue64(lin: torch.Tensor, bias: torch.Tensor | None, res: torch.Tensor | None, relu: bool) -> torch.Tensor:
    """Bias, residual and ReLU in float64 on a float64 convolution."""
    if bias is None and res is None:
        return torch.relu(lin) if relu else lin
    out = lin + bias.double().view(1, -1, 1, 1) if bias is not None else lin + res
    if bias is not None and res is not None:
        out.add_(res)  # (float32 widens exactly)
    return out.relu_() if relu else out


def to_half_once(exact: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """ONE rounding of an exact float64 value to half (through float32, which holds the exact tier's integers below 2^24 exactly)."""
    return exact.float().to(dtype)


# ------------------------------------------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------------------------------------------
def make_data(case: Case, seed: int):
    """Tolerance tiers: normal inputs and residual, He-scaled weights, bias of 0.1 sigma (the data of the existing kernel tests).  For
    the half kernel the inputs, weights and residual are rounded to half here, so the reference sees the kernel's own values."""
    g = torch.Generator().manual_seed(seed)
    cg = case.cin // case.groups
    x = torch.randn((case.n, case.cin, case.h, case.w), generator=g)
    weight = torch.randn((case.cout, cg, case.k, case.k), generator=g) * (2.0 / (cg * case.k * case.k)) ** 0.5
    bias = torch.randn(case.cout, generator=g) * 0.1
    res = torch.randn((case.n, case.cout, case.ho, case.wo), generator=g)
    if case.kernel == "half":
        dt = getattr(torch, case.dtype)
        x, weight, res = x.to(dt).float(), weight.to(dt).float(), res.to(dt).float()
    return x, weight, bias, res


# value ranges of the exact tier per kernel: inputs in {-x .. x}, weights in w_step * {-1, 0, 1}, |bias| and |residual| up to the two
# last entries.  Winograd weights are multiples of 4 (F(2x2): G has halves, G g G^T quarters) / 48 (F(4x2): G4 has 1/24, G2 1/2), which
# makes the transformed weights integers; F(4x2) takes inputs in {-1, 0, 1} so that 192 input channels stay below 2^24 (exact_bound).
# The half kernel's bias and residual are LARGE on purpose: the results must lie where half no longer holds every integer (above
# 256 for bf16, above 2048 for fp16), or a second rounding inside the epilogue could not show.
EXACT_RANGES = {
    "direct": (2, 1, 64, 64),
    "grouped": (2, 1, 64, 0),
    "wino22": (2, 4, 64, 64),
    "wino42": (1, 48, 64, 64),
    "bfloat16": (2, 1, 700, 1024),
    "float16": (2, 1, 6000, 8192),
}
HALF_INTEGER_LIMIT = {"bfloat16": 256, "float16": 2048}  # integers up to here are all representable


def exact_ranges(case: Case):
    return EXACT_RANGES[case.dtype if case.kernel == "half" else case.kernel]


def make_exact_data(case: Case, seed: int):
    """Integer data of the exact tier (float32 tensors holding integers; for the half kernel every value is representable in half)."""
    x_max, w_step, b_max, r_max = exact_ranges(case)
    rng = np.random.default_rng(seed)
    cg = case.cin // case.groups
    x = torch.from_numpy(rng.integers(-x_max, x_max + 1, (case.n, case.cin, case.h, case.w)).astype(np.float32))
    weight = torch.from_numpy((w_step * rng.integers(-1, 2, (case.cout, cg, case.k, case.k))).astype(np.float32))
    if case.kernel == "half":
        # magnitudes in the upper half of the range, random signs: conv + bias alone is already beyond half's exact integers
        bias = torch.from_numpy((rng.integers(b_max // 2, b_max + 1, case.cout) * rng.choice([-1, 1], case.cout)).astype(np.float32))
        res = torch.from_numpy(rng.integers(-r_max, r_max + 1, (case.n, case.cout, case.ho, case.wo)).astype(np.float32))
        dt = getattr(torch, case.dtype)
        res = res.to(dt).float()  # the residual arrives in half: representable integers only
        assert torch.equal(x.to(dt).float(), x) and torch.equal(weight.to(dt).float(), weight)
    else:
        bias = torch.from_numpy(rng.integers(-b_max, b_max + 1, case.cout).astype(np.float32))
        res = torch.from_numpy(rng.integers(-r_max, r_max + 1, (case.n, case.cout, case.ho, case.wo)).astype(np.float32))
    return x, weight, bias, res


# The Winograd transform matrices (Lavin & Gray), for the bounds only.
_BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
_G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
_AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
_BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                 [0, 4, 0, -5, 0, 1]], dtype=np.float64)
_G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                [0, 0, 1]], dtype=np.float64)
_AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def _row_sum(m: np.ndarray) -> float:
    return float(np.abs(m).sum(axis=1).max())


def exact_bound(case: Case) -> float:
    """Largest magnitude any product, partial sum or result can reach with the exact tier's value ranges, from the absolute row sums
    of the transform matrices: while it is below 2^24 every float32 operation of the kernel is exact in any order.
    Direct / grouped / half: ``k * k * cin_per_group`` products of at most ``x_max * w_max``.  Winograd: transformed input
    ``|B^T d B| <= rows(B^T)_y * rows(B^T)_x * x_max``, transformed weight ``|G g G^T| <= rows(G)_y * rows(G)_x * w_max``, ``cin`` products
    per position, then the output transform ``rows(A^T)_y * rows(A^T)_x`` (its partial sums are bounded by the same figure)."""
    x_max, w_max, b_max, r_max = exact_ranges(case)
    if case.kernel in ("wino22", "wino42"):
        bty, gy, aty = (_BT4, _G4, _AT4) if case.kernel == "wino42" else (_BT2, _G2, _AT2)
        v = _row_sum(bty) * _row_sum(_BT2) * x_max
        u = _row_sum(gy) * _row_sum(_G2) * w_max
        conv = _row_sum(aty) * _row_sum(_AT2) * case.cin * u * v
    else:
        conv = case.k * case.k * (case.cin // case.groups) * x_max * w_max
    return conv + b_max + (0 if case.kernel == "grouped" else r_max)


def wino_weights_are_integral(case: Case, weight: torch.Tensor) -> bool:
    """``G g G^T`` of the exact tier's weights has integer entries (so the packed weights, rounded once from float64, are exact)."""
    gy = _G4 if case.kernel == "wino42" else _G2
    u = np.einsum("ia,ocab,jb->ocij", gy, weight.double().numpy(), _G2)
    return bool(np.all(np.abs(u - np.round(u)) < 1e-9))  # (1/6 and 1/24 are not binary fractions: float64 leaves ~1e-14)


# ------------------------------------------------------------------------------------------------------------------------------------
# comparisons: each raises AssertionError with the case and the worst element (image, channel, row, column)
# ------------------------------------------------------------------------------------------------------------------------------------
GATE_REL = 1e-5      # Winograd and grouped: max |delta| / max |ref|
GATE_ABS = 1e-4      # float32 direct, He-scaled weights: max |delta|
HALF_EPS = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}  # per element: eps * |ref| + 1e-4 * max |ref|


def worst_element(excess: torch.Tensor):
    """Index (image, channel, row, column) of the largest entry (a NaN counts as the largest) of a [n, c, h, w] tensor of any strides.
    (``amax`` and one comparison: many times faster than ``argmax`` on the 15 M element outputs of the ring cases.)"""
    top = excess.amax()
    hit = torch.isnan(excess) if bool(torch.isnan(top)) else excess == top
    return tuple(int(i) for i in torch.nonzero(hit)[0])


def tolerance_ratio(case: Case, got: torch.Tensor, ref: torch.Tensor):
    """(worst error relative to the case's gate, index of that element).  ``ref`` float64; ``got`` the kernel's output on the CPU."""
    assert got.shape == ref.shape, (case, tuple(got.shape), tuple(ref.shape))
    err = got.double().sub_(ref).abs_()  # (a NaN is the worst element and fails every `ratio <= 1` downstream)
    if case.kernel == "direct":
        gate = GATE_ABS
    elif case.kernel == "half":
        scale = float(ref.abs().max())
        err.div_(ref.abs().mul_(HALF_EPS[case.dtype]).add_(1e-4 * scale).clamp_min_(1e-300))
        gate = 1.0
    else:
        gate = max(GATE_REL * float(ref.abs().max()), 1e-300)
    idx = worst_element(err)
    return float(err[idx]) / gate, idx


def check_tolerance(case: Case, epilogue, got: torch.Tensor, ref: torch.Tensor) -> float:
    ratio, idx = tolerance_ratio(case, got, ref)
    assert ratio <= 1.0, (f"{case} epilogue (bias, residual, relu) {epilogue}: error {ratio:.3g} x the gate at (image, channel, row, "
                          f"column) {idx}: got {float(got[idx])!r}, reference {float(ref[idx])!r}")
    return ratio


def check_exact(case: Case, epilogue, got: torch.Tensor, ref: torch.Tensor) -> None:
    """Bit for bit: ``ref`` float64 holding the exact integers; float32 kernels must return ``ref.float()``, the half kernel one
    rounding of it."""
    exp = to_half_once(ref, got.dtype) if case.kernel == "half" else ref.float()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (case, tuple(got.shape), got.dtype)
    if torch.equal(got, exp):
        return
    wrong = got != exp
    idx = worst_element((got.double() - exp.double()).abs().nan_to_num(nan=float("inf")))
    msg = (f"{case} epilogue (bias, residual, relu) {epilogue}: {int(wrong.sum())} of {wrong.numel()} elements differ from the exact "
           f"result; worst at (image, channel, row, column) {idx}: got {float(got[idx])!r}, exact {float(ref[idx])!r}")
    raise AssertionError(msg)


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 1: fixed rectangular and edge cases
# ------------------------------------------------------------------------------------------------------------------------------------
# maps the F(4x2) route really gets that are not square (32x16, 16x32, <= 8 x 8), 16x48, 16 x 16 blocks clipped differently per axis,
# and every combination of (rows a multiple of 4 or not) x (columns a multiple of 2 or not)
_WINO_RECTS = [(32, 16), (16, 32), (16, 48), (8, 3), (3, 8), (1, 8), (8, 1), (5, 7), (1, 1), (30, 18), (18, 30), (17, 33), (36, 20),
               (13, 40), (20, 13), (6, 5), (4, 7), (7, 4)]
_WINO_CHANNELS = [(16, 64), (48, 192), (48, 64), (16, 192)]  # 1 and 3 slices of 16 channels (odd: never the persistent form)
_WINO_BATCHES = [1, 3, 4, 5, 9, 2]


def _wino_cases(kernel: str) -> list[Case]:
    cases = []
    for i, (h, w) in enumerate(_WINO_RECTS):
        cin, cout = _WINO_CHANNELS[i % 4]
        cases.append(Case(kernel, _WINO_BATCHES[i % 6], cin, cout, h, w))
    # every batch size on the four-image geometry (maps of at most 8 x 8): whole, partial and single blocks
    for i, n in enumerate((1, 3, 4, 5, 9)):
        cases.append(Case(kernel, n, (16, 48)[i % 2], 64, *((8, 3), (5, 7), (3, 8))[i % 3]))
    # borders: valid, two zeros on every side, and unequal front / behind (0 / 1 is TensorFlow's "same")
    for i, (lo, hi) in enumerate(((0, 0), (2, 2), (0, 1), (1, 0), (2, 1))):
        for j, (h, w) in enumerate(((32, 16), (8, 3), (13, 40), (17, 33), (3, 8))):
            if h + lo + hi - 2 >= 1 and w + lo + hi - 2 >= 1:
                cases.append(Case(kernel, (2, 5, 1, 3, 6)[j], (16, 48)[(i + j) % 2], 64, h, w, pad_lo=lo, pad_hi=hi))
    # many slices (the persistent form needs an even slice count and two rounds of items: these stay one block per workgroup)
    cases += [Case(kernel, 2, 512, 64, 16, 32), Case(kernel, 5, 512, 192, 8, 3), Case(kernel, 1, 512, 64, 18, 30)]
    return cases


# F(2x2) window geometry on maps that are not square; the batch sizes make wino_plan pick windows with a partial last block (checked
# through tia_conv3x3_wino_geometry by a host-only test)
WINDOW_CASES = [Case("wino22", 7, 16, 64, 14, 28), Case("wino22", 5, 32, 64, 28, 14), Case("wino22", 5, 16, 128, 21, 56),
                Case("wino22", 7, 48, 64, 56, 7), Case("wino22", 6, 16, 64, 9, 42), Case("wino22", 9, 32, 64, 37, 12),
                Case("wino22", 4, 16, 64, 44, 30, pad_lo=0, pad_hi=0), Case("wino22", 5, 16, 64, 14, 28, pad_lo=0, pad_hi=1),
                Case("wino22", 7, 16, 64, 29, 14, pad_lo=1, pad_hi=0)]

# float32 direct, two images of at most 8 x 8 per block, on maps that are not square: the geometry wants 7/8 of the 64 pixels (7 x 8
# outputs) and loses to a band under "same" and valid borders, so these are the unequal and the two-zero borders
DIRECT_TWO_IMAGE_CASES = [Case("direct", 5, 32, 64, 8, 9, pad_lo=0, pad_hi=1), Case("direct", 3, 64, 128, 6, 5, pad_lo=2, pad_hi=2),
                          Case("direct", 4, 32, 64, 9, 8, pad_lo=1, pad_hi=0), Case("direct", 1, 96, 64, 5, 6, pad_lo=2, pad_hi=2)]


def _direct_cases() -> list[Case]:
    cases = []
    # band maps: widths that factor into strips, with unrelated heights, and the transposes
    chans = [(32, 64), (64, 128), (96, 192), (32, 128)]
    for i, (h, w) in enumerate(((10, 7), (9, 14), (33, 21), (12, 28), (19, 42), (23, 56), (40, 56))):
        cin, cout = chans[i % 4]
        cases.append(Case("direct", (3, 1, 2, 5, 1, 2, 1)[i], cin, cout, h, w))
        cases.append(Case("direct", (2, 4, 1, 3, 2, 1, 1)[i], cout // 2 if cout // 2 % 32 == 0 else 32, 64, w, h))
    # 16 x 16 blocks whole and clipped, two-image blocks, on rectangles
    cases += [Case("direct", 2, 32, 64, 32, 16), Case("direct", 1, 64, 128, 16, 48), Case("direct", 2, 32, 64, 30, 18),
              Case("direct", 3, 64, 64, 8, 3), Case("direct", 5, 32, 128, 5, 7), Case("direct", 1, 32, 64, 1, 8),
              Case("direct", 2, 32, 64, 1, 1), *DIRECT_TWO_IMAGE_CASES]
    # stride 2 on odd x even maps (3x3 "same" and TensorFlow-"same"), 1x1 stride 2 on rectangles
    cases += [Case("direct", 2, 32, 64, 15, 22, stride=2), Case("direct", 3, 64, 128, 22, 15, stride=2),
              Case("direct", 2, 32, 64, 15, 22, stride=2, pad_lo=0, pad_hi=1), Case("direct", 1, 32, 64, 9, 6, stride=2),
              Case("direct", 2, 64, 128, 13, 20, k=1, stride=2, pad_lo=0, pad_hi=0),
              Case("direct", 3, 32, 64, 20, 13, k=1, stride=2, pad_lo=0, pad_hi=0),
              Case("direct", 2, 96, 192, 11, 17, k=1, stride=1, pad_lo=0, pad_hi=0)]
    # explicit borders at stride 1
    for lo, hi in ((0, 1), (1, 0), (2, 2), (0, 0)):
        cases += [Case("direct", 2, 32, 64, 18, 30, pad_lo=lo, pad_hi=hi), Case("direct", 3, 64, 64, 28, 14, pad_lo=lo, pad_hi=hi)]
    # the ring (>= 384 blocks of 256 pixels x 128 channels): 1x1 at stride 1 and 2, and gathering 3x3 taps at stride 2
    # (the gathering ring is taken while its round of two workgroups per CU is at least 85 % full: 436 .. 512 blocks x column tiles)
    cases += [Case("direct", 8, 32, 512, 48, 66, k=1, pad_lo=0, pad_hi=0), Case("direct", 9, 32, 512, 97, 130, k=1, stride=2, pad_lo=0, pad_hi=0),
              Case("direct", 9, 32, 512, 99, 128, stride=2)]
    return cases


def _half_cases() -> list[Case]:
    cases = []
    for dtype in ("float16", "bfloat16"):
        for i, (h, w) in enumerate(((33, 55), (55, 33), (28, 42), (42, 28), (15, 64), (64, 15), (8, 5), (30, 18))):
            cin, cout = ((32, 64), (64, 128), (32, 128), (96, 64))[i % 4]
            cases.append(Case("half", (2, 1, 3, 2, 1, 2, 5, 1)[i], cin, cout, h, w, dtype=dtype))
        cases += [Case("half", 2, 32, 64, 33, 55, stride=2, dtype=dtype), Case("half", 3, 64, 128, 15, 13, stride=2, dtype=dtype),
                  Case("half", 2, 32, 64, 13, 20, k=1, stride=2, pad_lo=0, pad_hi=0, dtype=dtype)]
    return cases


GROUPED_P = {4: 4, 8: 4, 16: 4, 32: 2, 64: 2}  # output pixels per lane of the grouped kernel, per group width: blocks of 64 * P pixels


def _grouped_cases() -> list[Case]:
    """Every (groups, channels per group), each on three of the maps: 1x1, 1xW, Hx1, 2x2 at stride 2, and output pixel counts one
    below, at and one above the block of 64 * P pixels."""
    cases = []
    combos = [(g, cg) for cg in (4, 8, 16, 32, 64) for g in (1, 3, 5, 32, 33, 64)]
    for i, (groups, cg) in enumerate(combos):
        c = groups * cg
        block = 64 * GROUPED_P[cg]
        # (n, h, w, stride) with n * ho * wo == block - 1, block, block + 1 (255 = 3 * 5 * 17, 257 prime; 127 prime, 129 = 3 * 43)
        edge = ([(3, 5, 17, 1), (1, 8, 32, 1), (1, 1, 257, 1), (1, 16, 63, 2)] if block == 256 else  # noqa: PLR2004
                [(1, 127, 1, 1), (1, 8, 16, 1), (3, 1, 43, 1), (1, 15, 32, 2)])
        small = [(1, 1, 1, 1), (3, 1, 9, 1), (7, 9, 1, 1), (3, 2, 2, 2), (7, 1, 1, 2), (1, 3, 2, 2), (7, 5, 3, 1)]
        picks = [edge[i % 4], edge[(i + 1) % 4], small[i % 7], small[(i + 3) % 7]]
        for n, h, w, stride in picks:
            cases.append(Case("grouped", n, c, c, h, w, stride=stride, groups=groups))
    return cases


def fixed_cases(kernel: str) -> list[Case]:
    if kernel == "wino42":
        return _wino_cases("wino42")
    if kernel == "wino22":
        return _wino_cases("wino22") + WINDOW_CASES
    return {"direct": _direct_cases, "half": _half_cases, "grouped": _grouped_cases}[kernel]()


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 2: seeded random cases (only what each entry point documents as served)
# ------------------------------------------------------------------------------------------------------------------------------------
RANDOM_SEED = 20261016
RANDOM_COUNT = {"direct": 40, "half": 32, "wino22": 40, "wino42": 32, "grouped": 36}
_BAND_WIDTHS = (7, 14, 21, 28, 30, 33, 42, 45, 56, 60)


def _draw_hw(rng, kind: int, shrink: int):
    """Height and width drawn independently; ``kind`` biases the draw towards one block geometry (``shrink`` = 2 - pad_lo - pad_hi,
    so that the OUTPUT map has the drawn size)."""
    if kind == 0:    # anything
        h, w = int(rng.integers(1, 72)), int(rng.integers(1, 72))
    elif kind == 1:  # maps of at most 8 x 8: several images per block
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    elif kind == 2:  # whole 16 x 16 blocks
        h, w = 16 * int(rng.integers(1, 5)), 16 * int(rng.integers(1, 5))
    elif kind == 3:  # widths that factor into strips (bands, windows)
        h, w = int(rng.integers(4, 64)), int(rng.choice(_BAND_WIDTHS))
    else:            # the same, transposed
        h, w = int(rng.choice(_BAND_WIDTHS)), int(rng.integers(4, 64))
    return max(h + shrink, 1), max(w + shrink, 1)


def random_cases(kernel: str) -> list[Case]:
    rng = np.random.default_rng([RANDOM_SEED, sorted(RANDOM_COUNT).index(kernel)])
    cases = []
    for i in range(RANDOM_COUNT[kernel]):
        n = int(rng.integers(1, 10))
        if kernel in ("wino22", "wino42"):
            lo, hi = ((1, 1), (1, 1), (0, 0), (2, 2), (0, 1), (1, 0), (2, 1))[int(rng.integers(0, 7))]
            kinds = (0, 1, 2, 3, 4) if kernel == "wino22" else (0, 1, 2, 1, 0)
            h, w = _draw_hw(rng, kinds[i % 5], 2 - lo - hi)
            cases.append(Case(kernel, n, 16 * int(rng.integers(1, 9)), 64 * int(rng.integers(1, 4)), h, w, pad_lo=lo, pad_hi=hi))
        elif kernel == "grouped":
            cg = int(rng.choice([4, 8, 16, 32, 64]))
            groups = int(rng.integers(1, 512 // cg + 1)) if i % 3 else int(rng.choice([1, 2, 3, 5, 7, 33]))
            cases.append(Case(kernel, n, groups * cg, groups * cg, int(rng.integers(1, 40)), int(rng.integers(1, 40)),
                              stride=int(rng.integers(1, 3)), groups=groups))
        else:
            cin, cout = 32 * int(rng.integers(1, 5)), 64 * int(rng.integers(1, 4))
            dtype = ("float16", "bfloat16")[i % 2] if kernel == "half" else "float32"
            form = i % 8
            if form == 5:                         # 1x1, stride 1 or 2
                stride = int(rng.integers(1, 3))
                cases.append(Case(kernel, n, cin, cout, int(rng.integers(1, 48)), int(rng.integers(1, 48)), k=1, stride=stride,
                                  pad_lo=0, pad_hi=0, dtype=dtype))
            elif form == 6:                       # 3x3 at stride 2, "same" or (float32) TensorFlow-"same"
                lo = 1 if kernel == "half" else int(rng.integers(0, 2))
                cases.append(Case(kernel, n, cin, cout, int(rng.integers(2, 60)), int(rng.integers(2, 60)), stride=2, pad_lo=lo,
                                  pad_hi=1, dtype=dtype))
            elif form == 7 and kernel == "direct":  # large enough for the ring: >= 384 blocks of 256 pixels x 128 channels
                stride = int(rng.integers(1, 3))
                if i == 7:                        # gathering 3x3 taps at stride 2: one round of workgroups, >= 85 % full
                    nb, k, stride, ho, wo = 9, 3, 2, int(rng.integers(49, 52)), int(rng.integers(64, 70))
                else:                             # 1x1
                    nb, k, ho, wo = int(rng.integers(8, 10)), 1, int(rng.integers(44, 50)), int(rng.integers(70, 76))
                cases.append(Case(kernel, nb, 32, 512, ho * stride - int(rng.integers(0, stride)), wo * stride - int(rng.integers(0, stride)),
                                  k=k, stride=stride, pad_lo=k // 2, pad_hi=k // 2))
            elif form == 1 and kernel == "direct":  # two images of at most 8 x 8 per block: 7 x 8 outputs under an unequal border
                lo, hi = ((0, 1), (1, 0), (2, 2), (2, 1))[int(rng.integers(0, 4))]
                ho, wo = ((7, 8), (8, 7))[int(rng.integers(0, 2))]
                cases.append(Case(kernel, n, cin, cout, ho + 2 - lo - hi, wo + 2 - lo - hi, pad_lo=lo, pad_hi=hi))
            else:                                 # 3x3 at stride 1
                if kernel == "half":
                    lo = hi = int(rng.integers(0, 2))
                else:
                    lo, hi = ((1, 1), (1, 1), (0, 0), (2, 2), (0, 1), (1, 0))[int(rng.integers(0, 6))]
                h, w = _draw_hw(rng, form % 5, 2 - lo - hi)
                cases.append(Case(kernel, n, cin, cout, h, w, pad_lo=lo, pad_hi=hi, dtype=dtype))
    return cases


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 3: the exact tier's cases -- a subset of tier 1 that reaches every form, rectangular maps first
# ------------------------------------------------------------------------------------------------------------------------------------
def exact_cases(kernel: str) -> list[Case]:
    cases = fixed_cases(kernel)
    if kernel in ("wino22", "wino42"):
        keep = [c for c in cases if c.cin <= 48][::2] + [c for c in cases if c in WINDOW_CASES][1::2]  # noqa: PLR2004
        # more channels, still below 2^24 for F(4x2): 12 slices (an even count)
        return keep + [Case(kernel, 2, 192, 64, 16, 32), Case(kernel, 5, 192, 64, 8, 3), Case(kernel, 9, 64, 128, 5, 7)]
    if kernel == "grouped":
        return cases[::3]
    if kernel == "half":
        # plus many channels: the convolution itself beyond half's exact integers now and then
        return cases[::2] + [Case("half", 2, 512, 64, 28, 42, dtype=d) for d in ("float16", "bfloat16")]
    small = [c for c in cases if c.n * c.ho * c.wo < 20000]  # noqa: PLR2004  (the ring cases are added by name: 15 M outputs each)
    ring = [c for c in cases if c not in small and c.stride == 2]  # noqa: PLR2004  (1x1 at stride 2, gathered 3x3 taps)
    return small[::2] + [c for c in small if c.k == 1 or c.stride == 2 or c in DIRECT_TWO_IMAGE_CASES][1::2] + ring  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------------------------------------------
# route coverage through the library's host-only queries
# ------------------------------------------------------------------------------------------------------------------------------------
def form_of(lib, case: Case) -> str:
    """Which form of its kernel a case runs on, from the host-only queries (no launch): direct ``geometry 0 / 1 / 2 / 4`` or ``ring``;
    F(2x2) ``blocks16 / four-image / windows``; F(4x2) ``blocks16 / four-image``."""
    import ctypes

    if case.kernel == "direct":
        route = lib.tia_conv2d_route_f32(case.n, case.h, case.w, case.cin, case.cout, case.k, case.k, case.stride, case.pad_lo,
                                         case.pad_lo, case.ho, case.wo)
        assert route >= 0, (case, route)
        if route == 2:  # noqa: PLR2004
            return "ring"
        geom = (ctypes.c_int32 * 4)()
        kind = lib.tia_conv3x3_geometry(case.h, case.w, case.ho, case.wo, case.pad_lo, case.pad_lo, geom) if route == 1 else 0
        return f"geometry {kind}"
    if case.kernel == "wino22":
        kind = lib.tia_conv3x3_wino_geometry(case.n, case.ho, case.wo, None)
        assert kind >= 0, (case, kind)
        return ("blocks16", "four-image", "windows")[kind]
    if case.kernel == "wino42":
        return "four-image" if case.ho <= 8 and case.wo <= 8 else "blocks16"  # noqa: PLR2004  (its only two geometries: by output size)
    return case.kernel


REQUIRED_FORMS = {
    "direct": ("geometry 0", "geometry 1", "geometry 2", "geometry 4", "ring"),
    "wino22": ("blocks16", "four-image", "windows"),
    "wino42": ("blocks16", "four-image"),
}
FORM_FLOOR = 4  # non-square cases per form in the random sweep


def non_square_form_counts(lib, cases) -> dict[str, int]:
    counts: dict[str, int] = {}
    for c in cases:
        if c.h != c.w:
            f = form_of(lib, c)
            counts[f] = counts.get(f, 0) + 1
    return counts

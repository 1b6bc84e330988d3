"""Helpers of ``tests/test_imgops_reference.py``: NumPy / SciPy references of the image primitives of ``csrc/imgops.hip``, the fixed and
the seeded random cases, the comparisons, and which form or path of its kernel a case takes (restated from the source, so that the
host tests can prove the reach of the lists without a device).  Everything above the last section is host only and is exercised on
a CPU-only checkout; the last section holds the three device runners that the test module and the fall-back child share.

``python tests/_imgops_ref.py --child OUT.npz`` is that child: it runs the small labelling, hole-filling and area-filter cases in a
fresh process (started with ``TIA_DEV=1 TIA_NO_CCL_TILE=1``, read once per process by the library) and stores what the kernels
returned; the parent compares it with the same references."""

from __future__ import annotations

import os
import sys
from pathlib import Path
from typing import NamedTuple

import numpy as np
from scipy import ndimage

# ------------------------------------------------------------------------------------------------------------------------------------
# shapes and thresholds of imgops.hip (each with the line it mirrors)
# ------------------------------------------------------------------------------------------------------------------------------------
CCL_TILE_MAX_PIXELS = 36864       # common.hpp:243 kCclTileMaxPixels; imgops.hip:1385 (tia_ccl_label_i32), 1422 (tia_fill_holes_u8)
BLOCK = 256                       # imgops.hip:11 BT
GRID_CAP = 4096                   # workgroups: imgops.hip:464 (ccl_run), 1397 (tia_label_area_filter_i32), 1409 (tia_binary_morph_u8),
                                  # 1431 (tia_fill_holes_u8)
ROUND_LANES = GRID_CAP * BLOCK    # 1,048,576 lanes per grid round; morph_kernel's fast path counts 4-pixel quads (imgops.hip:1087)
HIST_GRID_CAP = 2048              # imgops.hip:1283 (tia_hist256_u8): workgroups of hist256_kernel, 4 bytes per lane and round
HIST_ROUND_BYTES = HIST_GRID_CAP * BLOCK * 4
LUT_GRID_CAP = 2048               # imgops.hip:1439 (tia_lut_apply_u8): workgroups of lut_apply_kernel per image, 16 bytes per lane and round
LUT_ROUND_BYTES = LUT_GRID_CAP * BLOCK * 16
RANK_TILE = 8192                  # imgops.hip:411: pixels per sweep of ccl_rank_kernel
LDS_RANK_TILE = 4096              # imgops.hip:573: pixels per sweep of tile_rank_filter, the LDS form's ranking
AREA_BLOCK_PIXELS = 16384         # imgops.hip:1399 (tia_label_area_filter_i32): pixels per workgroup that sizes area_count_kernel's grid ...
AREA_BLOCKS, AREA_BLOCKS_MANY, AREA_MANY_PLANES = 64, 8, 64  # ... capped at 64 workgroups per plane, 8 when n >= 64
MORPH_MAX_DX, MORPH_MAX_ROWS = 4, 16  # imgops.hip:1064, 1068 (morph_kernel): the bit-window path's element limits
SEED = 20261017


# ------------------------------------------------------------------------------------------------------------------------------------
# references (NumPy / SciPy only)
# ------------------------------------------------------------------------------------------------------------------------------------
def label_ref(mask: np.ndarray, conn: int):
    """``scipy.ndimage.label`` of one plane: (int32 labels numbered in raster order of each component's first pixel, count)."""
    lab, count = ndimage.label(mask != 0, structure=np.ones((3, 3), int) if conn == 8 else None)  # noqa: PLR2004
    return lab.astype(np.int32), int(count)


def fill_ref(mask: np.ndarray) -> np.ndarray:
    """``scipy.ndimage.binary_fill_holes`` (4-connected background) as 0/1 bytes."""
    return ndimage.binary_fill_holes(mask != 0).astype(np.uint8)


def area_filter_ref(labels: np.ndarray, min_keep: int) -> np.ndarray:
    """Labels whose pixel count is below ``min_keep`` zeroed, the others unchanged (one plane)."""
    areas = np.bincount(labels.ravel(), minlength=labels.size + 1)
    return np.where((labels > 0) & (areas[labels] >= min_keep), labels, 0).astype(np.int32)


def morph_ref(src: np.ndarray, offsets, op: str, *, erode_outside: int = 1) -> np.ndarray:
    """``out[y, x] = any (dilate) / all (erode) of src[y + dy, x + dx]`` over the element's offsets, written out as shifts; outside the
    plane a dilation sees 0 and an erosion 1.  ``src`` [h, w], non-zero = set; 0/1 bytes."""
    s = src != 0
    h, w = s.shape
    outside = (op == "erode") and bool(erode_outside)
    out = np.zeros((h, w), bool) if op == "dilate" else np.ones((h, w), bool)
    for dy, dx in offsets:
        shifted = np.full((h, w), outside)
        y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)  # output pixels whose source pixel is inside
        if y0 < y1 and x0 < x1:
            shifted[y0:y1, x0:x1] = s[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        out = (out | shifted) if op == "dilate" else (out & shifted)
    return out.astype(np.uint8)


def gray_ref(rgb: np.ndarray) -> np.ndarray:
    """The header's integer formula: ``(R * 9798 + G * 19235 + B * 3735 + 2^14) >> 15`` of [npix, 3] bytes."""
    p = rgb.reshape(-1, 3).astype(np.int64)
    return ((p[:, 0] * 9798 + p[:, 1] * 19235 + p[:, 2] * 3735 + (1 << 14)) >> 15).astype(np.uint8)


def hist_ref(data: np.ndarray, *, shift_bin: int | None = None) -> np.ndarray:
    counts = np.bincount(data.ravel(), minlength=256).astype(np.int64)
    if shift_bin is not None:  # (the fault of the sensitivity test: one bin's count lands in the next bin)
        counts[shift_bin + 1] += counts[shift_bin]
        counts[shift_bin] = 0
    return counts


def lut_ref(img: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """``out[i, j] = lut[i, img[i, j]]``: img [n, len], lut [n, 256]."""
    return np.stack([lut[i][img[i]] for i in range(img.shape[0])])


def box_ref(img: np.ndarray, factor: int, *, half_up: bool = False) -> np.ndarray:
    """The exact rational mean of every ``factor x factor`` box of an [h, w, c] byte image rounded half to even, in integer
    arithmetic; rows and columns beyond ``h // factor * factor`` and ``w // factor * factor`` are dropped."""
    h, w, c = img.shape
    th, tw, area = h // factor, w // factor, factor * factor
    boxes = img[:th * factor, :tw * factor].astype(np.int64).reshape(th, factor, tw, factor, c)
    q, r = np.divmod(boxes.sum(axis=(1, 3)), area)
    up = (2 * r > area) | ((2 * r == area) & (True if half_up else (q & 1) == 1))
    return (q + up).astype(np.uint8)


def box_float32_rule(factor: int) -> np.ndarray:
    """What the kernel computes, for EVERY possible box sum of the factor: ``rint(float32(sum) * float32(1 / area))``."""
    area = factor * factor
    sums = np.arange(255 * area + 1, dtype=np.int64)
    scale = np.float32(1.0) / np.float32(area)
    return np.rint(sums.astype(np.float32) * scale).astype(np.int64)


def box_exact_rule(factor: int) -> np.ndarray:
    area = factor * factor
    q, r = np.divmod(np.arange(255 * area + 1, dtype=np.int64), area)
    return q + ((2 * r > area) | ((2 * r == area) & (q & 1 == 1)))


# ------------------------------------------------------------------------------------------------------------------------------------
# comparison: equality, with the plane, the first differing element and its neighbourhood in the message
# ------------------------------------------------------------------------------------------------------------------------------------
def check_equal(label: str, got: np.ndarray, exp: np.ndarray, src: np.ndarray | None = None) -> None:
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, f"{label}: shape {got.shape}, reference {exp.shape}"
    assert got.dtype.kind in "iub" and exp.dtype.kind in "iub", (label, got.dtype, exp.dtype)
    if np.array_equal(got, exp):
        return
    wrong = got != exp
    idx = np.unravel_index(int(np.flatnonzero(wrong.ravel())[0]), got.shape)
    lead, tail = idx[:-2], idx[-2:]  # the window spans the last two axes (rows and columns of a plane; +-4 elements of a vector)
    reach = 2 if got.ndim >= 2 else 4  # noqa: PLR2004
    win = lead + tuple(slice(max(0, i - reach), i + reach + 1) for i in tail)
    where = (f"plane {idx[0]}, row {idx[1]}, column {idx[2]}" if got.ndim == 3 else  # noqa: PLR2004
             "index " + ", ".join(str(int(i)) for i in idx))
    msg = (f"{label}: {int(wrong.sum())} of {wrong.size} elements differ; first differing element at {where}: got {int(got[idx])}, "
           f"reference {int(exp[idx])}\ngot around it:\n{got[win].astype(np.int64)}\nreference around it:\n{exp[win].astype(np.int64)}")
    if src is not None and src.shape == got.shape:
        msg += f"\nsource around it:\n{src[win].astype(np.int64)}"
    raise AssertionError(msg)


# ------------------------------------------------------------------------------------------------------------------------------------
# patterns
# ------------------------------------------------------------------------------------------------------------------------------------
def _corners(h: int, w: int):
    return ((0, 0, 1, 1), (0, w - 1, 1, -1), (h - 1, 0, -1, 1), (h - 1, w - 1, -1, -1))  # (row, column, step inwards y, x)


def make_plane(name: str, h: int, w: int) -> np.ndarray | None:  # noqa: C901, PLR0911, PLR0912
    """Boolean [h, w] plane of the named pattern, or None when the shape cannot hold it.  ``random<p>`` takes an optional ``#k``."""
    yy, xx = np.indices((h, w))
    m = np.zeros((h, w), bool)
    base, _, variant = name.partition("#")
    if base == "empty":
        return m
    if base == "full":
        return ~m
    if base == "checker":            # hw / 2 components under 4, one under 8: the largest rank and the densest root set
        return (yy + xx) % 2 == 0
    if base == "serpentine":         # full rows joined alternately at the ends: one component, the deepest union chains
        m[::2, :] = True
        m[1::4, -1] = True
        m[3::4, 0] = True
        return m
    if base == "comb":               # teeth that first meet in the last row: every tooth's root is re-hooked at the very end
        m[:, ::2] = True
        m[-1, :] = True
        return m
    if base == "diag_down":          # stripes along (1, 1): joined under 8 through the upper-left neighbour, separate under 4
        return (yy - xx) % 3 == 0
    if base == "diag_up":            # stripes along (1, -1): joined through the upper-right neighbour
        return (yy + xx) % 3 == 0
    if base == "rings":              # nested rings: holes inside islands inside holes
        return (np.minimum(np.minimum(yy, xx), np.minimum(h - 1 - yy, w - 1 - xx)) % 4 == 1) if min(h, w) >= 3 else None  # noqa: PLR2004
    if base == "corner_ring":        # the ring's "hole" is the frame's corner pixel: it touches the frame, so it stays open
        if min(h, w) < 5:  # noqa: PLR2004
            return None
        for cy, cx, sy, sx in _corners(h, w):
            m[cy, cx + sx] = m[cy + sy, cx] = m[cy + sy, cx + sx] = True
        return m
    if base == "diag_hole":          # a hole one step inside each corner: it touches the frame only diagonally, so it is filled
        if min(h, w) < 7:  # noqa: PLR2004
            return None
        for cy, cx, sy, sx in _corners(h, w):
            m[cy, cx + sx] = m[cy + sy, cx] = m[cy + sy, cx + 2 * sx] = m[cy + 2 * sy, cx + sx] = True
        return m
    if base.startswith("random"):
        p = float(base[len("random"):])
        rng = np.random.default_rng([SEED, int(p * 1000), h, w, int(variant or 0)])
        return rng.random((h, w)) < p
    raise ValueError(name)


def holds(name: str, h: int, w: int) -> bool:
    """Whether ``make_plane`` returns a plane (from the shape alone)."""
    return min(h, w) >= {"rings": 3, "corner_ring": 5, "diag_hole": 7}.get(name.partition("#")[0], 1)


PATTERNS = ("empty", "full", "checker", "serpentine", "comb", "diag_down", "diag_up", "rings", "corner_ring", "diag_hole",
            "random0.3", "random0.5", "random0.62", "random0.9")
FG_BYTES = (1, 255, 128, 2)  # tia_ccl_label_i32: "non-zero = foreground"


def mask_bytes(names, h: int, w: int, *, binary: bool = False) -> np.ndarray:
    """[n, h, w] bytes of the named patterns; foreground 1, or (labelling) another non-zero value per plane, mixed in random planes."""
    planes = []
    for k, name in enumerate(names):
        m = make_plane(name, h, w)
        assert m is not None, (name, h, w)
        if binary:
            planes.append(m.astype(np.uint8))
        elif name.startswith("random"):
            values = np.random.default_rng([SEED, 7, h, w, k]).choice(np.array(FG_BYTES, np.uint8), (h, w))
            planes.append(np.where(m, values, 0).astype(np.uint8))
        else:
            planes.append(np.where(m, FG_BYTES[k % 4], 0).astype(np.uint8))
    return np.stack(planes)


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 1: labelling and hole filling
# ------------------------------------------------------------------------------------------------------------------------------------
class LabelCase(NamedTuple):
    """One call: ``len(patterns)`` planes of h x w (hole filling takes the cases of connectivity 4 and ignores it)."""

    h: int
    w: int
    conn: int
    patterns: tuple

    @property
    def n(self) -> int:
        return len(self.patterns)


LDS_SHAPES = [(1, 1), (1, 200), (200, 1), (130, 63), (131, 64), (129, 65), (192, 192), (191, 193)]
MULTI_SHAPES = [(193, 192), (1, 40000), (40000, 1), (190, 211), (1024, 1024), (1100, 1000)]
MANY_PLANES_SHAPE, MANY_PLANES = (23, 37), 70


def label_form(h: int, w: int) -> str:
    """imgops.hip:1385 / 1422 in the tested configuration (the LDS attribute granted)."""
    return "lds" if h * w <= CCL_TILE_MAX_PIXELS else "multi-launch"


def grid_rounds(h: int, w: int) -> int:
    """Rounds of the 4096 x 256-lane grid-stride loops (imgops.hip:352, 374, 394, 455)."""
    return -(-h * w // ROUND_LANES)


def shape_label_cases(h: int, w: int) -> list[LabelCase]:
    """Every pattern the shape can hold, in calls of alternately three planes and one, for both connectivities."""
    names = [p for p in PATTERNS if holds(p, h, w)]
    groups, i = [], 0
    while i < len(names):
        size = 3 if len(groups) % 2 == 0 and len(names) - i >= 3 else 1  # noqa: PLR2004
        groups.append(tuple(names[i:i + size]))
        i += size
    return [LabelCase(h, w, conn, g) for conn in (4, 8) for g in groups]


def many_planes_cases() -> list[LabelCase]:
    h, w = MANY_PLANES_SHAPE
    names = tuple(PATTERNS[k % len(PATTERNS)] if k < len(PATTERNS) else f"random0.{3 + k % 5}#{k}" for k in range(MANY_PLANES))
    return [LabelCase(h, w, conn, names) for conn in (4, 8)]


def label_cases() -> list[LabelCase]:
    return [c for h, w in LDS_SHAPES + MULTI_SHAPES for c in shape_label_cases(h, w)] + many_planes_cases()


def small_label_cases() -> list[LabelCase]:
    """Tier 3: the cases below the LDS limit (the multi-launch forms reach them only when the LDS form is switched off)."""
    return [c for c in label_cases() if label_form(c.h, c.w) == "lds"]


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 1: area filter
# ------------------------------------------------------------------------------------------------------------------------------------
class AreaCase(NamedTuple):
    """Label planes ``pattern/connectivity`` (SciPy's labels of the pattern) or ``direct#k`` (ids handed in, not consecutive)."""

    h: int
    w: int
    planes: tuple

    @property
    def n(self) -> int:
        return len(self.planes)

    @property
    def min_keeps(self) -> tuple:
        hw = self.h * self.w
        return (0, 1, 10, hw, hw + 1)


def direct_labels(h: int, w: int, k: int) -> np.ndarray:
    """Runs of 1 .. 40 pixels with ids drawn from 48 values spread over 1 .. hw (hw itself among them: the last entry of the area
    table), the 40 smallest repeated in runs that do not touch, the others rare, and zeros."""
    hw = h * w
    rng = np.random.default_rng([SEED, 11, h, w, k])
    ids = np.unique(np.concatenate([[1, hw, hw - 1, hw // 2], rng.integers(1, hw + 1, 44)]))
    flat = np.zeros(hw, np.int32)
    pos = 0
    while pos < hw:
        ln = int(rng.integers(1, 41))
        flat[pos:pos + ln] = 0 if rng.random() < 0.25 else int(rng.choice(ids[:40]))  # noqa: PLR2004
        pos += ln
    for rare in ids[40:-1]:  # the largest ids occur once, in a run of fewer than 10 pixels
        pos = int(rng.integers(0, hw - 10))
        flat[pos:pos + int(rng.integers(1, 10))] = rare
    flat[-1] = hw
    return flat.reshape(h, w)


def area_labels(case: AreaCase) -> np.ndarray:
    planes = []
    for spec in case.planes:
        if spec.startswith("direct"):
            planes.append(direct_labels(case.h, case.w, int(spec.partition("#")[2])))
        else:
            name, _, conn = spec.partition("/")
            planes.append(label_ref(make_plane(name, case.h, case.w), int(conn))[0])
    return np.stack(planes)


def area_path(h: int, w: int) -> str:
    return "int4" if h * w % 4 == 0 else "scalar"  # imgops.hip:997


def area_count_blocks(n: int, h: int, w: int) -> int:
    """Workgroups per plane of area_count_kernel (imgops.hip:1399); each sweeps 1024 pixels per iteration."""
    return max(1, min(-(-h * w // AREA_BLOCK_PIXELS), AREA_BLOCKS_MANY if n >= AREA_MANY_PLANES else AREA_BLOCKS))


def area_cases() -> list[AreaCase]:
    many = tuple(f"random0.5#{k}/{4 + 4 * (k % 2)}" for k in range(AREA_MANY_PLANES))
    big = ("full/4", "serpentine/4", "random0.62#{k}/8", "checker/4", "comb/4", "random0.3#{k}/4", "rings/8", "checker/8")
    many_big = tuple(big[k % len(big)].format(k=k) for k in range(AREA_MANY_PLANES))
    return [AreaCase(97, 131, ("random0.3/4", "random0.5/8", "checker/4")),                 # hw odd: scalar loads
            AreaCase(64, 64, ("random0.62/4", "checker/4", "full/4", "direct#0")),          # hw % 4 == 0: int4 loads
            AreaCase(190, 211, ("random0.5/4", "direct#1")),                                # hw % 4 == 2
            AreaCase(193, 192, ("random0.9/8", "comb/4", "direct#2")),
            AreaCase(1100, 1000, ("full/4", "checker/8", "random0.62/8")),                  # one component of > 10^6 pixels: run cache
            AreaCase(1024, 1024, ("checker/4",)),                                           # every lane non-uniform, ids up to hw / 2
            AreaCase(1001, 1049, ("full/4", "serpentine/4")),                               # the same through the scalar loads
            AreaCase(23, 37, many), AreaCase(24, 36, many),                                 # n >= 64, one workgroup per plane
            AreaCase(384, 512, many_big), AreaCase(383, 513, many_big)]                     # n >= 64: the cap of 8 workgroups binds


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 1: morphology
# ------------------------------------------------------------------------------------------------------------------------------------
class MorphCase(NamedTuple):
    name: str
    h: int
    w: int
    offsets: tuple      # (dy, dx) pairs
    src_off: int = 0    # bytes between the allocation base and the source view
    n: int = 2


def ellipse_offsets(ksize) -> tuple:
    """``offsets_of(get_structuring_element_ellipse(ksize))``: the library's own host-side element and anchor."""
    from tiatoolbox_amd.tools._img_device import get_structuring_element_ellipse

    elem = get_structuring_element_ellipse(ksize)
    kh, kw = elem.shape
    ys, xs = np.nonzero(elem)
    return tuple((int(y) - kh // 2, int(x) - kw // 2) for y, x in zip(ys, xs))


def morph_triggers(case: MorphCase) -> set:
    """What sends a case to the generic loop (imgops.hip:1410, 1064, 1068); empty: the bit-window path."""
    t = set()
    if case.w % 4:
        t.add("w % 4")
    if case.src_off % 4:
        t.add("unaligned source")
    if any(abs(dx) > MORPH_MAX_DX for _, dx in case.offsets):
        t.add("|dx| > 4")
    if len({dy for dy, _ in case.offsets}) > MORPH_MAX_ROWS:
        t.add("more than 16 rows")
    return t


def morph_path(case: MorphCase) -> str:
    return "generic" if morph_triggers(case) else "fast"


ONE_OFFSETS = ((0, 4), (0, -4), (3, -4), (-8, 0))
SIXTEEN_ROWS = tuple((dy, (dy * 4) % 9 - 4) for dy in range(-8, 8))   # exactly 16 rows, every dx in -4 .. 4
SEVENTEEN_ROWS = tuple((dy, (dy * 4) % 9 - 4) for dy in range(-8, 9))
ASYMMETRIC = ((-2, -1), (-2, 3), (0, 0), (1, -4), (1, 2), (3, 4), (5, -3))
MORPH_BIG = (2052, 2048)  # 1,050,624 quads: a second round of the fast path's grid


def morph_cases() -> list[MorphCase]:
    cases = [MorphCase(f"one offset {o}", 41, 68, (o,)) for o in ONE_OFFSETS]
    cases += [MorphCase(f"ellipse {k}", 41, 68, ellipse_offsets(k)) for k in ((20, 1), (1, 20), (5, 5), (16, 16))]
    cases += [MorphCase("16 rows", 41, 68, SIXTEEN_ROWS), MorphCase("duplicated offsets", 41, 68, ASYMMETRIC + ASYMMETRIC[2:5] + ((0, 0),)),
              MorphCase("w = 4", 19, 4, ASYMMETRIC), MorphCase("h = 1", 1, 64, ASYMMETRIC), MorphCase("1 x 4", 1, 4, ((0, 1), (0, -3))),
              MorphCase("three planes", 33, 128, ASYMMETRIC, n=3)]
    # the generic loop by each of its four triggers alone
    cases += [MorphCase("w % 4 != 0", 41, 67, ASYMMETRIC), MorphCase("|dx| = 5", 41, 68, ((0, 5), (2, -1))),
              MorphCase("dx = -5", 41, 68, ((-1, -5), (0, 0))), MorphCase("17 rows", 41, 68, SEVENTEEN_ROWS),
              MorphCase("source one byte off a dword", 41, 68, ASYMMETRIC, src_off=1), MorphCase("w = 1", 50, 1, ((-1, 0), (2, 0), (0, 1)))]
    cases.append(MorphCase("second grid round", *MORPH_BIG, ellipse_offsets((5, 5)), n=1))
    return cases


def morph_planes(case: MorphCase) -> np.ndarray:
    """[n, h, w] bytes that reach every border: a sparse plane with its corners set (dilation), a dense plane with its corners
    clear (erosion), then half-dense planes; the odd planes use other non-zero bytes than 1 (the kernels test ``!= 0``)."""
    rng = np.random.default_rng([SEED, 13, case.h, case.w, len(case.offsets)])
    planes = []
    for k in range(case.n):
        m = rng.random((case.h, case.w)) < (0.08, 0.92, 0.5)[min(k, 2)]
        for cy, cx, _, _ in _corners(case.h, case.w):
            m[cy, cx] = k != 1
        values = rng.choice(np.array(FG_BYTES, np.uint8), (case.h, case.w)) if k % 2 else np.uint8(1)
        planes.append(np.where(m, values, 0).astype(np.uint8))
    return np.stack(planes)


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 1: bytes (grey, histogram, threshold, LUT) and box down-sampling
# ------------------------------------------------------------------------------------------------------------------------------------
BYTE_LENGTHS = (1, 3, 15, 16, 17, 1000, 1001, 1002, 1003, 4099)
BYTE_OFFSETS = (0, 1, 2, 3)
LUT_OFFSETS = tuple(range(16))
THRESHOLDS = (0, 1, 128, 255, 256)
HIST_BIG = 2 * HIST_ROUND_BYTES + 1003   # a third, partial round of hist256_kernel's grid
LUT_BIG = 2 * LUT_ROUND_BYTES + 1003     # the same for lut_apply_kernel
BYTE_KINDS = ("random", "ramp", "constant")


def byte_data(length: int, kind: str, seed: int = 0) -> np.ndarray:
    if kind == "ramp":       # every byte value once the length allows it
        return (np.arange(length) * 7 % 256).astype(np.uint8)
    if kind == "constant":   # all lanes on one counter
        return np.full(length, 200, np.uint8)
    return np.random.default_rng([SEED, 17, length, seed]).integers(0, 256, length, dtype=np.uint8)


class BoxCase(NamedTuple):
    h: int
    w: int
    c: int
    factor: int


BOX_FACTORS = (1, 2, 3, 7, 16, 49)
BOX_CHANNELS = (1, 3, 4)
HALF_PARTS = (0, 1, 2, 127, 128, 253, 254)  # integer parts of the exact .5 means built into the even factors' images
BOX_FILLS = (0, 1, "black", "white", 2, 127, 128, 253, 254)


def box_cases() -> list[BoxCase]:
    cases = []
    for f in BOX_FACTORS:
        for c in BOX_CHANNELS:
            cases.append(BoxCase(5 * f, 3 * f, c, f))
            cases.append(BoxCase(4 * f + (f > 1), 6 * f + f - 1, c, f))  # neither a multiple (factor 1: everything is)
    return cases


def box_image(case: BoxCase) -> np.ndarray:
    """Random bytes; every third box black, white (the means 0 and 255) or -- even factors -- half ``k`` and half ``k + 1``, whose
    mean is exactly ``k + .5``, for even and odd ``k``."""
    rng = np.random.default_rng([SEED, 19, *case])
    img = rng.integers(0, 256, (case.h, case.w, case.c), dtype=np.uint8)
    f, j = case.factor, 0
    for by in range(case.h // f):
        for bx in range(case.w // f):
            if (by + bx) % 3:
                continue
            box = img[by * f:(by + 1) * f, bx * f:(bx + 1) * f]
            pick = BOX_FILLS[j % len(BOX_FILLS)]
            j += 1
            if pick in ("black", "white"):
                box[:] = 0 if pick == "black" else 255
            elif f % 2 == 0:
                k = pick
                half = np.full(f * f, k, np.uint8)
                half[rng.permutation(f * f)[:f * f // 2]] = k + 1
                box[:] = half.reshape(f, f, 1)
    return img


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 2: seeded random sweep
# ------------------------------------------------------------------------------------------------------------------------------------
RANDOM_COUNT = 24
FORM_FLOOR = 4  # cases per form / path in each random list


def _draw_hw(rng, kind: int):
    """Height and width drawn independently, on both sides of the 36,864-pixel limit."""
    if kind == 0:
        return int(rng.integers(1, 193)), int(rng.integers(1, 193))
    if kind == 1:
        return int(rng.integers(150, 261)), int(rng.integers(150, 261))
    if kind == 2:  # noqa: PLR2004
        return int(rng.integers(1, 9)), int(rng.integers(1000, 30001))
    return int(rng.integers(200, 701)), int(rng.integers(200, 701))


def random_label_cases() -> list[LabelCase]:
    rng = np.random.default_rng([SEED, 1])
    cases = []
    for i in range(RANDOM_COUNT):
        h, w = _draw_hw(rng, i % 4)
        if i % 8 >= 4:  # noqa: PLR2004
            h, w = w, h
        names = tuple(f"random{rng.uniform(0.05, 0.95):.3f}#{i}" for _ in range(int(rng.integers(1, 4))))
        cases.append(LabelCase(h, w, (4, 8)[int(rng.integers(0, 2))], names))
    return cases


def random_morph_cases() -> list[MorphCase]:
    rng = np.random.default_rng([SEED, 2])
    cases = []
    for i in range(RANDOM_COUNT):
        h, w = int(rng.integers(1, 151)), int(rng.integers(1, 151))
        if i % 2 == 0:
            w = 4 * max(1, w // 4)
        reach_x = 4 if i % 4 < 3 else 7  # noqa: PLR2004
        offs = tuple((int(rng.integers(-9, 10)), int(rng.integers(-reach_x, reach_x + 1))) for _ in range(int(rng.integers(1, 13))))
        cases.append(MorphCase(f"random {i}", h, w, offs, src_off=int(i % 6 == 4), n=int(rng.integers(1, 4))))  # noqa: PLR2004
    return cases


def random_area_cases() -> list[tuple[AreaCase, int]]:
    """(case, min_keep) pairs."""
    rng = np.random.default_rng([SEED, 3])
    cases = []
    for i in range(16):
        h, w = _draw_hw(rng, i % 2)
        if i % 4 < 2:  # noqa: PLR2004
            w = 4 * max(1, w // 4)
        else:
            h, w = h | 1, w | 1  # an odd pixel count: the scalar loads
        planes = tuple(f"random{rng.uniform(0.2, 0.8):.3f}#{i}/{(4, 8)[int(rng.integers(0, 2))]}" for _ in range(int(rng.integers(1, 4))))
        cases.append((AreaCase(h, w, planes), int(rng.integers(1, 31))))
    return cases


# ------------------------------------------------------------------------------------------------------------------------------------
# device runners (shared by the test module and the fall-back child)
# ------------------------------------------------------------------------------------------------------------------------------------
WS_SENTINEL = -123456789  # no rank, root index or flag ever has this value


def dev_label(masks: np.ndarray, conn: int):
    """``tia_ccl_label_i32`` on [n, h, w] bytes: (labels, counts, whether the scratch buffer was written -- the LDS form leaves it
    alone, the multi-launch form keeps its ranks there)."""
    import torch

    from tiatoolbox_amd import _lib

    m = torch.from_numpy(masks).cuda()
    n, h, w = m.shape
    labels = torch.full((n, h, w), -7, dtype=torch.int32, device="cuda")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ws = torch.full((n * h * w,), WS_SENTINEL, dtype=torch.int32, device="cuda")
    rc = _lib.load().tia_ccl_label_i32(m.data_ptr(), n, h, w, conn, labels.data_ptr(), count.data_ptr(), ws.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_ccl_label_i32")
    return labels.cpu().numpy(), count.cpu().numpy(), bool((ws != WS_SENTINEL).any())


def dev_fill(masks: np.ndarray) -> np.ndarray:
    import torch

    from tiatoolbox_amd.tools import _img_device as img

    return img.fill_holes(torch.from_numpy(masks).cuda()).cpu().numpy()


def dev_area_filter(labels: np.ndarray, min_keep: int) -> np.ndarray:
    import torch

    from tiatoolbox_amd.tools import _img_device as img

    return img.label_area_filter(torch.from_numpy(labels).cuda(), min_keep).cpu().numpy()


def small_area_cases() -> list[AreaCase]:
    return [c for c in area_cases() if label_form(c.h, c.w) == "lds"]


def child_main(out_path: str) -> None:
    assert os.environ.get("TIA_DEV") == "1" and os.environ.get("TIA_NO_CCL_TILE"), "the child runs with the LDS form switched off"
    out = {}
    for i, case in enumerate(small_label_cases()):
        labels, count, touched = dev_label(mask_bytes(case.patterns, case.h, case.w), case.conn)
        out[f"label_{i}"], out[f"count_{i}"], out[f"touched_{i}"] = labels, count, np.array(touched)
        if case.conn == 4:  # noqa: PLR2004
            out[f"fill_{i}"] = dev_fill(mask_bytes(case.patterns, case.h, case.w, binary=True))
    for i, case in enumerate(small_area_cases()):
        labels = area_labels(case)
        for keep in case.min_keeps:
            out[f"area_{i}_{keep}"] = dev_area_filter(labels, keep)
    np.savez(out_path, **out)
    print(f"child: {len(out)} arrays")


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    if len(sys.argv) == 3 and sys.argv[1] == "--child":  # noqa: PLR2004
        child_main(sys.argv[2])
    else:
        sys.exit("usage: _imgops_ref.py --child OUT.npz")

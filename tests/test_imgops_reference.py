"""The image primitives of ``csrc/imgops.hip`` -- connected-component labelling, the area filter, binary morphology, hole filling, grey
conversion, histogram, threshold, the per-image LUT and box down-sampling -- each against a plain NumPy / SciPy reference of the same
operation, in BOTH forms or paths of its kernel.  Every value is an integer, so every comparison is by equality.

Tier 1: fixed cases (the LDS and the multi-launch form of labelling and hole filling on both sides of the 36,864-pixel limit, a second
round of every capped grid, widths around the 64-pixel wave cut, adversarial patterns; the ``int4`` and the scalar path of the area
filter; the bit-window and the generic path of the morphology, the latter by each of its four triggers; byte kernels at every
alignment and tail).  Tier 2: a seeded random sweep.  Tier 3: the small cases once more in a fresh child process that has the LDS form
switched off, which is the only way to the multi-launch forms below the limit.  References, case lists and comparisons are in
``tests/_imgops_ref.py``; the tests without the ``gpu`` mark check them on the host: hand-computed examples, that the lists hold the
edges and reach every form and path, and that each comparison rejects a reference that is wrong in a way a kernel can be."""

from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _imgops_ref as R  # noqa: E402, N812

GUARD = 0xA5
FIRST = "first differing element"


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
def test_references_match_hand_computed_examples():
    """One written-out example per reference."""
    m = np.array([[1, 0, 1, 0],
                  [0, 1, 0, 0],
                  [0, 0, 0, 1],
                  [1, 1, 0, 1]], np.uint8)
    lab4, n4 = R.label_ref(m, 4)
    assert n4 == 5 and lab4.tolist() == [[1, 0, 2, 0], [0, 3, 0, 0], [0, 0, 0, 4], [5, 5, 0, 4]]  # noqa: PLR2004
    lab8, n8 = R.label_ref(m, 8)  # the three upper pixels join through (1, 1)
    assert n8 == 3 and lab8.tolist() == [[1, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 2], [3, 3, 0, 2]]  # noqa: PLR2004
    # areas 1, 1, 1, 2, 2: min_keep 2 keeps labels 4 and 5 with their numbers
    assert R.area_filter_ref(lab4, 2).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 4], [5, 5, 0, 4]]
    assert np.array_equal(R.area_filter_ref(lab4, 0), lab4) and not R.area_filter_ref(lab4, 3).any()
    # one set pixel at (1, 2); element {(0, 0), (1, -2)}: out[y, x] = src[y, x] | src[y + 1, x - 2] -> (1, 2) and (0, 4)
    src = np.zeros((3, 5), np.uint8)
    src[1, 2] = 7
    assert np.argwhere(R.morph_ref(src, ((0, 0), (1, -2)), "dilate")).tolist() == [[0, 4], [1, 2]]
    # erosion of a full plane by (0, -1) and (2, 0) stays full (outside = 1); with one clear pixel at (1, 2) the outputs (1, 3) and
    # (-1, 2) would clear: only (1, 3) exists
    full = np.ones((3, 5), np.uint8)
    assert R.morph_ref(full, ((0, -1), (2, 0)), "erode").all()
    full[1, 2] = 0
    assert np.argwhere(R.morph_ref(full, ((0, -1), (2, 0)), "erode") == 0).tolist() == [[1, 3]]
    assert not R.morph_ref(np.ones((3, 5), np.uint8), ((0, -1),), "erode", erode_outside=0)[:, 0].any()
    ring = np.array([[0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0]], np.uint8)
    assert R.fill_ref(ring).tolist() == [[0, 1, 1, 0], [1, 1, 1, 1], [0, 1, 1, 0]]
    # grey: (255 * (9798 + 19235 + 3735) + 16384) >> 15 = 255; pure red 255 * 9798 + 16384 = 2514874 >> 15 = 76; (1, 1, 1) -> 1
    assert R.gray_ref(np.array([[255, 255, 255], [255, 0, 0], [1, 1, 1], [0, 0, 2]], np.uint8)).tolist() == [255, 76, 1, 0]
    h = R.hist_ref(np.array([3, 3, 255, 0], np.uint8))
    assert (h[0], h[3], h[255], h.sum()) == (1, 2, 1, 4)
    lut = np.stack([np.arange(256, dtype=np.uint8)[::-1], np.full(256, 9, np.uint8)])
    assert R.lut_ref(np.array([[0, 5], [7, 200]], np.uint8), lut).tolist() == [[255, 250], [9, 9]]
    # boxes of 2 x 2: sums 2 (0.5 -> 0), 6 (1.5 -> 2), 10 (2.5 -> 2), 7 (1.75 -> 2); the third row and the fifth column are dropped
    img = np.array([[0, 1, 1, 2, 9], [1, 0, 2, 1, 9], [2, 3, 1, 2, 9], [3, 2, 2, 2, 9], [9, 9, 9, 9, 9]], np.uint8)[..., None]
    assert R.box_ref(img, 2)[..., 0].tolist() == [[0, 2], [2, 2]] and R.box_ref(img, 2, half_up=True)[..., 0].tolist() == [[1, 2], [3, 2]]
    assert R.box_ref(img, 1).tolist() == img.tolist() and R.box_ref(img, 5).tolist() == [[[4]]]  # 106 / 25 = 4.24


def test_morph_reference_equals_scipy_with_the_mirrored_element():
    """The shifts equal ``binary_dilation`` with the element mirrored about its anchor and ``binary_erosion(border_value=1)`` with
    the element itself, on an asymmetric element (odd-sized, anchor at the centre)."""
    elem = np.zeros((11, 9), np.uint8)
    for dy, dx in R.ASYMMETRIC:
        elem[dy + 5, dx + 4] = 1
    for k, src in enumerate(R.morph_planes(R.MorphCase("host", 30, 44, R.ASYMMETRIC, n=3))):
        assert np.array_equal(R.morph_ref(src, R.ASYMMETRIC, "dilate"), ndimage.binary_dilation(src != 0, structure=elem[::-1, ::-1])), k
        assert np.array_equal(R.morph_ref(src, R.ASYMMETRIC, "erode"), ndimage.binary_erosion(src != 0, structure=elem, border_value=1)), k
        assert not np.array_equal(R.morph_ref(src, R.ASYMMETRIC, "dilate"), ndimage.binary_dilation(src != 0, structure=elem)), k


@pytest.mark.parametrize("factor", R.BOX_FACTORS)
def test_float32_box_rule_equals_the_exact_mean_rounded_half_to_even(factor):
    """``rint(float32(sum) * float32(1 / area))`` for every possible sum of the factor equals the exact rule, so the integer reference
    is what the header promises at this factor."""
    assert np.array_equal(R.box_float32_rule(factor), R.box_exact_rule(factor))


def test_constants_restate_the_source():
    assert R.CCL_TILE_MAX_PIXELS == 192 * 192 and R.ROUND_LANES == 1048576 and R.HIST_ROUND_BYTES == 2097152  # noqa: PLR2004
    assert R.LUT_ROUND_BYTES == 8388608 and (R.RANK_TILE, R.LDS_RANK_TILE, R.AREA_BLOCK_PIXELS) == (8192, 4096, 16384)  # noqa: PLR2004
    src = (Path(__file__).resolve().parent.parent / "tiatoolbox_amd" / "csrc" / "imgops.hip").read_text()
    common = (Path(__file__).resolve().parent.parent / "tiatoolbox_amd" / "csrc" / "common.hpp").read_text()
    assert "constexpr long kCclTileMaxPixels = 36864;" in common and "constexpr int BT = 256;" in src
    assert "dim3 grid(nblocks(hw, BT, 4096), (unsigned)n);" in src and "nblocks(n >> 2 ? n >> 2 : 1, BT, 2048)" in src
    assert "nblocks((len + 15) / 16, BT, 2048)" in src and "nblocks(hw, BT * 4 * 16, n >= 64 ? 8 : 64)" in src
    assert "base += 8192" in src and "base += 4096" in src and "if (dx < -4 || dx > 4)" in src and "if (rows == 16)" in src


def test_label_case_lists_hold_the_named_shapes_and_patterns():  # noqa: C901
    lds, multi = set(R.LDS_SHAPES), set(R.MULTI_SHAPES)
    assert {(1, 1), (1, 200), (200, 1), (192, 192), (191, 193)} <= lds and {63, 64, 65} <= {w for _, w in lds}
    assert all(R.label_form(h, w) == "lds" for h, w in lds) and 192 * 192 == R.CCL_TILE_MAX_PIXELS
    assert {(193, 192), (1, 40000), (40000, 1), (1024, 1024)} <= multi and all(R.label_form(h, w) == "multi-launch" for h, w in multi)
    assert 192 * 192 < 193 * 192 and any(w % 4 and h * w % 4 for h, w in multi) and any(h * w > R.ROUND_LANES for h, w in multi)
    assert 1024 * 1024 == R.ROUND_LANES  # exactly one round: the plane above it is the one that makes a second
    cases = R.label_cases()
    for h, w in lds | multi:
        mine = [c for c in cases if (c.h, c.w) == (h, w)]
        for conn in (4, 8):
            names = [p for c in mine if c.conn == conn for p in c.patterns]
            assert sorted(names) == sorted(p for p in R.PATTERNS if R.holds(p, h, w)), (h, w, conn)
            assert {c.n for c in mine if c.conn == conn} == {1, 3}, (h, w)
        if min(h, w) >= 7:  # noqa: PLR2004
            assert len({p for c in mine for p in c.patterns}) == len(R.PATTERNS) == 14  # noqa: PLR2004
    assert {c.conn for c in cases if c.n >= 64} == {4, 8} and all(R.label_form(c.h, c.w) == "lds" for c in cases if c.n >= 64)  # noqa: PLR2004
    assert {"random0.3", "random0.5", "random0.62", "random0.9", "empty", "full"} <= set(R.PATTERNS)
    for p in R.PATTERNS:  # holds() is make_plane()'s own answer
        for h, w in ((1, 1), (1, 9), (4, 4), (6, 6), (7, 7), (9, 2)):
            assert (R.make_plane(p, h, w) is not None) == R.holds(p, h, w), (p, h, w)
    # what the patterns are for, on a plane that crosses the 64-pixel wave cut in every row
    h, w = 21, 131
    checker = R.make_plane("checker", h, w)
    assert R.label_ref(checker, 4)[1] == (h * w + 1) // 2 and R.label_ref(checker, 8)[1] == 1
    for name in ("serpentine", "comb"):
        assert R.label_ref(R.make_plane(name, h, w), 4)[1] == 1 and not R.make_plane(name, h, w).all(), name
    assert R.label_ref(R.make_plane("comb", h, w), 4)[0][0, ::2].tolist() == [1] * 66  # every tooth carries the first tooth's label
    for name in ("diag_down", "diag_up"):
        m = R.make_plane(name, h, w)
        assert R.label_ref(m, 4)[1] == int(m.sum()) > R.label_ref(m, 8)[1] > 1, name
    rings = R.make_plane("rings", h, w)
    assert R.label_ref(rings, 8)[1] == 3 and R.fill_ref(rings).sum() == (h - 2) * (w - 2) > rings.sum()  # noqa: PLR2004
    corner, diag = R.make_plane("corner_ring", h, w), R.make_plane("diag_hole", h, w)
    assert np.array_equal(R.fill_ref(corner), corner) and not corner[0, 0] and not corner[h - 1, w - 1]  # the corner pixels stay open
    filled = R.fill_ref(diag)
    assert filled.sum() == diag.sum() + 4 and filled[1, 1] and filled[h - 2, w - 2] and not filled[0, 0] and not filled[2, 2]
    masks = R.mask_bytes(("random0.5", "full", "checker"), 9, 11)
    assert set(np.unique(masks[0])) == {0, *R.FG_BYTES} and set(np.unique(masks[1])) == {255} and masks.dtype == np.uint8
    assert set(np.unique(R.mask_bytes(("random0.5",), 9, 11, binary=True))) == {0, 1}


def test_area_filter_cases_hold_the_named_edges():
    cases = R.area_cases()
    assert {R.area_path(c.h, c.w) for c in cases} == {"int4", "scalar"}
    for c in cases:
        assert c.min_keeps == (0, 1, 10, c.h * c.w, c.h * c.w + 1)
    for path in ("int4", "scalar"):  # one component covering a plane of more than a million pixels, through both loads
        assert any(R.area_path(c.h, c.w) == path and c.h * c.w > R.ROUND_LANES and "full/4" in c.planes for c in cases), path
        assert any(R.area_path(c.h, c.w) == path and c.n >= R.AREA_MANY_PLANES for c in cases), path
    assert any("checker/4" in c.planes and c.h * c.w >= R.ROUND_LANES for c in cases)
    # the grid choice of area_count_kernel, each on a case of the list: 64 workgroups per plane binding (n < 64), 8 binding (n >= 64)
    capped64 = [c for c in cases if c.n < R.AREA_MANY_PLANES and R.area_count_blocks(c.n, c.h, c.w) == 64 < -(-c.h * c.w // R.AREA_BLOCK_PIXELS)]  # noqa: PLR2004
    capped8 = [c for c in cases if c.n >= R.AREA_MANY_PLANES and R.area_count_blocks(c.n, c.h, c.w) == 8 < -(-c.h * c.w // R.AREA_BLOCK_PIXELS)]  # noqa: PLR2004
    for capped, blocks in ((capped64, 64), (capped8, 8)):
        assert {R.area_path(c.h, c.w) for c in capped} == {"int4", "scalar"}, blocks
        # every workgroup sweeps 1024 pixels per iteration, more than 16 times: the per-lane run cache carries over
        assert all(c.h * c.w > blocks * 16 * 1024 for c in capped) and any("full/4" in c.planes for c in capped), blocks
    assert any(R.area_count_blocks(c.n, c.h, c.w) == 1 and c.n >= R.AREA_MANY_PLANES for c in cases)
    assert R.area_count_blocks(63, 384, 512) == 12 and R.area_count_blocks(64, 384, 512) == 8  # noqa: PLR2004  (n >= 64 is what caps it)
    direct = [(c, k) for c in cases for k, s in enumerate(c.planes) if s.startswith("direct")]
    assert len(direct) >= 3 and {R.area_path(c.h, c.w) for c, _ in direct} == {"int4", "scalar"}  # noqa: PLR2004
    for c, k in direct:
        lab = R.area_labels(c)[k]
        ids = np.unique(lab[lab > 0])
        assert ids.max() == c.h * c.w and len(ids) < ids.max() // 4 and lab.dtype == np.int32 and (lab == 0).any()
        areas = np.bincount(lab.ravel())
        assert (areas[ids] < 10).any() and (areas[ids] >= 10).any()  # noqa: PLR2004  (min_keep 10 separates them)
    assert R.label_ref(R.make_plane("checker", 8, 8), 4)[0].max() == 32  # noqa: PLR2004


def test_morphology_cases_hold_the_named_edges_and_reach_both_paths():
    cases = R.morph_cases()
    fast = [c for c in cases if R.morph_path(c) == "fast"]
    assert all(c.w % 4 == 0 for c in fast)
    for o in ((0, 4), (0, -4), (3, -4), (-8, 0)):
        assert any(c.offsets == (o,) for c in fast), o
    assert sum(c.name.startswith("ellipse") for c in cases) == 4 and any(c.name == "ellipse (5, 5)" for c in fast)  # noqa: PLR2004
    assert R.ellipse_offsets((5, 5)) == tuple((dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if abs(dy) < 2 or dx == 0)  # noqa: PLR2004
    assert any(len({dy for dy, _ in c.offsets}) == 16 for c in fast) and any(len(set(c.offsets)) < len(c.offsets) for c in fast)  # noqa: PLR2004
    assert {dx for _, dx in R.SIXTEEN_ROWS} == set(range(-4, 5))
    assert any(c.w == 4 and c.h > 1 for c in fast) and any(c.h == 1 and c.w > 4 for c in fast) and any(c.n > 2 for c in fast)  # noqa: PLR2004
    for trigger in ("w % 4", "|dx| > 4", "more than 16 rows", "unaligned source"):  # each alone
        assert any(R.morph_triggers(c) == {trigger} for c in cases), trigger
    assert any(max(abs(dx) for _, dx in c.offsets) == 5 and R.morph_triggers(c) == {"|dx| > 4"} for c in cases)  # noqa: PLR2004
    assert any(len({dy for dy, _ in c.offsets}) == 17 and max(abs(dx) for _, dx in c.offsets) <= 4 for c in cases)  # noqa: PLR2004
    assert any(c.h * c.w > 4 * R.ROUND_LANES for c in fast)  # more quads than one round of the grid has lanes
    for c in cases:  # the planes reach every border, set (dilation) and clear (erosion)
        if c.n < 2 or c.h * c.w > 100000:  # noqa: PLR2004  (the one-plane case of the second grid round uses the same generator)
            continue
        p = R.morph_planes(c)
        assert p[0, 0, 0] and p[0, -1, -1] and not p[1, 0, 0] and not p[1, -1, -1] and set(np.unique(p[1])) - {0, 1}, c.name
    mirrored = {(-dy, -dx) for dy, dx in R.ASYMMETRIC}
    assert not mirrored & (set(R.ASYMMETRIC) - {(0, 0)})  # no offset of the element is another one's mirror image


def test_byte_and_box_cases_hold_the_named_edges():
    assert {1, 3, 15, 16, 17} <= set(R.BYTE_LENGTHS) and {n % 4 for n in R.BYTE_LENGTHS if n > 17} == {0, 1, 2, 3}  # noqa: PLR2004
    assert R.BYTE_OFFSETS == (0, 1, 2, 3) and R.LUT_OFFSETS == tuple(range(16)) and R.THRESHOLDS == (0, 1, 128, 255, 256)
    assert R.HIST_BIG > 2 * R.HIST_ROUND_BYTES and R.LUT_BIG > 2 * R.LUT_ROUND_BYTES and R.HIST_BIG % 4 and R.LUT_BIG % 16
    assert sum(n % 16 != 0 for n in R.BYTE_LENGTHS) >= 8  # noqa: PLR2004  (successive images of a LUT call alternate between its paths)
    assert len(np.unique(R.byte_data(1000, "ramp"))) == 256 and len(np.unique(R.byte_data(4099, "random"))) == 256  # noqa: PLR2004
    assert len(np.unique(R.byte_data(1003, "constant"))) == 1 and len(np.unique(R.gray_ref(R.byte_data(3 * 4099, "random")))) > 200  # noqa: PLR2004
    cases = R.box_cases()
    assert {(c.factor, c.c) for c in cases} == {(f, c) for f in (1, 2, 3, 7, 16, 49) for c in (1, 3, 4)}
    for f in (2, 3, 7, 16, 49):
        mine = [c for c in cases if c.factor == f]
        assert any(c.h % f == 0 and c.w % f == 0 for c in mine) and any(c.h % f and c.w % f for c in mine), f
    for c in cases:
        if c.factor % 2:
            continue
        img = R.box_image(c)
        th, tw, area = c.h // c.factor, c.w // c.factor, c.factor ** 2
        sums = img[:th * c.factor, :tw * c.factor].astype(np.int64).reshape(th, c.factor, tw, c.factor, c.c).sum(axis=(1, 3))
        halves = sums[2 * (sums % area) == area] // area
        assert (halves % 2 == 0).any() and (halves % 2 == 1).any() and (sums == 0).any() and (sums == 255 * area).any(), c


def test_fixed_cases_reach_every_form_and_path():
    """From the shapes alone: both forms of labelling / hole filling with one and with two grid rounds, sweeps of more than one
    ranking tile in both forms, both loads of the area filter, both morphology paths."""
    cases = R.label_cases()
    assert {R.label_form(c.h, c.w) for c in cases} == {"lds", "multi-launch"}
    assert {R.grid_rounds(c.h, c.w) for c in cases if R.label_form(c.h, c.w) == "multi-launch"} == {1, 2}
    assert any(c.h * c.w > R.LDS_RANK_TILE for c in R.small_label_cases()) and any(c.h * c.w <= R.LDS_RANK_TILE for c in R.small_label_cases())
    multi = [c for c in cases if R.label_form(c.h, c.w) == "multi-launch"]
    assert any(c.h * c.w % 4 for c in multi) and any(c.h * c.w % 4 == 0 for c in multi) and all(c.h * c.w > R.RANK_TILE for c in multi)
    assert any(c.w < 64 for c in cases) and any(c.w % 64 for c in multi) and any(c.w % 64 == 0 for c in multi)  # noqa: PLR2004
    assert {R.morph_path(c) for c in R.morph_cases()} == {"fast", "generic"}
    assert {R.area_path(c.h, c.w) for c in R.area_cases()} == {"int4", "scalar"}
    assert R.small_area_cases() and R.small_label_cases()


def test_random_sweep_is_reproducible_and_reaches_both_forms_and_paths():
    labels, morph, area = R.random_label_cases(), R.random_morph_cases(), R.random_area_cases()
    assert (labels, morph, area) == (R.random_label_cases(), R.random_morph_cases(), R.random_area_cases())
    assert len(labels) == len(morph) == R.RANDOM_COUNT
    for form in ("lds", "multi-launch"):
        assert sum(R.label_form(c.h, c.w) == form and c.h != c.w for c in labels) >= R.FORM_FLOOR, form
    assert {c.conn for c in labels} == {4, 8} and {c.n for c in labels} == {1, 2, 3}
    assert any(c.h > 8 * c.w for c in labels) and any(c.w > 8 * c.h for c in labels)
    for path in ("fast", "generic"):
        assert sum(R.morph_path(c) == path for c in morph) >= R.FORM_FLOOR, path
    assert {frozenset(R.morph_triggers(c)) for c in morph} >= {frozenset(), frozenset({"w % 4"}), frozenset({"unaligned source"}),
                                                                frozenset({"|dx| > 4"})}
    for path in ("int4", "scalar"):
        assert sum(R.area_path(c.h, c.w) == path for c, _ in area) >= R.FORM_FLOOR, path
    assert all(1 <= keep <= 30 for _, keep in area)  # noqa: PLR2004


def test_comparisons_reject_a_subtly_wrong_reference():  # noqa: PLR0915
    """Each comparison passes for the reference itself and fails, naming the first differing element, for what a kernel with the
    named fault would return."""
    def rejected(label, bad, good, src=None):
        R.check_equal(label, good.copy(), good, src)
        with pytest.raises(AssertionError, match=FIRST):
            R.check_equal(label, bad, good, src)
            pytest.fail(f"accepted '{label}'")

    case = R.MorphCase("sensitivity", 20, 24, R.ASYMMETRIC, n=2)
    planes = R.morph_planes(case)
    mirrored = tuple((-dy, -dx) for dy, dx in R.ASYMMETRIC)
    for op in ("dilate", "erode"):
        good = np.stack([R.morph_ref(p, R.ASYMMETRIC, op) for p in planes])
        rejected(f"{op}: the element mirrored", np.stack([R.morph_ref(p, mirrored, op) for p in planes]), good, planes)
        for o in R.ONE_OFFSETS:  # and on each of the one-offset elements
            one = np.stack([R.morph_ref(p, (o,), op) for p in planes])
            rejected(f"{op}: offset {o} mirrored", np.stack([R.morph_ref(p, ((-o[0], -o[1]),), op) for p in planes]), one, planes)
    good = np.stack([R.morph_ref(p, R.ASYMMETRIC, "erode") for p in planes])
    rejected("erode: the border taken as 0", np.stack([R.morph_ref(p, R.ASYMMETRIC, "erode", erode_outside=0) for p in planes]), good)
    for name in ("diag_down", "diag_up", "checker", "random0.5"):
        m = R.make_plane(name, 20, 24)[None]
        rejected(f"{name}: connectivity 4 and 8 swapped", R.label_ref(m[0], 8)[0][None], R.label_ref(m[0], 4)[0][None], m)
        rejected(f"{name}: connectivity 8 and 4 swapped", R.label_ref(m[0], 4)[0][None], R.label_ref(m[0], 8)[0][None], m)
    m = R.make_plane("random0.3", 20, 24)
    for conn in (4, 8):
        good = R.label_ref(m, conn)[0]
        column_major = R.label_ref(m.T, conn)[0].T
        assert np.array_equal(column_major != 0, good != 0)  # the same components, numbered down the columns
        rejected(f"labels numbered in column-major order, connectivity {conn}", column_major[None], good[None], m[None])
    hole = R.make_plane("diag_hole", 9, 11)
    left_open = ndimage.binary_fill_holes(hole, structure=np.ones((3, 3))).astype(np.uint8)  # an 8-connected background leaks through
    assert R.fill_ref(hole)[1, 1] == 1 and left_open[1, 1] == 0
    rejected("the corner-touching hole left open", left_open[None], R.fill_ref(hole)[None], hole[None])
    with pytest.raises(AssertionError, match=FIRST) as exc:
        R.check_equal("message", left_open[None], R.fill_ref(hole)[None], hole[None])
    assert "plane 0, row 1, column 1: got 0, reference 1" in str(exc.value) and "source around it" in str(exc.value)
    lab = np.zeros((6, 8), np.int32)
    lab[0, :] = 1
    lab[1, :2] = 1      # area 10
    lab[3, :] = 2
    lab[4, 0] = 2       # area 9
    lab[5, 1:] = 3      # area 7
    lab[4, 4:8] = 3     # area 11
    assert np.bincount(lab.ravel())[1:].tolist() == [10, 9, 11]
    good = R.area_filter_ref(lab, 10)
    assert sorted(np.unique(good)) == [0, 1, 3]
    rejected("min_keep off by one (up)", R.area_filter_ref(lab, 11)[None], good[None], lab[None])
    rejected("min_keep off by one (down)", R.area_filter_ref(lab, 9)[None], good[None], lab[None])
    for c in (R.BoxCase(10, 6, 3, 2), R.BoxCase(80, 48, 1, 16)):
        img = R.box_image(c)
        rejected(f"box rounding half up {c}", R.box_ref(img, c.factor, half_up=True), R.box_ref(img, c.factor))
    data = R.byte_data(4099, "random")
    rejected("one histogram bin shifted", R.hist_ref(data, shift_bin=37), R.hist_ref(data))
    rgb = R.byte_data(3 * 1001, "random")
    rejected("grey without the rounding term", ((rgb.reshape(-1, 3).astype(np.int64) @ np.array([9798, 19235, 3735])) >> 15).astype(np.uint8),
             R.gray_ref(rgb))
    with pytest.raises(AssertionError, match="shape"):
        R.check_equal("shape", np.zeros((2, 3), np.uint8), np.zeros((3, 2), np.uint8))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _shape_id(shape) -> str:
    return f"{shape[0]}x{shape[1]}"


def _check_label_case(case, labels, count, touched, tag=""):
    masks = R.mask_bytes(case.patterns, case.h, case.w)
    for k, name in enumerate(case.patterns):
        exp, n = R.label_ref(masks[k], case.conn)
        label = f"{tag}labelling {case.h} x {case.w}, connectivity {case.conn}, pattern {name} (plane {k} of {case.n})"
        assert int(count[k]) == n, f"{label}: count {int(count[k])}, reference {n}"
        R.check_equal(label, labels[k][None], exp[None], masks[k][None])
    return bool(masks.any()) and touched


def _check_fill_case(case, filled, tag=""):
    masks = R.mask_bytes(case.patterns, case.h, case.w, binary=True)
    for k, name in enumerate(case.patterns):
        R.check_equal(f"{tag}hole filling {case.h} x {case.w}, pattern {name} (plane {k} of {case.n})", filled[k][None],
                      R.fill_ref(masks[k])[None], masks[k][None])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.LDS_SHAPES + R.MULTI_SHAPES, ids=_shape_id)
def test_labelling_matches_scipy_in_both_forms(shape):
    """Tier 1 of ``tia_ccl_label_i32``: every pattern the shape holds, both connectivities, calls of one and of three planes.  The
    scratch buffer shows which form ran: the LDS form never writes it, the multi-launch form keeps its ranks there."""
    form = R.label_form(*shape)
    for case in R.shape_label_cases(*shape):
        labels, count, touched = R.dev_label(R.mask_bytes(case.patterns, case.h, case.w), case.conn)
        used_ws = _check_label_case(case, labels, count, touched)
        has_fg = bool(R.mask_bytes(case.patterns, case.h, case.w).any())
        assert touched == (form == "multi-launch" and has_fg) and used_ws == touched, (case, form, touched)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.LDS_SHAPES + R.MULTI_SHAPES, ids=_shape_id)
def test_hole_filling_matches_scipy_in_both_forms(shape):
    """Tier 1 of ``tia_fill_holes_u8`` through ``_img_device.fill_holes``: the same planes as 0/1 bytes."""
    for case in R.shape_label_cases(*shape):
        if case.conn == 4:  # noqa: PLR2004
            _check_fill_case(case, R.dev_fill(R.mask_bytes(case.patterns, case.h, case.w, binary=True)))


@pytest.mark.gpu
def test_labelling_and_hole_filling_of_many_small_planes():
    """One call with n >= 64 planes (one workgroup per plane in the LDS form), through the package's wrappers."""
    import torch

    from tiatoolbox_amd.tools import _img_device as img

    for case in R.many_planes_cases():
        masks = R.mask_bytes(case.patterns, case.h, case.w)
        labels, count = img.ccl_label(torch.from_numpy(masks).cuda(), connectivity=case.conn)
        _check_label_case(case, labels.cpu().numpy(), count.cpu().numpy(), False)
        _check_fill_case(case, R.dev_fill(R.mask_bytes(case.patterns, case.h, case.w, binary=True)))


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(R.area_cases())))
def test_area_filter_matches_bincount(index):
    """Tier 1 of ``tia_label_area_filter_i32``: SciPy's labels of the patterns and label planes handed in directly, both loads, every
    ``min_keep`` of the list."""
    case = R.area_cases()[index]
    labels = R.area_labels(case)
    for keep in case.min_keeps:
        got = R.dev_area_filter(labels, keep)
        for k, spec in enumerate(case.planes):
            R.check_equal(f"area filter {case.h} x {case.w} ({R.area_path(case.h, case.w)}), min_keep {keep}, plane {k} {spec}", got[k][None],
                          R.area_filter_ref(labels[k], keep)[None], labels[k][None])
        survivors = int((got != 0).sum())
        assert keep <= case.h * case.w or survivors == 0
        assert keep > 1 or np.array_equal(got, labels)


def _guarded(data: np.ndarray, off: int):
    """(buffer, view): ``data`` on the device ``off`` bytes behind an allocation base, guard bytes around it."""
    import torch

    flat = torch.full((data.size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 256 == 0
    view = flat[off:off + data.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(data).ravel()))
    return flat, view


def _guards_intact(flat, off: int, length: int) -> bool:
    return bool((flat[:off] == GUARD).all()) and bool((flat[off + length:] == GUARD).all())


def _morph_case(case):
    import torch

    from tiatoolbox_amd.tools import _img_device as img

    planes = R.morph_planes(case)
    flat, view = _guarded(planes, case.src_off)
    src = view.view(case.n, case.h, case.w)
    assert src.data_ptr() % 4 == case.src_off % 4 and src.is_contiguous()
    offs = torch.tensor(case.offsets, dtype=torch.int32, device="cuda").view(-1, 2)
    for op in ("dilate", "erode"):
        got = img.binary_morph(src, offs, op).cpu().numpy()
        for k in range(case.n):
            R.check_equal(f"morphology '{case.name}' ({R.morph_path(case)}) {op} {case.h} x {case.w}, {len(case.offsets)} offsets, plane {k}",
                          got[k][None], R.morph_ref(planes[k], case.offsets, op)[None], planes[k][None])
    assert np.array_equal(view.cpu().numpy(), planes.ravel()) and _guards_intact(flat, case.src_off, planes.size)  # the source is read only


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(R.morph_cases())))
def test_morphology_matches_the_shifted_planes(index):
    """Tier 1 of ``tia_binary_morph_u8``: dilation and erosion on the bit-window path and on the generic loop."""
    from tiatoolbox_amd.tools import _img_device as img

    case = R.morph_cases()[index]
    if case.name.startswith("ellipse"):  # the host-side restatement is the package's own offsets_of(ellipse)
        k = tuple(int(v) for v in case.name[len("ellipse ("):-1].split(","))
        assert img.offsets_of(img.get_structuring_element_ellipse(k), "cuda").cpu().numpy().tolist() == [list(o) for o in case.offsets]
    _morph_case(case)


def _lib_call(name, *args):
    from tiatoolbox_amd import _lib

    _lib.check(getattr(_lib.load(), name)(*args, _lib.current_stream()), name)


OFFSET_PAIRS = [(s, 0) for s in R.BYTE_OFFSETS] + [(0, d) for d in R.BYTE_OFFSETS[1:]] + [(3, 3), (1, 2)]  # (source, destination)


@pytest.mark.gpu
def test_grey_conversion_matches_the_integer_formula():
    """``tia_rgb2gray_u8``: every length and tail, source and destination 0 .. 3 bytes off a dword, nothing written outside."""
    for npix in R.BYTE_LENGTHS:
        for kind in R.BYTE_KINDS:
            rgb = R.byte_data(3 * npix, kind, 1)
            for s_off, d_off in OFFSET_PAIRS:
                _, src = _guarded(rgb, s_off)
                out_flat, out = _guarded(np.full(npix, GUARD, np.uint8), d_off)
                _lib_call("tia_rgb2gray_u8", src.data_ptr(), npix, out.data_ptr())
                R.check_equal(f"rgb2gray {npix} pixels, {kind}, offsets {s_off} / {d_off}", out.cpu().numpy(), R.gray_ref(rgb))
                assert _guards_intact(out_flat, d_off, npix), (npix, kind, s_off, d_off)


@pytest.mark.gpu
def test_histogram_matches_bincount_and_accumulates():
    """``tia_hist256_u8``: every length, tail and alignment, a constant image, more than two rounds of the capped grid, and two calls
    into one buffer."""
    from tiatoolbox_amd.tools import _img_device as img

    for n in (*R.BYTE_LENGTHS, R.HIST_BIG):
        for kind in R.BYTE_KINDS:
            data, more = R.byte_data(n, kind, 2), R.byte_data(n, "random", 3)
            for off in R.BYTE_OFFSETS if n < R.HIST_BIG else (0, 1):
                _, view = _guarded(data, off)
                hist = img.hist256(view)
                R.check_equal(f"hist256 {n} bytes, {kind}, offset {off}", hist.cpu().numpy().astype(np.int64), R.hist_ref(data))
                _, second = _guarded(more, (off + 2) % 4)
                assert img.hist256(second, hist) is hist
                R.check_equal(f"hist256 {n} bytes, {kind}, offset {off}, second call into the same counts",
                              hist.cpu().numpy().astype(np.int64), R.hist_ref(data) + R.hist_ref(more))


@pytest.mark.gpu
@pytest.mark.parametrize("is_rgb", [0, 1])
def test_threshold_matches_the_comparison(is_rgb):
    """``tia_threshold_lt_u8`` and ``tia_threshold_lt_dev_u8``: ``grey < thr`` for thresholds at and beyond both ends of the byte
    range, from the host and from device memory, grey planes and RGB pixels, every length, tail and alignment."""
    import torch

    for npix in R.BYTE_LENGTHS:
        for kind in R.BYTE_KINDS:
            data = R.byte_data(3 * npix if is_rgb else npix, kind, 4)
            grey = R.gray_ref(data) if is_rgb else data
            for s_off, d_off in OFFSET_PAIRS:
                _, src = _guarded(data, s_off)
                for thr in R.THRESHOLDS:
                    exp = (grey.astype(np.int64) < thr).astype(np.uint8)
                    for from_device in (False, True):
                        out_flat, out = _guarded(np.full(npix, GUARD, np.uint8), d_off)
                        if from_device:
                            thr_dev = torch.tensor([thr, 77], dtype=torch.int32, device="cuda")
                            _lib_call("tia_threshold_lt_dev_u8", src.data_ptr(), npix, is_rgb, thr_dev.data_ptr(), out.data_ptr())
                        else:
                            _lib_call("tia_threshold_lt_u8", src.data_ptr(), npix, is_rgb, thr, out.data_ptr())
                        R.check_equal(f"threshold {npix} pixels, is_rgb {is_rgb}, {kind}, thr {thr}, device threshold {from_device}, "
                                      f"offsets {s_off} / {d_off}", out.cpu().numpy(), exp)
                        assert _guards_intact(out_flat, d_off, npix), (npix, kind, thr, s_off, d_off)


def _lut_case(n, length, s_off, d_off, seed):
    import torch

    rng = np.random.default_rng([R.SEED, 23, n, length % 100003, seed])
    imgs = np.stack([R.byte_data(length, R.BYTE_KINDS[(k + seed) % 3], seed + k) for k in range(n)])
    lut = rng.integers(0, 256, (n, 256), dtype=np.uint8)
    lut[0] = np.arange(256, dtype=np.uint8)[::-1]
    _, src = _guarded(imgs, s_off)
    out_flat, out = _guarded(np.full(n * length, GUARD, np.uint8), d_off)
    lut_dev = torch.from_numpy(lut).cuda()
    _lib_call("tia_lut_apply_u8", src.data_ptr(), n, length, lut_dev.data_ptr(), out.data_ptr())
    R.check_equal(f"lut {n} images of {length} bytes, offsets {s_off} / {d_off}", out.cpu().numpy().reshape(n, length), R.lut_ref(imgs, lut))
    assert _guards_intact(out_flat, d_off, n * length), (n, length, s_off, d_off)


@pytest.mark.gpu
def test_lut_matches_the_table_lookup():
    """``tia_lut_apply_u8``: three images per call (with ``len % 16 != 0`` they alternate between the 16-byte and the byte path), bases
    0 .. 15 bytes off, one length beyond two rounds of the capped grid on either path."""
    for length in R.BYTE_LENGTHS:
        for off in R.LUT_OFFSETS:
            _lut_case(3, length, off, off, off)
        _lut_case(3, length, 0, 5, 1)
        _lut_case(3, length, 9, 0, 2)
        _lut_case(1, length, 0, 0, 3)
    _lut_case(2, R.LUT_BIG, 0, 0, 4)
    _lut_case(1, R.LUT_BIG, 1, 0, 5)


@pytest.mark.gpu
def test_box_downsampling_matches_the_exact_mean():
    """``tia_box_downsample_u8``: the exact mean rounded half to even (ties with even and odd integer parts at the even factors),
    dropped rows and columns, 1 / 3 / 4 channels; and the entry point's TIA_EINVAL / TIA_ESIZE returns, which launch nothing."""
    import torch

    from tiatoolbox_amd import _lib

    lib = _lib.load()
    for case in R.box_cases():
        img = R.box_image(case)
        th, tw = case.h // case.factor, case.w // case.factor
        src = torch.from_numpy(img).cuda()
        out_flat, out = _guarded(np.full(th * tw * case.c, GUARD, np.uint8), 0)
        _lib_call("tia_box_downsample_u8", src.data_ptr(), case.h, case.w, case.c, case.factor, out.data_ptr())
        R.check_equal(f"box down-sampling {case}", out.cpu().numpy().reshape(th, tw, case.c), R.box_ref(img, case.factor))
        assert _guards_intact(out_flat, 0, th * tw * case.c), case
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((8 * 8 * 3,), GUARD, dtype=torch.uint8, device="cuda")
    s, o, st = src.data_ptr(), out.data_ptr(), _lib.current_stream()
    for args in ((0, 8, 8, 3, 2, o), (s, 8, 8, 3, 2, 0), (s, 0, 8, 3, 2, o), (s, 8, 0, 3, 2, o), (s, 8, 8, 0, 2, o), (s, 8, 8, 3, 0, o),
                 (s, 8, 8, 3, -1, o), (s, -8, 8, 3, 2, o)):
        assert lib.tia_box_downsample_u8(*args, st) == _lib.TIA_EINVAL, args
    for args in ((s, 8, 8, 3, 4097, o), (s, 8, 8, 3, 9, o), (s, 8, 1, 3, 2, o), (s, 1, 8, 3, 2, o)):
        assert lib.tia_box_downsample_u8(*args, st) == _lib.TIA_ESIZE, args
    assert lib.tia_box_downsample_u8(s, 8, 8, 3, 8, o, st) == 0
    torch.cuda.synchronize()
    assert out[:3].tolist() == [0, 0, 0] and bool((out[3:] == GUARD).all())


@pytest.mark.gpu
def test_random_shapes_match_the_references():
    """Tier 2: the seeded sweep (heights and widths drawn independently on both sides of the LDS limit, random densities, elements,
    ``min_keep``) of labelling, hole filling, the area filter and the morphology."""
    for case in R.random_label_cases():
        masks = R.mask_bytes(case.patterns, case.h, case.w)
        labels, count, touched = R.dev_label(masks, case.conn)
        _check_label_case(case, labels, count, touched, "random sweep: ")
        assert touched == (R.label_form(case.h, case.w) == "multi-launch" and bool(masks.any())), case
        _check_fill_case(case, R.dev_fill(R.mask_bytes(case.patterns, case.h, case.w, binary=True)), "random sweep: ")
    for case, keep in R.random_area_cases():
        labels = R.area_labels(case)
        got = R.dev_area_filter(labels, keep)
        for k, spec in enumerate(case.planes):
            R.check_equal(f"random sweep: area filter {case.h} x {case.w}, min_keep {keep}, plane {k} {spec}", got[k][None],
                          R.area_filter_ref(labels[k], keep)[None], labels[k][None])
    for case in R.random_morph_cases():
        _morph_case(case)


@pytest.mark.gpu
def test_multi_launch_forms_at_small_sizes_in_a_child_process(tmp_path):
    """Tier 3: below 36,864 pixels the multi-launch forms of labelling and hole filling run only when the LDS form is refused or
    switched off.  ONE fresh child process (the switch is read once per process) with ``TIA_DEV=1 TIA_NO_CCL_TILE=1`` in its
    environment runs the small fixed cases of labelling, hole filling and the area filter; its exit status is asserted before
    anything is read, its results are compared with the same references, and the written scratch buffer shows that the multi-launch
    form is what ran."""
    out = tmp_path / "child.npz"
    env = dict(os.environ, TIA_DEV="1", TIA_NO_CCL_TILE="1")
    proc = subprocess.run([sys.executable, str(Path(R.__file__).resolve()), "--child", str(out)], env=env, timeout=900,  # noqa: S603
                          capture_output=True, text=True, check=False)
    assert proc.returncode == 0, f"the child ended with status {proc.returncode}\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"
    got = np.load(out)
    tag = "multi-launch form below the LDS limit: "
    for i, case in enumerate(R.small_label_cases()):
        used_ws = _check_label_case(case, got[f"label_{i}"], got[f"count_{i}"], bool(got[f"touched_{i}"]), tag)
        assert used_ws == bool(R.mask_bytes(case.patterns, case.h, case.w).any()), (case, "the child did not run the multi-launch form")
        if case.conn == 4:  # noqa: PLR2004
            _check_fill_case(case, got[f"fill_{i}"], tag)
    for i, case in enumerate(R.small_area_cases()):
        labels = R.area_labels(case)
        for keep in case.min_keeps:
            for k, spec in enumerate(case.planes):
                R.check_equal(f"{tag}area filter {case.h} x {case.w}, min_keep {keep}, plane {k} {spec}", got[f"area_{i}_{keep}"][k][None],
                              R.area_filter_ref(labels[k], keep)[None], labels[k][None])

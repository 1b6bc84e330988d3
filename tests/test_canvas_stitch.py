"""The NumPy statement of the canvas stitching (``_canvas_ref``) against the CPU oracle and the real reference's fixture, the
properties the shared case lists exist for, and the sensitivity of the comparisons: all on the host.  The device tests
(``test_canvas_stitch_gpu.py``) compare the HIP kernels with the same statement on the same lists."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import semantic as osem

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _canvas_ref as ref  # noqa: E402

GOLD = Path(__file__).parent / "golden"


def same(a, b) -> bool:
    """Equal element by element, a NaN equal to a NaN (the NaN cases carry them into sums and quotients)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _oracle_row(blocks, xs, width):
    oh, ow, c = blocks.shape[1:]
    locs = ref.row_locs(xs, oh, ow)
    locs[:, 2] = np.minimum(locs[:, 2], width)  # as `merge_wsi` clips them
    canvas, count = osem.merge_batch_to_canvas(blocks, locs, (oh, width, c))
    return canvas, count[..., 0]


ROW_CASES = ref.row_merge_cases()
STITCH_CASES = ref.stitch_cases()
FIN_CASES = ref.finalize_cases()


# ------------------------------------------------------------------------------------------------ statement == oracle
def test_row_merge_ref_equals_the_real_reference_fixture():
    gold = np.load(GOLD / "grid_golden.npz")
    blocks, locs = gold["merge_blocks"], gold["merge_locs"]
    assert len(np.unique(locs[:, 1])) == 1 and int(locs[:, 2].max()) <= 60
    row, cnt = ref.row_merge_ref(blocks, locs[:, 0], 60)
    assert same(row[:16], gold["merge_canvas"].astype(np.float32)) and same(cnt[:16], gold["merge_count"][..., 0])
    canvas, count = osem.merge_batch_to_canvas(blocks, locs, (16, 60, 3))
    assert same(row[:16], canvas.astype(np.float32)) and same(cnt[:16], count[..., 0])


@pytest.mark.parametrize("name", list(ROW_CASES))
def test_row_merge_ref_equals_oracle(name):
    blocks, xs, width = ROW_CASES[name]
    row, cnt = ref.row_merge_ref(blocks, xs, width)
    exp_row, exp_cnt = _oracle_row(blocks, xs, width)
    assert row.dtype == np.float32 and cnt.dtype == np.uint8
    assert same(row, exp_row) and same(cnt, exp_cnt)
    oh, ow = blocks.shape[1:3]
    assert ref.within_wide(row, blocks, ref.row_locs(xs, oh, ow), (oh, width), divided=False)


def test_row_merge_ref_equals_oracle_on_the_grid_stride_case():
    blocks, xs, width = ref.grid_stride_case()
    row, cnt = ref.row_merge_ref(blocks, xs, width)
    exp_row, exp_cnt = _oracle_row(blocks, xs, width)
    assert same(row, exp_row) and same(cnt, exp_cnt)
    assert blocks.shape[1] * width > 16384 * 256 and xs[-1] + blocks.shape[2] > width
    assert ref.within_wide(row, blocks, ref.row_locs(xs, 2, 64), (2, width), divided=False)


@pytest.mark.parametrize("name", list(STITCH_CASES))
def test_stitch_ref_equals_oracle(name):
    blocks, locs, shape = STITCH_CASES[name]
    probs, pred = ref.stitch_ref(blocks, locs, shape)
    exp = osem.merge_wsi(blocks, locs, shape)
    assert same(probs, exp) and same(pred, exp.argmax(-1).astype(np.uint8))
    assert ref.within_wide(probs, blocks, locs, shape)


@pytest.mark.parametrize("name", [c["name"] for c in FIN_CASES])
def test_finalize_ref_lies_within_the_float64_bound(name):
    """Two terms, one addition, one division: ``|ref32 - ref64| <= 2 * 2^-24 * (|a| + |b|) / divisor``."""
    case = next(c for c in FIN_CASES if c["name"] == name)
    row_a, cnt_a, ys_a, row_b, cnt_b, ys_b, oh, y0, y1 = ref.finalize_args(case)
    probs, pred = ref.finalize_ref(row_a, cnt_a, ys_a, row_b, cnt_b, ys_b, oh, y0, y1)
    assert probs.shape == (y1 - y0, *row_a.shape[1:]) and pred.shape == probs.shape[:2] and pred.dtype == np.uint8
    total = np.zeros(probs.shape, np.float64)
    mag = np.zeros(probs.shape, np.float64)
    count = np.zeros(probs.shape[:2], np.int64)
    with np.errstate(invalid="ignore"):
        for row, cnt, ys in ((row_a, cnt_a, ys_a), (row_b, cnt_b, ys_b)):
            for y in range(y0, y1):
                if row is not None and 0 <= y - ys < oh:
                    total[y - y0] += row[y - ys].astype(np.float64)
                    mag[y - y0] += np.abs(row[y - ys].astype(np.float64))
                    count[y - y0] += cnt[y - ys].astype(np.int64)
        div = np.where(count % 256 == 0, 1, count % 256).astype(np.float64)[..., None]
        exact = total / div
    finite = np.isfinite(exact)
    assert np.array_equal(np.isfinite(probs), finite)
    assert np.all(np.abs(probs.astype(np.float64)[finite] - exact[finite]) <= (2 * ref.U * mag / div + 2.0 ** -150)[finite])
    assert same(pred, np.argmax(probs, -1).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ the lists are what they claim
def _depth(blocks, xs, width):
    ow = blocks.shape[2]
    depth = np.zeros(width, dtype=np.int64)
    for x in xs:
        depth[max(int(x), 0):min(int(x) + ow, width)] += 1
    return depth


def test_case_lists_have_the_properties_they_exist_for():
    for c in range(1, 9):
        blocks, xs, width = ROW_CASES[f"c{c}"]
        assert blocks.shape[1:] == (5, 12, c) and width == 53 and xs[0] == 0 and list(xs[:9]) == list(range(0, 45, 5))
        assert _depth(blocks, xs, width).max() == 3 and xs[-1] + 12 > width and (blocks < 0).any() and (blocks > 0).any()
    assert ROW_CASES["width1"][0].shape[1:3] == (3, 7) and ROW_CASES["width1"][2] == 1
    assert ROW_CASES["pixel_blocks"][0].shape[1:3] == (1, 1) and ROW_CASES["pixel_blocks"][2] == 9
    assert ROW_CASES["wider_than_canvas"][0].shape[2] == 40 > ROW_CASES["wider_than_canvas"][2] == 17
    # deep and unordered: four deep, and the given-order sums are not the x-sorted sums
    blocks, xs, width = ROW_CASES["deep"]
    assert blocks.shape[1:] == (4, 16, 3) and width == 40 and list(xs) == [20, 0, 10, 5, 15, 24]
    assert _depth(blocks, xs, width).max() >= 4
    order = np.argsort(xs, kind="stable")
    given, _ = ref.row_merge_ref(blocks, xs, width)
    by_x, _ = ref.row_merge_ref(blocks[order], xs[order], width)
    assert (given != by_x).sum() >= 1
    # zero blocks: five over column 2, the third a block of +0.0 / of -0.0 / with one subnormal / with one NaN
    for c in (1, 4):
        for kind in ref.ZERO_KINDS:
            blocks, xs, width = ROW_CASES[f"zero_{kind}_c{c}"]
            assert _depth(blocks, xs, width)[2] == 5
            third, (_, cnt) = blocks[2], ref.row_merge_ref(blocks, xs, width)
            if kind == "plus_zero":
                assert not np.any(third) and not np.signbit(third).any() and cnt[0, 2] == 4
            elif kind == "minus_zero":
                assert not np.any(third) and np.signbit(third).all() and cnt[0, 2] == 4
            elif kind == "subnormal":
                assert np.count_nonzero(third) == 1 and third.max() == np.float32(2.0 ** -149) > 0 and cnt[0, 2] == 5
                assert third.max() < np.finfo(np.float32).tiny
            else:
                assert np.isnan(third).sum() == 1 and np.count_nonzero(np.nan_to_num(third)) == 0 and cnt[0, 2] == 5
    # counts: 300 blocks wrap to 44, 256 to exactly 0 -- in the merge and in finalize's sum of two counts
    assert (ref.row_merge_ref(*ROW_CASES["wrap300"])[1][:, :3] == 44).all() and len(ROW_CASES["wrap300"][0]) == 300
    assert (ref.row_merge_ref(*ROW_CASES["wrap256"])[1][:, :3] == 0).all() and len(ROW_CASES["wrap256"][0]) == 256
    assert np.any(ref.row_merge_ref(*ROW_CASES["wrap256"])[0] != 0)
    by_name = {c["name"]: c for c in FIN_CASES}
    for name, wrapped in (("count_wrap44", 44), ("count_wrap0", 0), ("count_zero", 0)):
        case = by_name[name]
        assert ((case["cnt_a"] + case["cnt_b"]) == wrapped).all() and (case["cnt_a"] + case["cnt_b"]).dtype == np.uint8
    assert (by_name["count_wrap0"]["cnt_a"].astype(int) + by_name["count_wrap0"]["cnt_b"]).min() == 256
    # labels: NaN ties on which np.argmax and a > scan differ, exact ties, signed zeros, negatives, infinities
    v = ref.LABEL_VECTORS
    differ = np.argmax(v, -1) != ref.gt_scan_argmax(v)
    assert differ.sum() >= 1 and np.isnan(v[differ]).any(axis=-1).all()
    assert list(np.argmax(v[7:10], -1)) == [1, 2, 0] and list(ref.gt_scan_argmax(v[7:9])) == [2, 1]
    assert np.signbit(v[2, 1]) and not np.signbit(v[2, 0]) and (v[4] < 0).all() and np.isinf(v[5]).any()
    for name in ("labels_alone", "labels_divided", "labels_two_rows"):
        probs, pred = ref.finalize_ref(*ref.finalize_args(by_name[name]))
        assert (pred != ref.gt_scan_argmax(probs)).any(), name
    assert np.isnan(ref.finalize_ref(*ref.finalize_args(by_name["labels_two_rows"]))[0][0, 5]).sum() == 2  # inf - inf, made by the add
    # geometry: every offset, with rows of a alone, both, b alone and (offset 9) neither inside one range
    for off in ref.FIN_OFFSETS:
        case = by_name[f"c3_off{off}_span"]
        ya = np.arange(case["y0"], case["y1"]) - case["ys_a"]
        yb = np.arange(case["y0"], case["y1"]) - case["ys_b"]
        in_a, in_b = (ya >= 0) & (ya < ref.FIN_OH), (yb >= 0) & (yb < ref.FIN_OH)
        assert (in_a & ~in_b).any() and (in_b & ~in_a).any() and (in_a & in_b).any() == (off < ref.FIN_OH)
        assert (~in_a & ~in_b).any() == (off > ref.FIN_OH)
        if off > ref.FIN_OH:
            probs, pred = ref.finalize_ref(*ref.finalize_args(case))
            assert not probs[~in_a & ~in_b].any() and not pred[~in_a & ~in_b].any()
    # whole canvases: two deep in y, four deep in x, with whole patch rows and single patches masked
    blocks, locs, (h, w) = STITCH_CASES["two_by_four_deep_masked"]
    rows = ref.row_ys_of(locs)
    per_row = np.array([sum(bool(np.any(b)) for b in blocks[locs[:, 1] == y]) for y in rows])
    assert per_row[0] == 0 and per_row[4] == 0 and len(np.unique(per_row)) > 2 and np.diff(rows).max() == 8
    assert ref.wide_ref(blocks, locs, (h, w))[3].max() == 8 and (blocks < 0).any()


# ------------------------------------------------------------------------------------------------ the comparisons are sensitive
def test_a_reference_that_sorts_by_x_fails_the_equality():
    blocks, xs, width = ROW_CASES["deep"]
    order = np.argsort(xs, kind="stable")
    exp_row, exp_cnt = _oracle_row(blocks, xs, width)
    row, cnt = ref.row_merge_ref(blocks[order], xs[order], width)
    assert same(cnt, exp_cnt) and not same(row, exp_row)


@pytest.mark.parametrize("kind", ["plus_zero", "minus_zero"])
def test_a_reference_that_counts_zero_blocks_fails_the_equality(kind):
    blocks, xs, width = ROW_CASES[f"zero_{kind}_c4"]
    _, exp_cnt = _oracle_row(blocks, xs, width)
    counted = np.zeros_like(exp_cnt)
    for x in xs:  # every block counts, zero or not
        counted[:, int(x):int(x) + blocks.shape[2]] += np.uint8(1)
    assert same(ref.row_merge_ref(blocks, xs, width)[1], exp_cnt) and not same(counted, exp_cnt)


@pytest.mark.parametrize("name", ["count_wrap44", "count_wrap0"])
def test_a_reference_that_divides_by_the_unwrapped_count_fails_the_equality(name):
    case = next(c for c in FIN_CASES if c["name"] == name)
    probs, _ = ref.finalize_ref(*ref.finalize_args(case))
    unwrapped = (case["cnt_a"].astype(np.int64) + case["cnt_b"]).astype(np.float32)[..., None]
    assert not same((case["row_a"] + case["row_b"]) / unwrapped, probs)
    # and the statement is NumPy's own uint8 arithmetic, as `merge_vertical_chunkwise` runs it
    count = case["cnt_a"] + case["cnt_b"]
    assert same((case["row_a"] + case["row_b"]) / np.where(count == 0, 1, count).astype(np.float32)[..., None], probs)


def test_a_reference_that_scans_with_greater_than_fails_the_equality():
    for name in ("labels_alone", "labels_divided", "labels_two_rows"):
        case = next(c for c in FIN_CASES if c["name"] == name)
        probs, pred = ref.finalize_ref(*ref.finalize_args(case))
        assert not same(ref.gt_scan_argmax(probs), pred), name


def test_a_reference_that_drops_a_term_leaves_the_float64_bound():
    blocks, locs, shape = STITCH_CASES["two_by_four_deep_masked"]
    probs, _ = ref.stitch_ref(blocks, locs, shape)
    keep = np.ones(len(blocks), dtype=bool)
    keep[np.flatnonzero([bool(np.any(b)) for b in blocks])[7]] = False
    dropped, _ = ref.stitch_ref(blocks[keep], locs[keep], shape)
    assert ref.within_wide(probs, blocks, locs, shape) and not ref.within_wide(dropped, blocks, locs, shape)


# ------------------------------------------------------------------------------------------------ three patch rows over a canvas row
@pytest.mark.parametrize(("stride", "works"), [(5, False), (7, False), (8, True), (16, True)])
def test_statement_and_oracle_refuse_a_vertical_stride_below_half_the_output_height(stride, works):
    rng = np.random.default_rng(stride)
    locs = ref.grid_locs(48, 20, 16, 16, stride, 16)
    blocks = rng.random((len(locs), 16, 16, 2)).astype(np.float32)
    if works:
        assert same(ref.stitch_ref(blocks, locs, (48, 20))[0], osem.merge_wsi(blocks, locs, (48, 20)))
        return
    with pytest.raises(ValueError, match="all cover canvas row"):
        ref.stitch_ref(blocks, locs, (48, 20))
    with pytest.raises(ValueError, match="broadcast"):
        osem.merge_wsi(blocks, locs, (48, 20))


def test_engine_helper_refuses_the_same_configurations():
    """``check_patch_row_overlap`` (host arithmetic only): what both ``infer_wsi`` methods call once the coordinates are known."""
    from types import SimpleNamespace

    from tiatoolbox_amd.models.engine.semantic_segmentor import check_patch_row_overlap

    for stride, works in ((5, False), (7, False), (8, True), (16, True), (20, True)):
        cfg = SimpleNamespace(patch_output_shape=[16, 16], stride_shape=[stride, 5])
        locs = ref.grid_locs(48, 20, 16, 16, stride, 5)
        if works:
            check_patch_row_overlap(locs, cfg)
            continue
        with pytest.raises(ValueError, match=r"`patch_output_shape` \[16, 16\] with `stride_shape` \[%d, 5\]" % stride):
            check_patch_row_overlap(locs, cfg)
    # one or two patch rows can never stack three deep, whatever the stride
    check_patch_row_overlap(ref.grid_locs(6, 20, 16, 16, 5, 5), SimpleNamespace(patch_output_shape=[16, 16], stride_shape=[5, 5]))

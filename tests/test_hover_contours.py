"""Host side of the contour-kernel tests: the scipy statement of outer borders has hand-computed answers and agrees with ``cvref``; the
case arrays of ``_contour_ref`` really hold the edges they are named after (and the sizes they are built around still stand in
``contours.hip``); the comparison helper rejects subtly wrong references.  ``test_hover_contours_gpu.py`` runs the kernels."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
from scipy import ndimage

from oracle import cvref

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _contour_ref as ref  # noqa: E402


def _pixel_set(shape, pts) -> np.ndarray:
    a = np.zeros(shape, bool)
    for x, y in pts:
        a[y, x] = True
    return a


# -------------------------------------------------------------------------------------------- the scipy statement, by hand
def test_scipy_statement_known_answers():
    m = np.zeros((30, 30), np.uint8)
    m[10:21, 10:21] = 1
    edge = np.zeros((30, 30), bool)
    edge[10, 10:21] = edge[20, 10:21] = edge[10:21, 10] = edge[10:21, 20] = True
    for holed in (False, True):  # a hole changes neither the chosen component, nor its start, nor its outer border
        if holed:
            m[13:17, 14:18] = 0
            m[15, 15] = 1      # and an island in the hole does not touch the outside background: never chosen
        comp, start = ref.chosen_component(m)
        assert start == (10, 10) and comp[10, 10] and comp[15, 15] == (not holed) and comp.sum() == 121 - (16 if holed else 0)  # noqa: PLR2004
        assert np.array_equal(ref.outer_border_set(comp), edge) and edge.sum() == 40  # noqa: PLR2004
        chain = ref.expand(cvref.first_contour(m))
        assert len(chain) == 40 and np.array_equal(_pixel_set(m.shape, chain), edge)  # noqa: PLR2004
    d = np.zeros((7, 7), np.uint8)
    for r in range(7):
        d[r, abs(r - 3):7 - abs(r - 3)] = 1
    comp, start = ref.chosen_component(d)
    assert start == (3, 0)
    assert ref.expand([[3, 0], [0, 3], [3, 6], [6, 3]]) == [(3, 0), (2, 1), (1, 2), (0, 3), (1, 4), (2, 5), (3, 6), (4, 5), (5, 4),
                                                            (6, 3), (5, 2), (4, 1)]
    assert np.array_equal(ref.outer_border_set(comp), _pixel_set(d.shape, ref.expand([[3, 0], [0, 3], [3, 6], [6, 3]])))
    line = np.zeros((3, 8), np.uint8)
    line[1, 1:7] = 1
    comp, start = ref.chosen_component(line)
    assert start == (1, 1) and np.array_equal(ref.outer_border_set(comp), line.astype(bool))
    there_and_back = [(x, 1) for x in (1, 2, 3, 4, 5, 6, 5, 4, 3, 2)]
    assert ref.expand([[1, 1], [6, 1]]) == there_and_back  # a line's chain passes its inner pixels twice
    two = np.zeros((6, 12), np.uint8)
    two[1:3, 1:4] = 1
    two[3:5, 7:10] = 1
    comp, start = ref.chosen_component(two)
    assert start == (7, 3) and comp.sum() == 6 and comp[3:5, 7:10].all()  # noqa: PLR2004  -- the component found last
    thin = ref.binary_planes()["thin_ring"]
    comp, start = ref.chosen_component(thin)
    assert start == (2, 2) and np.array_equal(ref.outer_border_set(comp), thin.astype(bool))  # every pixel of a thin ring
    assert ref.expand([[2, 2], [2, 7], [9, 7], [9, 2]])[:6] == [(2, y) for y in range(2, 8)]
    eye = np.eye(4, dtype=np.uint8)
    comp, start = ref.chosen_component(eye)
    assert start == (0, 0) and comp.sum() == 4 and np.array_equal(ref.outer_border_set(comp), eye.astype(bool))  # noqa: PLR2004
    assert ref.chosen_component(eye, connectivity=4)[1] == (3, 3)  # 4-connected: four components, the last one starts at (3, 3)
    assert ref.expand([[0, 0], [3, 3]]) == [(0, 0), (1, 1), (2, 2), (3, 3), (2, 2), (1, 1)]
    assert ref.expand([[5, 6]]) == [(5, 6)]
    try:
        ref.expand([[0, 0], [2, 1]])
    except ValueError:
        pass
    else:
        raise AssertionError("a knight's move is on none of the 8 directions")
    assert ref.is_rotation([1, 2, 3], [3, 1, 2]) and not ref.is_rotation([1, 2, 3], [3, 2, 1]) and not ref.is_rotation([1], [1, 1])


def test_scipy_statement_agrees_with_cvref_on_random_masks():
    """300 random masks of up to 13 x 13 pixels at densities 0.3 to 0.9, every outer border: the expanded SIMPLE polygon is a
    rotation of the NONE chain, the chain's pixel set is the scipy outer-border set of its component, the chain starts at the
    component's raster-first pixel, and ``first_contour`` is the border of the scipy-chosen component."""
    rng = np.random.default_rng(0)
    total = 0
    for _ in range(300):
        h, w = rng.integers(1, 14, 2)
        m = rng.random((h, w)) < rng.choice([0.3, 0.5, 0.7, 0.9])
        if not m.any():
            continue
        lab, k = ndimage.label(m, structure=ref.EIGHT)
        found = ref.outer_borders(m)
        assert len(found) == k
        for b in found:
            total += 1
            chain = [tuple(p) for p in b["chain"].tolist()]
            assert ref.is_rotation(ref.expand(b["simple"]), chain), (m.astype(int), b)
            x0, y0 = chain[0]
            comp = lab == lab[y0, x0]
            assert np.flatnonzero(comp)[0] == y0 * w + x0
            assert np.array_equal(_pixel_set(m.shape, chain), ref.outer_border_set(comp)), (m.astype(int), b)
        comp, start = ref.chosen_component(m)
        poly, first = ref.choose_first_contour(found)
        assert start == tuple(first.tolist()) and np.array_equal(poly, cvref.first_contour(m.astype(np.uint8))), m.astype(int)
    assert total > 600  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------ constants read from the source
def test_sizes_the_cases_rest_on_still_stand_in_the_source():
    c = ref.source_constants()
    assert c == {"offset_threads": 1024, "first_pixel_blocks": 4096, "first_pixel_threads": 256, "CT": 64}
    assert ref.first_pixel_cap() == 1_048_576
    assert [ref.offsets_chunk(e) for e in (1, 1023, 1024, 1025, 2048, 2049, 3026)] == [1, 1, 1, 2, 2, 3, 3]


# ------------------------------------------------------------------------------------------------- what the label-map cases hold
def _census(case: str) -> dict:
    lab, max_inst = ref.label_case(case)
    borders = ref.borders_of(case)
    present = {(p, int(i)) for p in range(lab.shape[0]) for i in np.unique(lab[p]) if i > 0}
    assert present == set(borders), case  # no id is left out of the GPU comparison: it walks exactly these keys
    meta, points = ref.expected_contours(borders, lab.shape[0], max_inst)
    assert {(p, i) for p, i in zip(*np.nonzero(meta[..., 2]))} == {k for k in present if k[1] <= max_inst}
    assert not meta[:, 0].any() or (meta[:, 0, :3] == 0).all()
    counts = meta[..., 2]
    out = {"entries": lab.shape[0] * (max_inst + 1), "present": len(present), "absent": int((counts[:, 1:] == 0).sum()),
           "v1": int((counts == 1).sum()), "v2": int((counts == 2).sum()), "v3": int((counts >= 3).sum()),  # noqa: PLR2004
           "total": len(points), "multi": 0, "holes": 0, "nested": 0}
    for _, found in borders.values():
        out["multi"] += len(found) > 1
        out["nested"] += any(not b["top"] for b in found)
    for _, _, _, crop in ref.instance_crops(lab):
        out["holes"] += bool((ndimage.binary_fill_holes(crop) != crop).any())
    return out


def test_chunk_cases_straddle_the_offset_kernels_threads():
    threads = ref.source_constants()["offset_threads"]
    seen = {}
    for name, _, _, _ in ref.CHUNK_CASES:
        lab, max_inst = ref.chunk_case(name)
        assert not lab.flags.writeable and lab.dtype == np.int32 and lab.max() <= max_inst
        c = _census(name)
        seen[name] = (c["entries"], ref.offsets_chunk(c["entries"]))
        assert c["absent"] > 0 and c["multi"] > 0 and c["holes"] > 0 and c["v3"] > 0, (name, c)
        print(name, c)
    assert seen == {"1023-entries": (threads - 1, 1), "1024-entries": (threads, 1), "1025-entries": (threads + 1, 2),
                    "3x701-entries": (2103, 3), "3026-entries": (3026, 3)}
    assert {v[1] for v in seen.values()} == {1, 2, 3}  # chunk sizes 1, 2 and 3 of the prefix sum
    owning = -(-2103 // 3)  # threads of the n = 3 case that own an entry
    assert owning == 701 and threads - owning > 0.3 * threads  # noqa: PLR2004  -- the last third owns none
    lab, _ = ref.chunk_case("3x701-entries")
    assert lab.shape[0] == 3 and len({int((np.unique(p) > 0).sum()) for p in lab}) == 3  # noqa: PLR2004  -- planes differ in label count
    assert ref.chunk_case("3026-entries")[0].shape == (1, 550, 550)


def test_mixed_batch_holds_the_adversarial_instances():
    lab, max_inst = ref.label_case("mixed")
    assert not lab.flags.writeable and lab.shape == (4, 90, 100)
    per_plane = [int((np.unique(p) > 0).sum()) for p in lab]
    assert per_plane[1] == 0 and len(set(per_plane)) == 4 and max_inst > lab.max()  # noqa: PLR2004  -- planes differ; trailing ids absent
    c = _census("mixed")
    print("mixed", c, per_plane)
    assert c["v1"] >= 4 and c["v2"] >= 5 and c["v3"] > 50 and c["multi"] > 5 and c["holes"] > 5 and c["nested"] >= 3  # noqa: PLR2004
    h, w = lab.shape[1:]
    for kind, plane in (("rects", lab[0]), ("pixels", lab[3])):
        assert plane[0].any() and plane[-1].any() and plane[:, 0].any() and plane[:, -1].any()  # pixels on all four frame edges
        assert all(plane[y, x] for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))) or kind == "pixels"
    rects, where = ref.adversarial_plane("rects")
    masks = {name: np.isin(rects, ids) for name, (ids, _) in where.items()}
    assert masks["corner_tl"][0, 0] and masks["corner_tr"][0, -1] and masks["corner_bl"][-1, 0] and masks["corner_br"][-1, -1]
    assert masks["edge_top"][0].any() and masks["edge_bottom"][-1].any() and masks["edge_left"][:, 0].any() and masks["edge_right"][:, -1].any()
    assert all(ndimage.label(masks[k], structure=ref.EIGHT)[1] == 1 for k in ("hline", "vline", "diag", "antidiag", "pixel", "spiral"))
    assert [int(masks[k].sum()) for k in ("hline", "vline", "diag", "antidiag", "pixel")] == [12, 12, 10, 10, 1]
    assert ndimage.label(masks["diag"])[1] == 10 and ndimage.label(masks["antidiag"])[1] == 10  # noqa: PLR2004  -- diagonal links only
    sp = masks["spiral"]
    assert ndimage.label(sp)[1] == 1 and ndimage.label(~np.pad(sp, 1))[1] == 1  # one 4-connected stroke, no hole
    assert ndimage.convolve(sp.astype(int), ref.FOUR.astype(int), mode="constant")[sp].max() == 3  # noqa: PLR2004  -- itself + 2: one pixel wide
    assert sp.sum() == 14 * 3 + 2 * (12 + 10 + 8 + 6 + 4 + 2) + 1
    r4 = masks["rings4"]
    assert ndimage.label(r4, structure=ref.EIGHT)[1] == 2 and ndimage.label(~np.pad(r4, 1))[1] == 3  # noqa: PLR2004  -- nested: 2 rings, 2 holes
    pix, where = ref.adversarial_plane("pixels")
    masks = {name: np.isin(pix, ids) for name, (ids, _) in where.items()}
    assert masks["pixel_at_origin"][0, 0] and masks["pixel_at_origin"].sum() == 1
    assert masks["pixel_at_far_corner"][-1, -1] and masks["pixel_at_far_corner"].sum() == 1
    s = masks["whole_plane_bbox"]
    assert s[0].any() and s[-1].any() and s[:, 0].any() and s[:, -1].any() and ndimage.label(s)[1] == 1
    assert ndimage.label(~np.pad(s, 1))[1] == 1  # its two pockets open onto the frame: no hole
    r1 = masks["rings1"]
    assert ndimage.label(r1, structure=ref.EIGHT)[1] == 3 and ndimage.label(~np.pad(r1, 1))[1] == 3  # noqa: PLR2004  -- ring, ring, centre pixel
    ck = masks["checker"]
    assert ndimage.label(ck, structure=ref.EIGHT)[1] == 1 and ndimage.label(ck)[1] == ck.sum() == 25  # noqa: PLR2004
    isl = masks["island_in_own_hole"]
    assert ndimage.label(isl, structure=ref.EIGHT)[1] == 2 and ndimage.label(~np.pad(isl, 1))[1] == 2  # noqa: PLR2004
    ids_ab = where["ring_a_filled_by_b"][0]
    ring_a, fill_b = pix == ids_ab[0], pix == ids_ab[1]
    assert np.array_equal(ndimage.binary_fill_holes(ring_a), ring_a | fill_b) and fill_b.sum() == 25  # noqa: PLR2004
    borders = ref.borders_of("mixed")
    (rid,), _ = where["ring_then_component_on_its_rows"]
    _, found = borders[(3, rid)]
    assert [b["top"] for b in found] == [True, True]
    assert found[1]["chain"][0].tolist() == [7, 1] and found[0]["chain"][0].tolist() == [0, 0]  # right of the ring, on its rows
    (lid,), _ = where["last_found_starts_further_left"]
    _, found = borders[(3, lid)]
    assert [b["top"] for b in found] == [True, True] and found[1]["chain"][0, 0] < found[0]["chain"][0, 0]
    (iid,), _ = where["island_in_own_hole"]
    assert [b["top"] for b in borders[(3, iid)][1]] == [True, False]
    for lab_t in ref.tiny_label_batches():
        assert not lab_t.flags.writeable
    assert [t.shape for t in ref.tiny_label_batches()] == [(1, 1, 1), (2, 1, 9), (2, 9, 1)]
    for case in ("tiny0", "tiny1", "tiny2"):
        _census(case)


# --------------------------------------------------------------------------------------------------- what the binary cases hold
def _components(m: np.ndarray) -> tuple[int, int]:
    """(8-connected foreground components, 4-connected background components that do not reach the frame) = (outer, hole borders)."""
    bg, kb = ndimage.label(np.pad(m == 0, 1, constant_values=True))
    return ndimage.label(m != 0, structure=ref.EIGHT)[1], kb - 1


def test_binary_cases_hold_the_named_edges():
    cap = ref.first_pixel_cap()
    big = ref.big_plane()
    h, w = big.shape
    assert big.shape == (1025, 1024) and big.size > cap and (h - 1) * w == cap and not big.flags.writeable
    assert big.mean() < 0.002  # noqa: PLR2004  -- mostly empty
    fg, kf = ndimage.label(big, structure=ref.EIGHT)
    first = ndimage.minimum(np.arange(big.size).reshape(big.shape), fg, np.arange(1, kf + 1))
    assert kf == 9 and (first >= cap).sum() == 3 and first.min() == 0  # noqa: PLR2004  -- three components start in the second trip
    assert big[-1, -1] and big[0, 0]
    bg, kb = ndimage.label(big == 0)
    pocket = bg == bg[h - 2, 23]
    on_frame = pocket.copy()
    on_frame[1:-1, 1:-1] = False
    assert pocket.sum() == 9 and pocket[h - 1, 22:25].all() and np.flatnonzero(on_frame).min() >= cap  # noqa: PLR2004
    assert _components(big) == (9, 2) and bg[h - 3, 5] != bg[0, 10]  # the true hole of rows 1020-1023 and the one in the middle
    for simple in (False, True):
        assert len(ref.expected_borders("big", simple)) == 11  # noqa: PLR2004
    six = ref.six_planes()
    counts = [_components(p) for p in six]
    print("six planes (outer, hole) borders:", counts)
    assert counts[0] == (0, 0) and counts[1] == (1, 0) and counts[5] == (1, 0) and not six[0].any() and six[1].all() and six[5].sum() == 1
    assert counts[3] == (10, 10)  # ten rings, nine gaps between them and the centre pixel
    assert counts[4] == (4, 2)  # pockets: the corner hole and the diagonally closed pocket; the two open pockets have none
    nb = sum(a + b for a, b in counts)
    ct = ref.source_constants()["CT"]
    assert counts[2][0] + counts[2][1] >= 200 and nb % ct != 0 and len({a for a, _ in counts}) >= 5  # noqa: PLR2004
    assert all(len(ref.expected_borders(f"six{i}", True)) == a + b for i, (a, b) in enumerate(counts))
    pockets = ref.pockets_plane()
    bg, _ = ndimage.label(pockets == 0)
    assert bg[1, 1] != bg[0, 0] and pockets[0, 1] and pockets[1, 0]          # the corner hole meets the frame pixel by a diagonal
    assert bg[12, 12] == bg[5, 5] and bg[12, 32] != bg[5, 5] and bg[32, 48] == bg[5, 5]
    planes = ref.binary_planes()
    assert planes["1xW"].shape == (1, 11) and planes["Hx1"].shape == (11, 1) and all(not p.flags.writeable for p in planes.values())
    for name, m in planes.items():
        for simple in (False, True):
            assert len(ref.expected_borders(name, simple)) == sum(_components(m)), name


# -------------------------------------------------------------------------------------- the comparison can tell right from wrong
def test_the_comparison_rejects_subtly_wrong_references():
    lab, max_inst = ref.label_case("mixed")
    n = lab.shape[0]
    borders = ref.borders_of("mixed")
    meta, points = ref.expected_contours(borders, n, max_inst)
    present = sorted(borders)
    assert ref.compare_contours(meta.copy(), points.copy(), meta, points, present) == []
    assert ref.scipy_mismatches(lab, meta, points) == []

    def rejected(m, p, what):
        bad = ref.compare_contours(m, p, meta, points, present)
        assert bad, what
        return bad

    inclusive = meta.copy()
    inclusive[..., 3] += inclusive[..., 2]
    assert all(b.startswith("offset") or b.startswith("polygon") for b in rejected(inclusive, points, "inclusive offsets"))
    for what, choose in (
            ("the first top-level component", lambda f: ([b for b in f if b["top"]][0]["simple"], [b for b in f if b["top"]][0]["chain"][0])),
            ("a component inside a hole accepted as top-level", lambda f: (f[-1]["simple"], f[-1]["chain"][0])),
            ("points in reverse order", lambda f: (ref.choose_first_contour(f)[0][::-1], ref.choose_first_contour(f)[1])),
            ("CHAIN_APPROX_NONE", lambda f: ([b for b in f if b["top"]][-1]["chain"], ref.choose_first_contour(f)[1]))):
        m, p = ref.expected_contours(borders, n, max_inst, choose)
        bad = rejected(m, p, what)
        assert what == "points in reverse order" or ref.scipy_mismatches(lab, m, p) or what == "CHAIN_APPROX_NONE", what
        print(f"{what}: {len(bad)} differences")
    four = meta.copy()
    for p, i, tl, crop in ref.instance_crops(lab):
        four[p, i, :2] = np.array(ref.chosen_component(crop, connectivity=4)[1]) + tl
    bad = rejected(four, points, "the start pixel of a 4-connected component")
    assert all(b.startswith("start") for b in bad) and ref.scipy_mismatches(lab, four, points)
    assert rejected(meta.astype(np.int64), points, "dtype") and rejected(meta, points[:-1], "total") and rejected(meta[:, :-1], points, "shape")
    one_off = points.copy()
    one_off[len(points) // 2, 0] += 1
    assert len(rejected(meta, one_off, "one coordinate")) == 1
    exp = [np.array([[1, 2], [3, 4]], np.int32), np.array([[5, 6]], np.int32)]
    assert ref.compare_borders([e.copy() for e in exp], exp) == []
    assert ref.compare_borders(exp[::-1], exp) and ref.compare_borders(exp[:1], exp) and ref.compare_borders([e.astype(np.int64) for e in exp], exp)

"""``peak_local_max``: the NumPy statement (``tiatoolbox_amd/utils/_peaks.py``) against an independent brute-force definition,
hand-computed answers and -- where installed -- skimage; the Python surface's refusals and its CPU path; the host walk over
contested candidates (``tia_peak_resolve_host``) against the statement.  No GPU."""

from __future__ import annotations

import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _peaks_ref as ref  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent

FIVE = np.array([[0, 0, 0, 0, 0],
                 [0, 5, 0, 0, 0],
                 [0, 0, 0, 3, 0],
                 [0, 0, 0, 0, 0],
                 [4, 0, 0, 0, 0]], dtype=np.float32)


def _statement():
    from tiatoolbox_amd.utils import _peaks

    return _peaks


def _pairs(*points) -> np.ndarray:
    return np.asarray(points, dtype=np.int64).reshape(-1, 2)


def test_statement_equals_the_brute_force_definition_on_small_planes():
    st = _statement()
    seen_kept = seen_rejected = planes = 0
    for img, kw in ref.small_planes(200):
        got, exp = st.peak_local_max_ref(img, **kw), ref.brute_peaks(img, **kw)
        assert ref.same_peaks(got, exp), (img, kw, got, exp)
        cand = st.candidates_ref(img, kw["min_distance"], kw.get("threshold_abs"), kw.get("threshold_rel"), kw["exclude_border"])
        contested = st.contested_ref(cand, kw["min_distance"], img.shape)
        # an uncontested candidate is always a peak (what the device path rests on)
        if "num_peaks" not in kw:
            assert {tuple(c) for c in cand[~contested]} <= {tuple(c) for c in got}
            seen_rejected += len(cand) - len(got)
        seen_kept += len(got)
        planes += 1
    assert planes == 200 and seen_kept > 300 and seen_rejected > 100  # noqa: PLR2004  (the spacing walk did reject)


def test_hand_computed_answers():
    peaks = _statement().peak_local_max_ref
    # 3 x 3 windows: all three spikes; zeros equal their window's maximum elsewhere but are not > the minimum
    assert ref.same_peaks(peaks(FIVE, 1), _pairs((1, 1), (4, 0), (2, 3)))
    # 5 x 5 windows: the 3 has the 5 in its window
    assert ref.same_peaks(peaks(FIVE, 2), _pairs((1, 1), (4, 0)))
    assert ref.same_peaks(peaks(FIVE, 1, threshold_abs=3.0), _pairs((1, 1), (4, 0)))  # strict
    assert ref.same_peaks(peaks(FIVE, 1, threshold_rel=0.8), _pairs((1, 1)))  # 0.8 * 5 = 4: strict
    assert ref.same_peaks(peaks(FIVE, 1, num_peaks=2), _pairs((1, 1), (4, 0)))
    assert ref.same_peaks(peaks(FIVE, 1, num_peaks=0), _pairs())
    # a plateau run of seven 1s: every one is a candidate, the walk keeps every min_distance-th in raster order
    run = np.zeros((3, 9), dtype=np.float32)
    run[1, 1:8] = 1.0
    assert ref.same_peaks(peaks(run, 1), _pairs(*[(1, x) for x in range(1, 8)]))
    assert ref.same_peaks(peaks(run, 2), _pairs((1, 1), (1, 3), (1, 5), (1, 7)))
    assert ref.same_peaks(peaks(run, 3), _pairs((1, 1), (1, 4), (1, 7)))
    # exclude_border: after the window test -- the 4 in the last row goes, the 3 does not come back at distance 2
    assert ref.same_peaks(peaks(FIVE, 1, exclude_border=1), _pairs((1, 1), (2, 3)))
    assert ref.same_peaks(peaks(FIVE, 2, exclude_border=1), _pairs((1, 1)))
    assert ref.same_peaks(peaks(FIVE, 2, exclude_border=True), _pairs())  # True = min_distance = 2: only (2, 2) is left
    assert ref.same_peaks(peaks(FIVE, 1, exclude_border=0), peaks(FIVE, 1, exclude_border=False))
    # a constant plane has no peaks; a single pixel is `image > t`
    assert ref.same_peaks(peaks(np.ones((4, 4), np.float32), 1, threshold_abs=0.0), _pairs())
    assert ref.same_peaks(peaks(np.ones((1, 1), np.float32), 1), _pairs())
    assert ref.same_peaks(peaks(np.ones((1, 1), np.float32), 1, threshold_abs=0.5), _pairs((0, 0)))


def test_statement_equals_skimage():
    feature = pytest.importorskip("skimage.feature")
    st = _statement()
    for img, kw in ref.small_planes(200):
        exp = feature.peak_local_max(img, p_norm=np.inf, **kw)
        assert ref.same_peaks(st.peak_local_max_ref(img, **kw), np.asarray(exp, dtype=np.int64).reshape(-1, 2)), (img, kw)


def test_comparison_helper_rejects_wrong_rules():
    exp = ref.brute_peaks(FIVE, 1)
    assert ref.same_peaks(exp, exp.copy())
    assert not ref.same_peaks(exp[::-1], exp)            # a wrong order
    assert not ref.same_peaks(exp[[0, 2, 1]], exp)
    assert not ref.same_peaks(exp[:2], exp) and not ref.same_peaks(exp.astype(np.int32), exp)
    # `<=` for `<` in the spacing rule: candidates exactly min_distance apart
    run = np.zeros((3, 9), dtype=np.float32)
    run[1, 1:8] = 1.0
    assert not ref.same_peaks(ref.brute_peaks(run, 2, spacing_le=True), ref.brute_peaks(run, 2))
    assert not ref.same_peaks(ref.brute_peaks(run, 1, spacing_le=True), ref.brute_peaks(run, 1))
    # `>=` for `>` in the threshold: a threshold equal to a peak's value
    assert not ref.same_peaks(ref.brute_peaks(FIVE, 1, threshold_abs=3.0, threshold_ge=True), ref.brute_peaks(FIVE, 1, threshold_abs=3.0))
    # ... and the statement sides with the right rule in each
    peaks = _statement().peak_local_max_ref
    assert ref.same_peaks(peaks(run, 2), ref.brute_peaks(run, 2))
    assert ref.same_peaks(peaks(FIVE, 1, threshold_abs=3.0), ref.brute_peaks(FIVE, 1, threshold_abs=3.0))


def test_quantised_map_is_mostly_contested():
    """The fact the device tests lean on: on the smooth 257 x 300 map of 41 levels more than half of the candidates at
    ``min_distance=3`` have another candidate at Chebyshev distance < 3 (and of equal value), none at ``min_distance=1``; on a random
    map none."""
    st = _statement()
    img = ref.smooth_quantised_plane(257, 300, 15)
    assert len(np.unique(img)) == 41  # noqa: PLR2004
    cand = st.candidates_ref(img, 3)
    contested = st.contested_ref(cand, 3, img.shape)
    assert len(cand) > 2000 and contested.sum() > len(cand) / 2  # noqa: PLR2004
    assert not st.contested_ref(st.candidates_ref(img, 1), 1, img.shape).any()
    rnd = ref.random_plane(257, 300, 16)
    for d in (1, 3, 7, 16):
        assert not st.contested_ref(st.candidates_ref(rnd, d), d, rnd.shape).any()
    # contested candidates within reach of each other carry equal values
    ys, xs = cand[contested][:, 0], cand[contested][:, 1]
    for i in range(0, len(ys), 97):
        near = (np.abs(ys - ys[i]) < 3) & (np.abs(xs - xs[i]) < 3)  # noqa: PLR2004
        assert near.sum() >= 2 and np.all(img[ys[near], xs[near]] == img[ys[i], xs[i]])  # noqa: PLR2004


def test_header_declares_the_peak_entries():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tiatoolbox_amd.h").read_text(), flags=re.S)
    names = set(re.findall(r"^\s*(?:int|void|size_t)\s+(tia_\w+)\s*\(", text, flags=re.M))
    assert {"tia_peak_chunks", "tia_peak_scan_f32", "tia_peak_write_f32", "tia_peak_resolve_host"} <= names
    from tiatoolbox_amd import _lib

    assert {"tia_peak_chunks", "tia_peak_scan_f32", "tia_peak_write_f32", "tia_peak_resolve_host"} <= set(_lib._SIGNATURES)  # noqa: SLF001
    assert "`tia_peak_scan_f32`" in (ROOT / "INTEGRATION.md").read_text()


def test_module_imports_and_refuses_before_any_launch():
    import torch

    from tiatoolbox_amd import utils
    from tiatoolbox_amd.utils import peaks

    assert utils.peaks is peaks and callable(peaks.peak_local_max)
    img = torch.from_numpy(FIVE)
    for bad in (img.double(), img.to(torch.float16), img.to(torch.int32), img[0], img[None, None], FIVE):
        with pytest.raises(ValueError, match="image"):
            peaks.peak_local_max(bad)
    for d in (0, -1, 65, 1.5, True):
        with pytest.raises(ValueError, match="min_distance"):
            peaks.peak_local_max(img, min_distance=d)
    for b in (-1, 1.5, "yes"):
        with pytest.raises(ValueError, match="exclude_border"):
            peaks.peak_local_max(img, exclude_border=b)
    for k in (-1, 2.5):
        with pytest.raises(ValueError, match="num_peaks"):
            peaks.peak_local_max(img, num_peaks=k)


def test_cpu_tensors_run_the_statement():
    import torch

    from tiatoolbox_amd.utils import peaks

    st = _statement()
    got = peaks.peak_local_max(torch.from_numpy(FIVE), min_distance=1)
    assert got.dtype == torch.int64 and ref.same_peaks(got.numpy(), _pairs((1, 1), (4, 0), (2, 3)))
    batch = np.stack([ref.quantised_plane(20, 30, 1, 5), ref.random_plane(20, 30, 2), np.zeros((20, 30), np.float32)])
    out = peaks.peak_local_max(torch.from_numpy(batch), min_distance=2, exclude_border=True, num_peaks=7)
    assert isinstance(out, list) and len(out) == 3  # noqa: PLR2004
    for plane, got in zip(batch, out):
        assert ref.same_peaks(got.numpy(), st.peak_local_max_ref(plane, 2, exclude_border=True, num_peaks=7))
    coords, values, counts = peaks.peak_local_max_planes(torch.from_numpy(batch), min_distance=2)
    assert counts == [len(st.peak_local_max_ref(p, 2)) for p in batch] and counts[2] == 0
    first = coords[:counts[0]].numpy()
    assert np.array_equal(values[:counts[0]].numpy(), batch[0][first[:, 0], first[:, 1]])
    empty = peaks.peak_local_max(torch.zeros((0, 5), dtype=torch.float32))
    assert tuple(empty.shape) == (0, 2) and empty.dtype == torch.int64


def _resolve(lib, yx: np.ndarray, w: int, d: int):
    yx = np.ascontiguousarray(yx, dtype=np.int32)
    accept = np.full(len(yx), 7, dtype=np.uint8)
    rc = lib.tia_peak_resolve_host(ctypes.c_void_p(yx.ctypes.data), len(yx), w, d, ctypes.c_void_p(accept.ctypes.data))
    return rc, accept


def test_host_walk_over_the_contested_candidates_equals_the_statement():
    """Uncontested candidates plus what ``tia_peak_resolve_host`` accepts among the contested ones, put into the statement's order,
    is the statement's result: on the quantised map, the row of 300, saturated discs and a checkerboard."""
    from tiatoolbox_amd import _lib, build

    if not build.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load()
    st = _statement()
    row = np.zeros((5, 304), dtype=np.float32)
    row[2, 2:302] = 1.0
    yy, xx = np.mgrid[:34, :37]
    planes = [(ref.smooth_quantised_plane(257, 300, 15), 3), (ref.quantised_plane(257, 300, 15), 3), (row, 3), (ref.discs_plane(90, 120, 12), 4), (ref.discs_plane(90, 120, 12), 64),
              (((yy + xx) % 2).astype(np.float32), 2), (ref.quantised_plane(60, 70, 3, 3), 7)]
    for img, d in planes:
        cand = st.candidates_ref(img, d)
        contested = st.contested_ref(cand, d, img.shape)
        assert contested.any()
        rc, accept = _resolve(lib, cand[contested], img.shape[1], d)
        assert rc == 0 and set(accept.tolist()) <= {0, 1}
        keep = np.ones(len(cand), dtype=bool)
        keep[contested] = accept.astype(bool)
        kept = cand[keep]
        order = np.argsort(-img[kept[:, 0], kept[:, 1]], kind="stable")
        assert ref.same_peaks(kept[order], st.peak_local_max_ref(img, d)), d
    # refusals: nothing is read through a null pointer, candidates out of raster order or outside the plane are an error
    einval = -1
    assert lib.tia_peak_resolve_host(None, 0, 5, 2, None) == 0
    assert lib.tia_peak_resolve_host(None, 3, 5, 2, None) == einval
    for bad in ([[1, 1], [0, 2]], [[0, 2], [0, 2]], [[0, 5]], [[-1, 0]], [[0, -1]]):
        assert _resolve(lib, np.array(bad), 5, 2)[0] == einval, bad
    assert _resolve(lib, np.array([[0, 0]]), 0, 2)[0] == einval and _resolve(lib, np.array([[0, 0]]), 5, 0)[0] == einval


def test_tile_side_is_readable_from_the_source():
    text = (ROOT / "tiatoolbox_amd" / "csrc" / "peaks.hip").read_text()
    found = re.findall(r"constexpr int PEAK_TILE = (\d+);", text)
    assert len(found) == 1 and int(found[0]) >= 8  # noqa: PLR2004
    assert len(re.findall(r"constexpr int PEAK_MAX_DISTANCE = 64;", text)) == 1
    assert _statement().MAX_MIN_DISTANCE == 64  # noqa: PLR2004

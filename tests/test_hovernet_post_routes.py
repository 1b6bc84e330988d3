"""CPU side of the HoVer-Net post-processing route tests: the route table of ``_hover_routes_ref`` against the constants in the
sources, the Sobel sizes and object sizes of the scales used, and the oracle on the planes too thin for ``synth_maps``."""

from __future__ import annotations

import re
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import hovernet as oh

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _hover_routes_ref as ref  # noqa: E402

CSRC = Path(__file__).resolve().parent.parent / "tiatoolbox_amd" / "csrc"


def _one(pattern: str, text: str) -> re.Match:
    found = list(re.finditer(pattern, text))
    assert len(found) == 1, (pattern, len(found))
    return found[0]


def test_route_table_follows_the_thresholds_in_the_sources():
    common = (CSRC / "common.hpp").read_text()
    hover = (CSRC / "hover_post.hip").read_text()
    assert int(_one(r"constexpr long kCclTileMaxPixels = (\d+);", common).group(1)) == ref.CCL_TILE_MAX_PIXELS
    assert int(_one(r"constexpr long kMarkerTileMaxPixels = (\d+);", common).group(1)) == ref.MARKER_TILE_MAX_PIXELS
    m = _one(r"const long band_rows_max = \((\d+)L \* (\d+)\) / \(w \* (\d+)\) - \(ksize - 1\);", hover)
    assert int(m.group(1)) * int(m.group(2)) == ref.SOBEL_LDS_BYTES and int(m.group(3)) == ref.SOBEL_LDS_BYTES_PER_PIXEL
    # the conditions themselves, as route() restates them
    _one(r"const bool tile = ccl_tile_enabled\(\) && hw <= kCclTileMaxPixels;", hover)
    _one(r"const bool fused = tile && hw <= kMarkerTileMaxPixels && band_rows_max >= (8);", hover)
    _one(r"bool tile_sobel = tile && band_rows_max >= (8);", hover)
    _one(r"\} else if \(tile && hw <= kMarkerTileMaxPixels\) \{", hover)
    assert ref.MIN_BAND_ROWS == 8  # noqa: PLR2004
    # the launch picks <21>, <11> or the run-time form
    _one(r"variants\[ksize == 21 \? 0 : \(ksize == 11 \? 1 : 2\)\]", hover)
    assert ref.TEMPLATED_KSIZES == (21, 11)

    for (want, h, w, scale) in ref.ROUTE_CASES:
        assert ref.route(h, w, ref.ksize_of(scale)) == want, (want, h, w, scale)


def test_route_table_covers_every_route_size_and_threshold():
    for scale, ksize in ref.KSIZE_OF_SCALE.items():
        assert ref.ksize_of(scale) == ksize and ksize % 2 == 1 and 5 <= ksize <= 31, (scale, ref.ksize_of(scale))  # noqa: PLR2004
    assert [ref.obj_size_of(s) for s in (1, 0.5, 0.2, 0.3, 0.7, 1.5)] == [10, 3, 1, 1, 5, 23]
    seen = {(r, ref.ksize_of(s)) for (r, _, _, s) in ref.ROUTE_CASES}
    for r in "ABCD":
        assert (r, 21) in seen and (r, 11) in seen, r
    run_time = {(r, k) for (r, k) in seen if k not in ref.TEMPLATED_KSIZES}
    assert {r for r, _ in run_time} >= {"A", "C"}                 # KS = 0 on the tile kernel, with and without its Gaussian
    assert {r for r, _ in run_time} & {"B", "D"}                  # and a run-time size on the stand-alone kernels
    assert any(r == "E" for r, _ in seen)
    shapes = {(h, w, ref.ksize_of(s)) for (_, h, w, s) in ref.ROUTE_CASES}
    # both sides of every threshold, worked out from the formula
    for (h, w, k) in ((72, 438, 21), (46, 682, 11), (96, 323, 31)):
        assert (h, w, k) in shapes and (h, w + 1, k) in shapes
        assert ref.band_rows_max(w, k) == 8 and ref.band_rows_max(w + 1, k) == 7  # noqa: PLR2004
        assert h * (w + 1) <= ref.MARKER_TILE_MAX_PIXELS
    sizes = {h * w for (h, w, _) in shapes}
    assert {32000, 32001, 36864, 36865} <= sizes
    assert ref.route(160, 200, 21) == "A" and ref.route(10667, 3, 21) == "C"
    assert ref.route(192, 192, 21) == "C" and ref.route(365, 101, 21) == "D"


def test_tiny_maps_and_case_maps():
    npm, hv = ref.tiny_maps(4, 30, 50, seed=3)
    assert npm.shape == (4, 30, 50, 1) and hv.shape == (4, 30, 50, 2) and npm.dtype == hv.dtype == np.float32
    assert 0.77 < float((npm >= 0.5).mean()) < 0.83  # noqa: PLR2004
    assert np.all(np.diff(hv[0, 3, :, 0][::10]) > 0) and np.all(np.diff(hv[0, :, 7, 1][::10]) > 0)   # ramps, h along x, v along y
    assert np.abs(hv).max() < 1.2  # noqa: PLR2004
    again = ref.tiny_maps(4, 30, 50, seed=3)
    assert np.array_equal(npm, again[0]) and np.array_equal(hv, again[1])
    with pytest.raises(ValueError):  # noqa: PT011 -- the shapes synth_maps refuses are tiny_maps' reason to exist
        oh.synth_maps(1, 7, 50, seed=0, n_blobs=3)
    for (h, w) in ((2, 18433), (10667, 3), (96, 120)):
        a, b = ref.case_maps(2, h, w, seed=1)
        assert a.shape == (2, h, w, 1) and b.shape == (2, h, w, 2)


@pytest.mark.parametrize("scale", [1, 0.5])
def test_oracle_on_thin_and_tiny_planes(scale):
    for (h, w) in ref.TINY_SHAPES:
        npm, hv = ref.tiny_maps(2, h, w)
        for i in range(2):
            dbg = {}
            inst = oh.proc_np_hv(npm[i], hv[i], scale_factor=scale, debug=dbg)
            assert inst.shape == (h, w)
            for k in ("sobel_h_raw", "sobel_v_raw", "dist"):
                assert dbg[k].shape == (h, w) and dbg[k].dtype == np.float64 and np.isfinite(dbg[k]).all(), (h, w, k)
            assert set(np.unique(dbg["blb"])) <= {0, 1}
            if (h, w) in ref.TINY_NONEMPTY:
                assert dbg["blb"].any(), (h, w, i)
            assert np.array_equal(inst > 0, (dbg["blb"] > 0) & (inst > 0))
    assert set(ref.TINY_NONEMPTY) <= set(ref.TINY_SHAPES)
    anchor = ref.ksize_of(scale) // 2
    thin = [(h, w) for (h, w) in ref.TINY_SHAPES if h <= anchor or w <= anchor]
    near = [(h, w) for (h, w) in ref.TINY_SHAPES if h > anchor and w > anchor]
    assert thin and near   # both forms of the tile kernel's border reflection are reached at this size

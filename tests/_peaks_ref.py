"""An independent definition of ``peak_local_max`` and the planes the peak tests share.

:func:`brute_peaks` restates ``tiatoolbox_amd/utils/_peaks.py`` from the definitions alone: a direct window maximum per pixel (the
window clipped to the plane: replicating the edge only repeats pixels the clipped window already holds) and a naive greedy walk over
a list of accepted peaks -- no ``maximum_filter``, no occupancy plane.  Its two switches build the WRONG rules the helper test needs.
"""

from __future__ import annotations

import numpy as np


def brute_peaks(image, min_distance=1, threshold_abs=None, threshold_rel=None, exclude_border=False, num_peaks=np.inf, *,  # noqa: FBT002
                spacing_le: bool = False, threshold_ge: bool = False) -> np.ndarray:
    img = np.asarray(image, dtype=np.float32)
    h, w = img.shape
    d = int(min_distance)
    b = d if exclude_border is True else (0 if exclude_border is False else int(exclude_border))
    if img.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    t = np.float32(threshold_abs) if threshold_abs is not None else img.min()
    if threshold_rel is not None:
        t = max(t, np.float32(threshold_rel) * img.max())
    is_max = [[img[y, x] == img[max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1].max() for x in range(w)] for y in range(h)]
    if img.size > 1 and all(all(r) for r in is_max):
        return np.zeros((0, 2), dtype=np.int64)
    above = (lambda v: v >= t) if threshold_ge else (lambda v: v > t)
    cand = [(y, x) for y in range(h) for x in range(w)
            if (is_max[y][x] or img.size == 1) and above(img[y, x]) and b <= y < h - b and b <= x < w - b]
    cand.sort(key=lambda c: -float(img[c]))  # stable: ties stay in raster order
    out: list[tuple[int, int]] = []
    for y, x in cand:
        if len(out) >= num_peaks:
            break
        dist = [max(abs(y - py), abs(x - px)) for py, px in out]
        if any((q <= d) if spacing_le else (q < d) for q in dist):
            continue
        out.append((y, x))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def same_peaks(got, exp) -> bool:
    """The comparison every peak test uses: the same ``int64 [K, 2]`` array, order included."""
    got, exp = np.asarray(got), np.asarray(exp)
    return got.dtype == np.int64 and exp.dtype == np.int64 and got.ndim == 2 and got.shape == exp.shape and np.array_equal(got, exp)  # noqa: PLR2004


# ---------------------------------------------------------------------------------------------------------------- planes
def random_plane(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((h, w), dtype=np.float32)


def quantised_plane(h: int, w: int, seed: int, levels: int = 41) -> np.ndarray:
    """A random map rounded to ``levels`` values: ties everywhere, most candidates contested."""
    return (np.round(random_plane(h, w, seed) * (levels - 1)) / np.float32(levels - 1)).astype(np.float32)


def smooth_quantised_plane(h: int, w: int, seed: int, levels: int = 41, sigma: float = 3.0) -> np.ndarray:
    """A smooth map (Gaussian-filtered noise, stretched to [0, 1]) rounded to ``levels`` values: every hill top is a plateau."""
    from scipy import ndimage

    r = ndimage.gaussian_filter(random_plane(h, w, seed).astype(np.float64), sigma)
    r = (r - r.min()) / (r.max() - r.min())
    return (np.round(r * (levels - 1)) / np.float32(levels - 1)).astype(np.float32)


def discs_plane(h: int, w: int, seed: int, count: int = 6, radius: int = 6) -> np.ndarray:
    """Saturated sigmoid blobs: discs of exactly 1.0 on a smooth low background."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    out = (0.1 + 0.05 * np.sin(yy / 5.0) * np.cos(xx / 7.0)).astype(np.float32)
    for _ in range(count):
        cy, cx = rng.integers(0, h), rng.integers(0, w)
        out[(yy - cy) ** 2 + (xx - cx) ** 2 <= radius ** 2] = 1.0
    return out


def spikes_plane(h: int, w: int) -> np.ndarray:
    """Distinct peaks on the four corners, on every edge and inside."""
    out = np.zeros((h, w), dtype=np.float32)
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1),
             (h // 2, w // 2), (5, 5), (h - 6, w - 6), (h // 2, w // 2 + 3)]
    for i, (y, x) in enumerate(spots):
        out[y, x] = 1.0 + i
    return out


def special_values_plane(h: int, w: int, seed: int) -> np.ndarray:
    values = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], dtype=np.float32)
    return values[np.random.default_rng(seed).integers(0, len(values), (h, w))]


def small_planes(count: int = 200):
    """Seeded small planes with ties, each with a random set of options: ``(image, kwargs)``."""
    rng = np.random.default_rng(20240611)
    for i in range(count):
        h, w = int(rng.integers(1, 13)), int(rng.integers(1, 14))
        levels = int(rng.choice([2, 3, 5, 9, 1000]))
        img = (np.round(rng.random((h, w)) * (levels - 1)) / max(levels - 1, 1)).astype(np.float32)
        if i % 17 == 0:
            img[:] = img.flat[0]  # constant
        kw = {"min_distance": int(rng.integers(1, 5))}
        if rng.random() < 0.4:  # noqa: PLR2004
            kw["threshold_abs"] = float(rng.choice(img.ravel())) if rng.random() < 0.5 else float(rng.random())  # noqa: PLR2004
        if rng.random() < 0.3:  # noqa: PLR2004
            kw["threshold_rel"] = float(rng.choice([0.0, 0.25, 0.5, 1.0]))
        kw["exclude_border"] = [False, True, 0, 1, 2, 7][int(rng.integers(0, 6))]
        if rng.random() < 0.3:  # noqa: PLR2004
            kw["num_peaks"] = int(rng.integers(0, 6))
        yield img, kw


def device_cases(tile: int) -> dict:
    """Every case of the device test: ``name -> (planes [h, w] or [n, h, w], kwargs)``; ``tile`` is the kernel's tile side."""
    cases: dict = {}
    one = np.array([[0.5]], dtype=np.float32)
    cases["1x1"] = (one, {})
    cases["1x1_below_threshold_abs"] = (one, {"threshold_abs": 0.25})
    cases["1x1_at_threshold_abs"] = (one, {"threshold_abs": 0.5})
    cases["1x1_border"] = (one, {"threshold_abs": 0.25, "exclude_border": 1})
    cases["1x5"] = (np.array([[1, 3, 2, 3, 0]], dtype=np.float32), {"min_distance": 1})
    cases["1x5_d2"] = (np.array([[1, 3, 2, 3, 0]], dtype=np.float32), {"min_distance": 2})
    cases["5x1"] = (np.array([[2], [0], [1], [5], [5]], dtype=np.float32), {"min_distance": 1})
    cases["3x3_d7"] = (np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]], dtype=np.float32), {"min_distance": 7})
    for side in (tile - 1, tile, tile + 1, 2 * tile + 1):
        cases[f"side_{side}"] = (random_plane(side, side, side), {"min_distance": 3})
        cases[f"side_{side}_quantised"] = (quantised_plane(side, side, side + 1, 9), {"min_distance": 2})
    cases["rect"] = (random_plane(tile + 1, 2 * tile + 1, 5), {"min_distance": 4})
    const = np.full((40, 50), 0.25, dtype=np.float32)
    cases["batch_of_three"] = (np.stack([random_plane(40, 50, 7), quantised_plane(40, 50, 8), const]), {"min_distance": 2})
    cases["batch_no_candidates"] = (np.stack([const, const + 1]), {"min_distance": 2})
    for d in (1, 2, 7, 16, 64):
        cases[f"d{d}_random"] = (random_plane(70, 90, 10 + d), {"min_distance": d})
        cases[f"d{d}_quantised"] = (quantised_plane(70, 90, 20 + d, 5), {"min_distance": d})
    spikes = spikes_plane(37, 45)
    cases["corners_edges"] = (spikes, {"min_distance": 2})
    cases["corners_edges_d1"] = (spikes, {"min_distance": 1})
    for b in (0, 1, True, 10, 19, 30):  # True = min_distance; 19 > 37 / 2; 30 > 45 / 2: nothing left
        cases[f"border_{b}"] = (spikes, {"min_distance": 3, "exclude_border": b})
        cases[f"border_{b}_random"] = (random_plane(37, 45, 3), {"min_distance": 3, "exclude_border": b})
    cases["threshold_abs_at_a_peak"] = (spikes, {"min_distance": 2, "threshold_abs": 5.0})  # the peak of value 5 goes: strict
    cases["threshold_rel"] = (spikes, {"min_distance": 2, "threshold_rel": 0.5})
    cases["threshold_rel_at_a_peak"] = (spikes, {"min_distance": 2, "threshold_rel": 0.75})  # 0.75 * 12 = 9: strict
    cases["threshold_both_abs_wins"] = (spikes, {"min_distance": 2, "threshold_abs": 8.0, "threshold_rel": 0.25})
    cases["threshold_both_rel_wins"] = (spikes, {"min_distance": 2, "threshold_abs": 2.0, "threshold_rel": 0.5})
    cases["threshold_abs_below_minimum"] = (random_plane(20, 30, 4) + 1, {"min_distance": 2, "threshold_abs": -1.0})
    for d in (1, 2):
        cases[f"zeros_and_infinities_d{d}"] = (special_values_plane(33, 41, 6 + d), {"min_distance": d})
    cases["signed_zeros_only"] = (np.where(random_plane(9, 11, 2) < 0.5, np.float32(-0.0), np.float32(0.0)), {"min_distance": 1})  # noqa: PLR2004
    cases["infinite_threshold_rel"] = (special_values_plane(20, 20, 9), {"min_distance": 2, "threshold_rel": 0.5})
    cases["constant"] = (const, {"min_distance": 1})
    cases["two_valued"] = ((random_plane(41, 39, 11) < 0.3).astype(np.float32), {"min_distance": 2})  # noqa: PLR2004
    row = np.zeros((5, 304), dtype=np.float32)
    row[2, 2:302] = 1.0
    cases["row_of_300_d3"] = (row, {"min_distance": 3})
    cases["saturated_discs"] = (discs_plane(90, 120, 12), {"min_distance": 4})
    cases["saturated_discs_batch"] = (np.stack([discs_plane(50, 70, 13), discs_plane(50, 70, 14)]), {"min_distance": 3})
    yy, xx = np.mgrid[:34, :37]
    for d in (1, 2):
        cases[f"checkerboard_d{d}"] = (((yy + xx) % 2).astype(np.float32), {"min_distance": d})
    cases["quantised_257x300"] = (smooth_quantised_plane(257, 300, 15), {"min_distance": 3})
    cases["quantised_257x300_d1"] = (smooth_quantised_plane(257, 300, 15), {"min_distance": 1})
    cases["quantised_noise_257x300"] = (quantised_plane(257, 300, 15), {"min_distance": 3})
    return cases

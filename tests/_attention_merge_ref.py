"""Host-only helpers of the attention-merge tests: a NumPy restatement of the arithmetic ``merge_attention`` is specified by, written
from its text (``models/engine/_attention_merge.py``'s docstring) and importing nothing from the package, and the table of cases.

Every patch is evaluated on the full pixel mesh of its rectangle (``np.meshgrid``), in a floating-point type given by the caller:
``np.float32`` with the four per-patch numbers rounded once is the specification itself, bit for bit; ``np.float64`` with the numbers
left unrounded is the yardstick of its rounding error."""

from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24  # unit round-off of float32

# (Ws, Hs, patch w, patch h, stride, gh, gw, W, H)
CASES = [
    (256, 192, 64, 64, 64, 4, 4, 64, 48),
    (256, 192, 64, 64, 32, 4, 4, 64, 48),
    (300, 210, 56, 56, 40, 4, 4, 67, 47),
    (96, 64, 32, 32, 16, 2, 2, 192, 128),     # up-sampling
    (330, 250, 80, 96, 48, 6, 5, 83, 63),
    (672, 448, 224, 224, 112, 16, 16, 97, 65),
]
CASE_IDS = [f"{c[0]}x{c[1]}-p{c[2]}x{c[3]}-s{c[4]}-g{c[5]}x{c[6]}-{c[7]}x{c[8]}" for c in CASES]


def overlapping(case) -> bool:
    return case[4] < min(case[2], case[3])


def grid_coordinates(case) -> np.ndarray:
    """Patch bounds ``[N, 4]`` on a row-major grid from the origin, every start inside the patch space: the last column and row hang
    over the edge where the stride does not divide."""
    ws, hs, pw, ph, stride = case[:5]
    return np.array([(x, y, x + pw, y + ph) for y in range(0, hs, stride) for x in range(0, ws, stride)], dtype=np.int64)


def random_maps(n: int, c: int, gh: int, gw: int, seed: int) -> np.ndarray:
    """``rng.random`` grids, every patch's every channel divided by its own sum (as an attention row is)."""
    m = np.random.default_rng(seed).random((n, c, gh, gw))
    return (m / m.sum((-2, -1), keepdims=True)).astype(np.float32)


def case_inputs(case, c: int = 3, seed: int = 0) -> tuple[np.ndarray, np.ndarray]:
    coords = grid_coordinates(case)
    return coords, random_maps(len(coords), c, case[5], case[6], seed + 17 * CASES.index(case) if case in CASES else seed)


def rect_of(bounds, ws, hs, w, h) -> tuple[int, int, int, int]:
    """``X* = ceil(x* . fx)``, ``Y* = ceil(y* . fy)`` in float64, clipped to the canvas."""
    fx, fy = w / ws, h / hs
    x0, y0, x1, y1 = (float(v) for v in bounds)
    return (min(max(math.ceil(x0 * fx), 0), w), min(max(math.ceil(y0 * fy), 0), h),
            min(max(math.ceil(x1 * fx), 0), w), min(max(math.ceil(y1 * fy), 0), h))


def affine_of(bounds, rect, ws, hs, w, h, gh, gw) -> tuple[float, float, float, float]:
    """``(ax, cx, ay, cy)`` as Python floats (float64), each expression evaluated from left to right."""
    fx, fy = w / ws, h / hs
    x0, y0, x1, y1 = (float(v) for v in bounds)
    ax = gw / ((x1 - x0) * fx)
    cx = ((rect[0] + 0.5) / fx - x0) * gw / (x1 - x0) - 0.5
    ay = gh / ((y1 - y0) * fy)
    cy = ((rect[1] + 0.5) / fy - y0) * gh / (y1 - y0) - 0.5
    return ax, cx, ay, cy


def grid_coordinates_of_pixels(bounds, rect, space, canvas, grid, dtype):
    """``(gy, gx)`` meshes over the rectangle's pixels, clamped to the grid, in ``dtype``: float32 takes the four numbers rounded once."""
    (ws, hs), (h, w), (gh, gw) = space, canvas, grid
    ax, cx, ay, cy = (dtype(v) for v in affine_of(bounds, rect, ws, hs, w, h, gh, gw))
    yy, xx = np.meshgrid(np.arange(rect[1], rect[3]), np.arange(rect[0], rect[2]), indexing="ij")
    gx = ax * (xx - rect[0]).astype(dtype) + cx
    gy = ay * (yy - rect[1]).astype(dtype) + cy
    return np.clip(gy, dtype(0), dtype(gh - 1)), np.clip(gx, dtype(0), dtype(gw - 1))


def patch_samples(bounds, rect, grids, space, canvas, mode: str, dtype=np.float32) -> np.ndarray:
    """``[C, Y1 - Y0, X1 - X0]`` samples of one patch's ``grids`` ``[C, gh, gw]`` at the pixels of its rectangle."""
    gh, gw = grids.shape[-2:]
    gy, gx = grid_coordinates_of_pixels(bounds, rect, space, canvas, (gh, gw), dtype)
    m = grids.astype(dtype)
    if mode == "nearest":
        jx = np.minimum(np.floor(gx + dtype(0.5)).astype(np.int64), gw - 1)
        jy = np.minimum(np.floor(gy + dtype(0.5)).astype(np.int64), gh - 1)
        return m[:, jy, jx]
    jx0, jy0 = np.floor(gx).astype(np.int64), np.floor(gy).astype(np.int64)
    wx, wy = gx - jx0.astype(dtype), gy - jy0.astype(dtype)
    jx1, jy1 = np.minimum(jx0 + 1, gw - 1), np.minimum(jy0 + 1, gh - 1)
    v00, v01, v10, v11 = m[:, jy0, jx0], m[:, jy0, jx1], m[:, jy1, jx0], m[:, jy1, jx1]
    top = v00 + wx * (v01 - v00)
    bot = v10 + wx * (v11 - v10)
    out = top + wy * (bot - top)
    assert out.dtype == dtype
    return out


def merge(coords, maps, space, canvas, mode: str = "bilinear", *, descending: bool = False) -> dict:
    """``sum`` ``[C, H, W]``, ``count`` ``[H, W]``, ``raw`` ``[C, H, W]``: the patches added one at a time in ascending order
    (``descending``: in the opposite order, to show that the order matters)."""
    (ws, hs), (h, w) = space, canvas
    n, c = maps.shape[:2]
    total, count = np.zeros((c, h, w), dtype=np.float32), np.zeros((h, w), dtype=np.int32)
    for i in (range(n - 1, -1, -1) if descending else range(n)):
        r = rect_of(coords[i], ws, hs, w, h)
        if r[2] <= r[0] or r[3] <= r[1]:
            continue
        v = patch_samples(coords[i], r, maps[i], space, canvas, mode)
        total[:, r[1]:r[3], r[0]:r[2]] = total[:, r[1]:r[3], r[0]:r[2]] + v
        count[r[1]:r[3], r[0]:r[2]] += 1
    raw = (total.astype(np.float64) / (count.astype(np.float64) + 1e-8)).astype(np.float32)
    return {"sum": total, "count": count, "raw": raw}


def order_matters(coords, maps, space, canvas, mode: str) -> float:
    """Share of covered pixels (any channel) whose sum changes when the patches are added in descending order."""
    fwd, bwd = merge(coords, maps, space, canvas, mode), merge(coords, maps, space, canvas, mode, descending=True)
    covered = fwd["count"] > 0
    return float(((fwd["sum"] != bwd["sum"]).any(0) & covered).sum() / max(int(covered.sum()), 1))


def bilinear_bound(gh: int, gw: int, map_max: float) -> float:
    """``(3 (gw + 1) + 3 (gh + 1) + 6) u max(map)``: three roundings on a coordinate of magnitude at most ``g + 1``, times a slope of at
    most ``max(map)`` per cell, plus the roundings of the three lerps."""
    return (3 * (gw + 1) + 3 * (gh + 1) + 6) * U * map_max

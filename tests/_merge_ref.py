"""NumPy restatement of ``PatchPredictor.merge_predictions`` for the tests, written from the specification alone (it imports
nothing from the package): map-space rectangles, the slice-add loop in ascending patch order, raw map and labels; and the grid
cases both test files share."""

from __future__ import annotations

import math

import numpy as np

# (Ws, Hs, patch, stride, W, H, C): patch space, square patch and stride, canvas, classes
GRID_CASES = [
    (1000, 800, 224, 56, 63, 50, 9),
    (1000, 800, 224, 56, 370, 296, 9),
    (300, 260, 64, 16, 37, 53, 17),
    (512, 512, 224, 224, 32, 32, 2),
]


def rects(coordinates, ws: int, hs: int, w: int, h: int) -> np.ndarray:
    """``ceil(x * W / Ws)`` clipped to ``[0, W]``, ``ceil(y * H / Hs)`` clipped to ``[0, H]`` (float64) -> int32 ``[N, 4]``."""
    fx, fy = float(w) / float(ws), float(h) / float(hs)
    out = []
    for x0, y0, x1, y1 in np.asarray(coordinates).reshape(-1, 4).tolist():
        xa, xb = (min(max(math.ceil(float(v) * fx), 0), w) for v in (x0, x1))
        ya, yb = (min(max(math.ceil(float(v) * fy), 0), h) for v in (y0, y1))
        out.append((xa, ya, xb, yb))
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


def accumulate(rect, values, h: int, w: int, *, descending: bool = False):
    """``(sum float32 [H, W, C], count int32 [H, W])``: ``sum[y0:y1, x0:x1] += values[i]`` one patch at a time in ascending
    ``i`` (``descending``: the opposite order, for the tests that show the order matters)."""
    values = np.asarray(values, dtype=np.float32)
    total = np.zeros((h, w, values.shape[1]), dtype=np.float32)
    count = np.zeros((h, w), dtype=np.int32)
    order = range(len(rect) - 1, -1, -1) if descending else range(len(rect))
    for i in order:
        x0, y0, x1, y1 = (int(v) for v in rect[i])
        if x1 <= x0 or y1 <= y0:
            continue
        total[y0:y1, x0:x1, :] = total[y0:y1, x0:x1, :] + values[i][None, None, :]
        count[y0:y1, x0:x1] = count[y0:y1, x0:x1] + 1
    return total, count


def raw_map(total, count) -> np.ndarray:
    return (total.astype(np.float64) / (count.astype(np.float64)[:, :, None] + 1e-8)).astype(np.float32)


def labels(total, count) -> np.ndarray:
    lab = np.where(count > 0, 1 + np.argmax(total, axis=2), 0)
    return lab.astype(np.uint8 if total.shape[2] <= 254 else np.int32)


def merge(rect, values, h: int, w: int) -> dict:
    total, count = accumulate(rect, values, h, w)
    return {"sum": total, "count": count, "raw": raw_map(total, count), "labels": labels(total, count)}


def softmax_rows(n: int, c: int, seed: int) -> np.ndarray:
    """Softmax rows of seeded normals scaled by 2, float32."""
    z = 2.0 * np.random.default_rng(seed).standard_normal((n, c))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def grid_case(case, seed: int = 0):
    """``(coordinates int64 [N, 4], probabilities float32 [N, C])`` of a grid case: the regular grid of ``patch`` / ``stride``
    over the patch space (patches may hang over its edge), 20 % of the patches dropped at random."""
    ws, hs, patch, stride, _, _, c = case
    xs = np.arange(0, ws, stride)
    ys = np.arange(0, hs, stride)
    gx, gy = np.meshgrid(xs, ys)
    coords = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + patch, gy.ravel() + patch], axis=1).astype(np.int64)
    keep = np.random.default_rng(1000 + seed).random(len(coords)) >= 0.2
    coords = coords[keep]
    return coords, softmax_rows(len(coords), c, 2000 + seed)

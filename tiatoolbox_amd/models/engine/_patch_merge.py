"""Per-patch predictions painted into a whole-slide map (the arithmetic of the reference's
``PatchPredictor.merge_predictions``, ``tiatoolbox/models/engine/patch_predictor.py``).

Every patch ``i`` owns a rectangle of map pixels (:func:`patch_rects`); ``sum[Y, X, :]`` is the float32 sum of the rows
``values[i]`` of the patches whose rectangle holds ``(Y, X)``, added one at a time in ascending ``i`` -- what
``out[y0:y1, x0:x1] += values[i]`` in a loop over ``i`` computes -- and ``count[Y, X]`` is their number.  From these:
``raw = float32(float64(sum) / (float64(count) + 1e-8))`` and ``labels = 1 + argmax(sum)`` where ``count > 0``, else 0 (the
argmax of the sums is the argmax of the exact quotients: one positive divisor per pixel).

On the device this is ``tia_merge_patch_rects_f32`` (``csrc/canvas.hip``): a gather by map tiles over ascending per-tile
patch lists, no atomics, so the result equals the loop bit for bit.  Without a device (or with ``device="cpu"``) the loop
itself runs in NumPy: this step is host NumPy in the reference too.
"""

from __future__ import annotations

import numpy as np
import torch

_OUTPUTS = ("sum", "count", "raw", "labels")
_MAX_PIXELS = 1 << 31   # map pixels are indexed with int32 on the device
_MIN_TILE, _MAX_TILE = 16, 1024


def canvas_size(slide_dimensions, ratio: float) -> tuple[int, int]:
    """``(width, height)`` of a slide of baseline ``slide_dimensions = (width, height)`` seen at ``1 / ratio`` of its baseline
    resolution: ``np.round(dims / ratio)`` (halves to even), the rule of ``ResampledWSIView.slide_dimensions``."""
    w, h = (np.round(np.asarray(slide_dimensions, dtype=np.float64) / float(ratio))).astype(np.int64).tolist()
    return int(w), int(h)


def patch_rects(coordinates, patch_space, canvas_shape) -> np.ndarray:
    """Map-space rectangles ``int32 [N, 4]`` ``(X0, Y0, X1, Y1)`` (half-open) of the patch bounds ``coordinates`` ``[N, 4]``
    ``(x0, y0, x1, y1)`` given in a ``patch_space = (Ws, Hs)`` pixel space, on a canvas of ``canvas_shape = (H, W)`` pixels.

    In float64: ``fx = W / Ws``, ``fy = H / Hs``; ``X* = ceil(x* . fx)`` clipped to ``[0, W]``, ``Y* = ceil(y* . fy)`` clipped to
    ``[0, H]``.  A rectangle with ``X1 <= X0`` or ``Y1 <= Y0`` covers nothing (patches hanging over the slide edge, tiny factors).
    The reference scales the (x, y) bounds by a (y, x) factor; that only shows on canvases not proportional to the patch space,
    and this function scales x by ``fx`` and y by ``fy``."""
    c = np.asarray(coordinates.cpu() if isinstance(coordinates, torch.Tensor) else coordinates).reshape(-1, 4).astype(np.float64)
    ws, hs = float(patch_space[0]), float(patch_space[1])
    h, w = int(canvas_shape[0]), int(canvas_shape[1])
    if not (ws > 0 and hs > 0 and h > 0 and w > 0):
        msg = f"empty patch space {patch_space} or canvas {canvas_shape}."
        raise ValueError(msg)
    scale = np.array([w / ws, h / hs, w / ws, h / hs], dtype=np.float64)
    r = np.ceil(c * scale)
    r[:, 0::2] = np.clip(r[:, 0::2], 0, w)
    r[:, 1::2] = np.clip(r[:, 1::2], 0, h)
    return np.ascontiguousarray(r.astype(np.int32))


def label_dtype(classes: int):
    """``uint8`` while ``1 + argmax`` fits (``classes <= 254``), else ``int32``."""
    return np.uint8 if classes <= 254 else np.int32  # noqa: PLR2004


def _host_merge(rects: np.ndarray, values: np.ndarray, h: int, w: int, want: tuple[str, ...]) -> dict:
    """The loop itself, in NumPy."""
    c = values.shape[1]
    total = np.zeros((h, w, c), dtype=np.float32)
    count = np.zeros((h, w), dtype=np.int32)
    for (x0, y0, x1, y1), row in zip(rects.tolist(), values):
        if x1 <= x0 or y1 <= y0:
            continue
        total[y0:y1, x0:x1] += row
        count[y0:y1, x0:x1] += 1
    out = {}
    if "sum" in want:
        out["sum"] = total
    if "count" in want:
        out["count"] = count
    if "raw" in want:
        out["raw"] = (total.astype(np.float64) / (count.astype(np.float64)[..., None] + 1e-8)).astype(np.float32)
    if "labels" in want:
        out["labels"] = np.where(count > 0, total.argmax(-1) + 1, 0).astype(label_dtype(c))
    return out


def choose_tile(rects: np.ndarray) -> int:
    """Side of the (square) map tiles: the root of the mean area of the non-empty rectangles, rounded up to a multiple of 16
    within [16, 1024] -- a rectangle then meets about four tiles whatever its size, which bounds the (tile, patch) pairs."""
    wd = np.maximum(rects[:, 2].astype(np.int64) - rects[:, 0], 0)
    ht = np.maximum(rects[:, 3].astype(np.int64) - rects[:, 1], 0)
    area = (wd * ht)[(wd > 0) & (ht > 0)]
    side = float(np.sqrt(area.mean())) if len(area) else 1.0
    return int(min(max(-(-int(np.ceil(side)) // _MIN_TILE) * _MIN_TILE, _MIN_TILE), _MAX_TILE))


def _pair_counts(rects: np.ndarray, tile_h: int, tile_w: int):
    """Per rectangle: first tile column / row it meets and how many columns / rows (0 x 0 for an empty one), int64."""
    r = rects.astype(np.int64)
    live = (r[:, 2] > r[:, 0]) & (r[:, 3] > r[:, 1])
    tx0, ty0 = r[:, 0] // tile_w, r[:, 1] // tile_h
    nx = np.where(live, (r[:, 2] - 1) // tile_w - tx0 + 1, 0)
    ny = np.where(live, (r[:, 3] - 1) // tile_h - ty0 + 1, 0)
    return tx0, ty0, nx, ny


def build_tile_lists(rects_dev: torch.Tensor, h: int, w: int, tile_h: int, tile_w: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``(offsets int32 [tiles + 1], items int32 [pairs])``: for every tile of the map (row-major) the patches whose rectangle
    meets it, ASCENDING -- (tile, patch) pairs generated in patch order and stable-sorted by tile.  N-sized device plumbing."""
    dev = rects_dev.device
    tiles_x, tiles_y = -(-w // tile_w), -(-h // tile_h)
    r = rects_dev.to(torch.int64)
    live = (r[:, 2] > r[:, 0]) & (r[:, 3] > r[:, 1])
    tx0 = torch.div(r[:, 0], tile_w, rounding_mode="floor")
    ty0 = torch.div(r[:, 1], tile_h, rounding_mode="floor")
    zero = torch.zeros_like(tx0)
    nx = torch.where(live, torch.div(r[:, 2] - 1, tile_w, rounding_mode="floor") - tx0 + 1, zero)
    ny = torch.where(live, torch.div(r[:, 3] - 1, tile_h, rounding_mode="floor") - ty0 + 1, zero)
    per = nx * ny
    patch = torch.repeat_interleave(torch.arange(len(r), device=dev), per)
    start = torch.cumsum(per, 0) - per
    local = torch.arange(len(patch), device=dev) - start[patch]
    nxp = nx[patch]
    ly = torch.div(local, nxp, rounding_mode="floor")
    tile = (ty0[patch] + ly) * tiles_x + tx0[patch] + (local - ly * nxp)
    _, order = torch.sort(tile, stable=True)
    items = patch[order].to(torch.int32).contiguous()
    offsets = torch.zeros(tiles_x * tiles_y + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.bincount(tile, minlength=tiles_x * tiles_y), 0)
    if len(items) == 0:  # the entry point takes no null list: one unused item
        items = torch.zeros(1, dtype=torch.int32, device=dev)
    return offsets.to(torch.int32).contiguous(), items


def _too_large(h: int, w: int, c: int, why: str) -> ValueError:
    return ValueError(f"a merged map of {h} x {w} pixels with {c} classes {why}; choose a coarser `resolution` for the map.")


def merge_patch_rects(rects, values, canvas_shape, *, want=("labels",), device=None, tile=None) -> dict:
    """Paint the rows ``values`` ``[N, C]`` float32 into a ``canvas_shape = (H, W)`` map through the map-space rectangles
    ``rects`` ``[N, 4]`` int ``(X0, Y0, X1, Y1)`` (half-open, as from :func:`patch_rects`; clipped here once more).

    ``want`` names the outputs to return, any of ``"sum"`` ``[H, W, C]`` float32, ``"count"`` ``[H, W]`` int32, ``"raw"``
    ``[H, W, C]`` float32 and ``"labels"`` ``[H, W]`` (``uint8`` for ``C <= 254``, else ``int32``); see the module docstring for
    their definitions.  The result is a ``dict`` of arrays of the kind of ``values``: NumPy in, NumPy out; CUDA tensors in, CUDA
    tensors out, never visiting the host.  ``device``: ``"cpu"`` runs the NumPy loop, as does a machine without a HIP device;
    otherwise the kernel runs on ``values``' device (the current one for NumPy input).  ``tile = (tile_h, tile_w)`` overrides the
    tile size (:func:`choose_tile`).  A map of 2^31 pixels or more, or one whose outputs and lists do not fit the device's free
    memory, is a ``ValueError`` raised before anything is allocated."""
    want = tuple(want)
    if not want or any(k not in _OUTPUTS for k in want):
        msg = f"`want` names outputs among {_OUTPUTS}, got {want}."
        raise ValueError(msg)
    h, w = int(canvas_shape[0]), int(canvas_shape[1])
    if h <= 0 or w <= 0:
        msg = f"empty canvas {h} x {w}."
        raise ValueError(msg)
    if values.ndim != 2 or len(values) != len(rects) or values.shape[1] < 1:  # noqa: PLR2004
        msg = f"values [N, C] and rects [N, 4] must agree, got {tuple(values.shape)} and {tuple(rects.shape)}."
        raise ValueError(msg)
    c = int(values.shape[1])
    if h * w >= _MAX_PIXELS:
        raise _too_large(h, w, c, "has 2^31 pixels or more")
    as_tensor = isinstance(values, torch.Tensor)
    on_device = str(device) != "cpu" and torch.cuda.is_available() and (not as_tensor or values.is_cuda or device is not None)
    rects_np = np.asarray(rects.cpu() if isinstance(rects, torch.Tensor) else rects).reshape(-1, 4).astype(np.int64)
    rects_np[:, 0::2] = np.clip(rects_np[:, 0::2], 0, w)
    rects_np[:, 1::2] = np.clip(rects_np[:, 1::2], 0, h)
    rects_np = np.ascontiguousarray(rects_np.astype(np.int32))
    n = len(rects_np)
    if not on_device or n == 0:
        vals = values.detach().cpu().numpy() if as_tensor else np.asarray(values)
        out = _host_merge(rects_np, np.ascontiguousarray(vals, dtype=np.float32), h, w, want)
        return {k: torch.from_numpy(v).to(values.device) for k, v in out.items()} if as_tensor else out

    dev = values.device if as_tensor and values.is_cuda else torch.device(device if device is not None else "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    tile_h, tile_w = (int(tile[0]), int(tile[1])) if tile is not None else (choose_tile(rects_np),) * 2
    if tile_h <= 0 or tile_w <= 0:
        msg = f"tile sizes must be positive, got {tile}."
        raise ValueError(msg)
    tile_h, tile_w = min(tile_h, h), min(tile_w, w)
    # memory guard: the outputs, the lists and the int64 temporaries of the list building, against what the device has free
    _, _, nx, ny = _pair_counts(rects_np, tile_h, tile_w)
    pairs = int((nx * ny).sum())
    tiles = (-(-h // tile_h)) * (-(-w // tile_w))
    lab_bytes = np.dtype(label_dtype(c)).itemsize
    per_pixel = {"sum": 4 * c, "raw": 4 * c, "count": 4, "labels": lab_bytes}
    need = h * w * sum(per_pixel[k] for k in set(want)) + 4 * (pairs + tiles + 1) + 8 * (8 * pairs + 3 * tiles + 12 * n) + 4 * n * (c + 4)
    if pairs >= _MAX_PIXELS:
        raise _too_large(h, w, c, f"needs {pairs} (tile, patch) pairs, beyond the lists' 32-bit offsets")
    free, _ = torch.cuda.mem_get_info(dev)
    if need > free:
        raise _too_large(h, w, c, f"needs {need} bytes on the device, which has {free} free")

    with torch.cuda.device(dev):
        rects_dev = torch.from_numpy(rects_np).to(dev)
        vals = values if as_tensor else torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
        vals = vals.detach().to(device=dev, dtype=torch.float32).contiguous()
        offsets, items = build_tile_lists(rects_dev, h, w, tile_h, tile_w)
        out = launch_merge(rects_dev, vals, h, w, offsets, items, tile_h, tile_w, want)
    return out if as_tensor else {k: v.cpu().numpy() for k, v in out.items()}


def launch_merge(rects_dev, vals, h: int, w: int, offsets, items, tile_h: int, tile_w: int, want) -> dict:
    """One ``tia_merge_patch_rects_f32`` launch on the current stream; allocates the wanted outputs (every pixel is written)."""
    from tiatoolbox_amd import _lib

    n, c = vals.shape
    dev = vals.device
    out = {}
    if "sum" in want:
        out["sum"] = torch.empty((h, w, c), dtype=torch.float32, device=dev)
    if "raw" in want:
        out["raw"] = torch.empty((h, w, c), dtype=torch.float32, device=dev)
    if "count" in want:
        out["count"] = torch.empty((h, w), dtype=torch.int32, device=dev)
    lab_bytes = np.dtype(label_dtype(c)).itemsize
    if "labels" in want:
        out["labels"] = torch.empty((h, w), dtype=torch.uint8 if lab_bytes == 1 else torch.int32, device=dev)
    ptr = {k: (out[k].data_ptr() if k in out else None) for k in _OUTPUTS}
    rc = _lib.load().tia_merge_patch_rects_f32(rects_dev.data_ptr(), vals.data_ptr(), n, c, h, w, offsets.data_ptr(), items.data_ptr(),
                                               tile_h, tile_w, ptr["sum"], ptr["raw"], ptr["count"], ptr["labels"], lab_bytes,
                                               _lib.current_stream())
    _lib.check(rc, "tia_merge_patch_rects_f32")
    return out

"""Per-patch attention maps resampled into a whole-slide heat map (``PatchPredictor.merge_attention``).

**Inputs.**  ``coordinates`` ``[N, 4]``: the patch bounds ``(x0, y0, x1, y1)`` in a patch space of ``(Ws, Hs)`` pixels; ``maps``
``[N, C, gh, gw]`` float32, one grid of ``gh x gw`` cells per patch and channel (``C = heads`` for ``return_attention="class"``,
``C = 1`` for ``"rollout"``); a canvas of ``(H, W)`` pixels.

**Coverage** is exactly :func:`_patch_merge.patch_rects`: in float64 ``fx = W / Ws``, ``fy = H / Hs``, ``X* = ceil(x* . fx)``,
``Y* = ceil(y* . fy)``, clipped to the canvas, half-open.  ``count`` therefore equals what ``merge_patch_rects`` returns for the same
rectangles, bit for bit.

**Per patch** ``i`` with a non-empty rectangle the host computes four float32 numbers, each evaluated in float64 from left to right
and rounded once::

    ax = gw / ((x1 - x0) * fx)
    cx = ((X0 + 0.5) / fx - x0) * gw / (x1 - x0) - 0.5        (X0: the clipped left edge of the rectangle)
    ay = gh / ((y1 - y0) * fy)
    cy = ((Y0 + 0.5) / fy - y0) * gh / (y1 - y0) - 0.5

-- the centre of a canvas pixel mapped to grid coordinates whose cell centres are the integers (the ``align_corners=False``
convention), written relative to the rectangle's own corner so that the magnitudes stay small.

**Per covered pixel** ``(Y, X)``, all in float32, every operation rounded on its own (no contraction into an fma):

* ``gx = ax * float(X - X0) + cx`` clamped to ``[0, gw - 1]``; ``gy = ay * float(Y - Y0) + cy`` clamped to ``[0, gh - 1]``.
* ``interpolation="nearest"``: the sample is ``maps[i, k, jy, jx]`` with ``jx = min(int(floor(gx + 0.5f)), gw - 1)`` and ``jy`` likewise.
* ``interpolation="bilinear"`` (the default): ``j0 = int(floor(gx))``, ``wx = gx - j0`` (exact), ``j1 = min(j0 + 1, gw - 1)``, the same
  in y; with ``v00 = maps[i, k, jy0, jx0]``, ``v01 = maps[i, k, jy0, jx1]``, ``v10 = maps[i, k, jy1, jx0]``, ``v11 = maps[i, k, jy1, jx1]``:
  ``top = v00 + wx * (v01 - v00)``, ``bot = v10 + wx * (v11 - v10)``, ``v = top + wy * (bot - top)``.

**Outputs**, planar: ``sum[k, Y, X]`` = the float32 sum of the samples over the covering patches, added one at a time in ascending
``i``; ``count[Y, X]`` = their number (int32); ``raw = float32(float64(sum) / (float64(count) + 1e-8))`` -- the divisor of
``merge_predictions`` -- which is 0 where nothing covers.

On the device this is ``tia_merge_patch_grids_f32`` (``csrc/canvas.hip``): the gather by map tiles of ``tia_merge_patch_rects_f32``
over the same ascending per-tile lists, no atomics, compiled with floating-point contraction off, so the result equals the loop below
bit for bit.  Without a device (or with ``device="cpu"``) the loop itself runs in NumPy: it is the specification.
Nothing is normalised, per patch or per slide: "class" maps are relative within a patch.
"""

from __future__ import annotations

import numpy as np
import torch

from tiatoolbox_amd.models.engine import _patch_merge

_OUTPUTS = ("sum", "count", "raw")
INTERPOLATIONS = ("nearest", "bilinear")
_MAX_GRID_SIDE = 1 << 24  # gw - 1 and gh - 1, the ends of the clamp, are float32 numbers up to here


def patch_affines(coordinates, rects: np.ndarray, patch_space, canvas_shape, grid) -> np.ndarray:
    """``float32 [N, 4]`` ``(ax, cx, ay, cy)`` of the module docstring for the patch bounds ``coordinates`` and their map rectangles
    ``rects`` (:func:`_patch_merge.patch_rects`); zeros for a patch whose rectangle is empty."""
    c = np.asarray(coordinates.cpu() if isinstance(coordinates, torch.Tensor) else coordinates).reshape(-1, 4).astype(np.float64)
    gh, gw = float(grid[0]), float(grid[1])
    fx, fy = int(canvas_shape[1]) / float(patch_space[0]), int(canvas_shape[0]) / float(patch_space[1])
    r = rects.astype(np.float64)
    live = (rects[:, 2] > rects[:, 0]) & (rects[:, 3] > rects[:, 1])
    out = np.zeros((len(c), 4), dtype=np.float64)
    x0, y0, x1, y1 = (c[live, k] for k in range(4))  # a live rectangle has x1 > x0 and y1 > y0: ceil is monotonic
    out[live, 0] = gw / ((x1 - x0) * fx)
    out[live, 1] = ((r[live, 0] + 0.5) / fx - x0) * gw / (x1 - x0) - 0.5
    out[live, 2] = gh / ((y1 - y0) * fy)
    out[live, 3] = ((r[live, 1] + 0.5) / fy - y0) * gh / (y1 - y0) - 0.5
    return np.ascontiguousarray(out.astype(np.float32))


def _axis(a: np.float32, c: np.float32, length: int, cells: int, *, bilinear: bool):
    """Cell indices (and the weight) of ``length`` consecutive canvas pixels along one axis, in float32 as stated above."""
    g = a * np.arange(length, dtype=np.float32) + c
    g = np.minimum(np.maximum(g, np.float32(0.0)), np.float32(cells - 1))
    if not bilinear:
        return np.minimum(np.floor(g + np.float32(0.5)).astype(np.int64), cells - 1), None, None
    j0 = np.floor(g).astype(np.int64)
    return j0, np.minimum(j0 + 1, cells - 1), g - j0.astype(np.float32)


def _host_merge(rects: np.ndarray, affine: np.ndarray, maps: np.ndarray, h: int, w: int, mode: str, want: tuple[str, ...]) -> dict:
    """The loop itself, in NumPy float32: the specification."""
    _, c, gh, gw = maps.shape
    total = np.zeros((c, h, w), dtype=np.float32)
    count = np.zeros((h, w), dtype=np.int32)
    bilinear = mode == "bilinear"
    for i, (x0, y0, x1, y1) in enumerate(rects.tolist()):
        if x1 <= x0 or y1 <= y0:
            continue
        ax, cx, ay, cy = affine[i]
        jx0, jx1, wx = _axis(ax, cx, x1 - x0, gw, bilinear=bilinear)
        jy0, jy1, wy = _axis(ay, cy, y1 - y0, gh, bilinear=bilinear)
        m = maps[i]
        if not bilinear:
            v = m[:, jy0[:, None], jx0[None, :]]
        else:
            wx, wy = wx[None, None, :], wy[None, :, None]
            v00, v01 = m[:, jy0[:, None], jx0[None, :]], m[:, jy0[:, None], jx1[None, :]]
            v10, v11 = m[:, jy1[:, None], jx0[None, :]], m[:, jy1[:, None], jx1[None, :]]
            top = v00 + wx * (v01 - v00)
            bot = v10 + wx * (v11 - v10)
            v = top + wy * (bot - top)
        total[:, y0:y1, x0:x1] += v
        count[y0:y1, x0:x1] += 1
    out = {}
    if "sum" in want:
        out["sum"] = total
    if "count" in want:
        out["count"] = count
    if "raw" in want:
        out["raw"] = (total.astype(np.float64) / (count.astype(np.float64)[None] + 1e-8)).astype(np.float32)
    return out


def _too_large(h: int, w: int, c: int, why: str) -> ValueError:
    return ValueError(f"a merged attention map of {h} x {w} pixels with {c} channels {why}; choose a coarser `resolution` for the map.")


def merge_patch_grids(coordinates, maps, patch_space, canvas_shape, *, interpolation: str = "bilinear", want=("raw",), device=None,
                      tile=None) -> dict:
    """Resample the per-patch grids ``maps`` ``[N, C, gh, gw]`` float32 (or ``[N, gh, gw]``: one channel) of the patches at
    ``coordinates`` ``[N, 4]`` (``patch_space = (Ws, Hs)`` pixels) onto a ``canvas_shape = (H, W)`` map and average overlapping
    patches; the module docstring states the arithmetic.

    ``want`` names the outputs to return, any of ``"sum"`` / ``"raw"`` ``[C, H, W]`` float32 (``[H, W]`` for three-dimensional
    ``maps``) and ``"count"`` ``[H, W]`` int32.  The result is a ``dict`` of arrays of the kind of ``maps``: NumPy in, NumPy out; CUDA
    tensors in, CUDA tensors out, never visiting the host.  ``device="cpu"``, or a machine without a HIP device, runs the NumPy loop;
    otherwise ``tia_merge_patch_grids_f32`` runs on ``maps``' device (the current one for NumPy input).  ``tile = (tile_h, tile_w)``
    overrides the tile size (:func:`_patch_merge.choose_tile`).  A map of 2^31 pixels or more, or one whose outputs and lists do not
    fit the device's free memory, is a ``ValueError`` raised before anything is allocated."""
    want = tuple(want)
    if not want or any(k not in _OUTPUTS for k in want):
        msg = f"`want` names outputs among {_OUTPUTS}, got {want}."
        raise ValueError(msg)
    if interpolation not in INTERPOLATIONS:
        msg = f"`interpolation` is one of {INTERPOLATIONS}, got {interpolation!r}."
        raise ValueError(msg)
    h, w = int(canvas_shape[0]), int(canvas_shape[1])
    if h <= 0 or w <= 0:
        msg = f"empty canvas {h} x {w}."
        raise ValueError(msg)
    n = len(coordinates)
    squeeze = maps.ndim == 3  # noqa: PLR2004
    if maps.ndim not in (3, 4) or len(maps) != n or min(maps.shape[1:]) < 1:
        msg = f"maps [N, C, gh, gw] (or [N, gh, gw]) and coordinates [N, 4] must agree, got {tuple(maps.shape)} and {n} patches."
        raise ValueError(msg)
    if squeeze:
        maps = maps[:, None]
    c, gh, gw = (int(v) for v in maps.shape[1:])
    if max(gh, gw) > _MAX_GRID_SIDE:
        msg = f"a grid side above 2^24 cells is not supported (the clamp's upper end must be a float32 number), got {gh} x {gw}."
        raise ValueError(msg)
    if h * w >= _patch_merge._MAX_PIXELS:  # noqa: SLF001
        raise _too_large(h, w, c, "has 2^31 pixels or more")
    as_tensor = isinstance(maps, torch.Tensor)
    on_device = str(device) != "cpu" and torch.cuda.is_available() and (not as_tensor or maps.is_cuda or device is not None)
    rects = _patch_merge.patch_rects(coordinates, patch_space, (h, w))
    affine = patch_affines(coordinates, rects, patch_space, (h, w), (gh, gw))

    def finish(out: dict) -> dict:
        return {k: (v[0] if squeeze and k != "count" else v) for k, v in out.items()}

    if not on_device or n == 0:
        grids = maps.detach().cpu().numpy() if as_tensor else np.asarray(maps)
        out = _host_merge(rects, affine, np.ascontiguousarray(grids, dtype=np.float32), h, w, interpolation, want)
        return finish({k: torch.from_numpy(v).to(maps.device) for k, v in out.items()} if as_tensor else out)

    dev = maps.device if as_tensor and maps.is_cuda else torch.device(device if device is not None else "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    tile_h, tile_w = (int(tile[0]), int(tile[1])) if tile is not None else (_patch_merge.choose_tile(rects),) * 2
    if tile_h <= 0 or tile_w <= 0:
        msg = f"tile sizes must be positive, got {tile}."
        raise ValueError(msg)
    tile_h, tile_w = min(tile_h, h), min(tile_w, w)
    # memory guard: the outputs, the lists and the int64 temporaries of the list building, against what the device has free
    _, _, nx, ny = _patch_merge._pair_counts(rects, tile_h, tile_w)  # noqa: SLF001
    pairs = int((nx * ny).sum())
    tiles = (-(-h // tile_h)) * (-(-w // tile_w))
    per_pixel = {"sum": 4 * c, "raw": 4 * c, "count": 4}
    need = h * w * sum(per_pixel[k] for k in set(want)) + 4 * (pairs + tiles + 1) + 8 * (8 * pairs + 3 * tiles + 12 * n) + 4 * n * 8
    if not (as_tensor and maps.is_cuda and maps.dtype == torch.float32 and maps.is_contiguous()):
        need += 4 * n * c * gh * gw
    if pairs >= _patch_merge._MAX_PIXELS:  # noqa: SLF001
        raise _too_large(h, w, c, f"needs {pairs} (tile, patch) pairs, beyond the lists' 32-bit offsets")
    free, _ = torch.cuda.mem_get_info(dev)
    if need > free:
        raise _too_large(h, w, c, f"needs {need} bytes on the device, which has {free} free")

    with torch.cuda.device(dev):
        rects_dev = torch.from_numpy(rects).to(dev)
        affine_dev = torch.from_numpy(affine).to(dev)
        grids = maps if as_tensor else torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float32))
        grids = grids.detach().to(device=dev, dtype=torch.float32).contiguous()
        offsets, items = _patch_merge.build_tile_lists(rects_dev, h, w, tile_h, tile_w)
        out = launch_merge(rects_dev, affine_dev, grids, h, w, offsets, items, tile_h, tile_w, interpolation, want)
    return finish(out if as_tensor else {k: v.cpu().numpy() for k, v in out.items()})


def launch_merge(rects_dev, affine_dev, grids, h: int, w: int, offsets, items, tile_h: int, tile_w: int, interpolation: str, want) -> dict:
    """One ``tia_merge_patch_grids_f32`` launch on the current stream; allocates the wanted outputs (every pixel is written)."""
    from tiatoolbox_amd import _lib

    n, c, gh, gw = grids.shape
    dev = grids.device
    out = {}
    if "sum" in want:
        out["sum"] = torch.empty((c, h, w), dtype=torch.float32, device=dev)
    if "raw" in want:
        out["raw"] = torch.empty((c, h, w), dtype=torch.float32, device=dev)
    if "count" in want:
        out["count"] = torch.empty((h, w), dtype=torch.int32, device=dev)
    ptr = {k: (out[k].data_ptr() if k in out else None) for k in _OUTPUTS}
    rc = _lib.load().tia_merge_patch_grids_f32(rects_dev.data_ptr(), affine_dev.data_ptr(), grids.data_ptr(), n, c, gh, gw, h, w,
                                               offsets.data_ptr(), items.data_ptr(), tile_h, tile_w, INTERPOLATIONS.index(interpolation),
                                               ptr["sum"], ptr["raw"], ptr["count"], _lib.current_stream())
    _lib.check(rc, "tia_merge_patch_grids_f32")
    return out

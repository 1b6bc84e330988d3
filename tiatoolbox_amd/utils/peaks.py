"""``peak_local_max`` on probability maps, on the device.

``skimage.feature.peak_local_max`` with a square footprint, ``p_norm=inf`` and no ``labels`` -- what the reference's detection
models (``mapde``, ``sccnn``) call in ``postproc`` -- for float32 maps that already live in HBM: stitched probability canvases,
``merged_attention``, ``merged_cam``.  ``utils/_peaks.py`` states the result; a CUDA tensor is served by ``csrc/peaks.hip``
(``tia_peak_scan_f32`` / ``tia_peak_write_f32``), a CPU tensor by the statement itself.

One call on the device: per-plane minimum and maximum, window maximum on LDS tiles, candidate flags, the flags' window count
(contested candidates), count pass, ONE read of the totals, write pass.  Candidates that have no other candidate at Chebyshev
distance ``< min_distance`` are peaks and never visit the host; the contested ones (ties on plateaus) go to the host as
coordinates, are walked in raster order by ``tia_peak_resolve_host`` and return as one mask.  The stable descending sort is
``torch.sort``.  The number of host synchronisations per call is constant: it depends neither on the plane's size nor on the batch.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from tiatoolbox_amd import _lib
from tiatoolbox_amd.utils import _peaks

__all__ = ["peak_local_max", "peak_local_max_planes"]


def _checked_options(min_distance, exclude_border, num_peaks) -> tuple[int, int, float]:
    if isinstance(min_distance, bool) or not isinstance(min_distance, (int, np.integer)):
        msg = f"`min_distance` must be an int, got {min_distance!r}."
        raise ValueError(msg)  # noqa: TRY004  (every refusal of this function is a ValueError)
    d = int(min_distance)
    if not 1 <= d <= _peaks.MAX_MIN_DISTANCE:
        msg = f"`min_distance` must lie in [1, {_peaks.MAX_MIN_DISTANCE}] (the kernels' window), got {d}."
        raise ValueError(msg)
    b = _peaks.border_width(exclude_border, d)
    if num_peaks is None or not (num_peaks == np.inf or (float(num_peaks) == int(num_peaks) and num_peaks >= 0)):
        msg = f"`num_peaks` must be a whole number >= 0 or inf, got {num_peaks!r}."
        raise ValueError(msg)
    return d, b, float(num_peaks)


def _checked_image(image) -> torch.Tensor:
    if not isinstance(image, torch.Tensor):
        msg = f"`image` must be a torch.Tensor (CUDA for the kernels, CPU for the statement), got {type(image).__name__}."
        raise ValueError(msg)  # noqa: TRY004
    if image.dtype != torch.float32 or image.ndim not in (2, 3):
        msg = f"`image` must be float32 [h, w] or [n, h, w], got {image.dtype} {tuple(image.shape)}."
        raise ValueError(msg)
    if image.shape[-1] * image.shape[-2] >= 2 ** 31:
        msg = f"a plane must have fewer than 2^31 pixels, got {tuple(image.shape[-2:])}."
        raise ValueError(msg)
    return image


def _planes_cpu(planes: torch.Tensor, d: int, threshold_abs, threshold_rel, b: int, num_peaks: float):
    coords, values, counts = [], [], []
    for plane in planes.detach().numpy():
        c = _peaks.peak_local_max_ref(plane, d, threshold_abs, threshold_rel, b, num_peaks)
        coords.append(c)
        values.append(plane[c[:, 0], c[:, 1]])
        counts.append(len(c))
    return (torch.from_numpy(np.concatenate(coords).reshape(-1, 2)), torch.from_numpy(np.concatenate(values).astype(np.float32)),
            counts)


def _resolve_contested(yx: torch.Tensor, plane_id: torch.Tensor, contested: torch.Tensor, n: int, w: int, d: int):
    """Mask over the candidates: ``True`` for every uncontested one and for the contested ones the raster-order walk accepts.
    ``None`` when nothing is contested.  Only the contested candidates' coordinates cross to the host."""
    idx = torch.nonzero(contested).flatten()
    if idx.numel() == 0:
        return None
    c_yx = np.ascontiguousarray(yx[idx].cpu().numpy(), dtype=np.int32)
    c_plane = plane_id[idx].cpu().numpy()
    accept = np.zeros(len(c_yx), dtype=np.uint8)
    lib = _lib.load()
    cuts = np.searchsorted(c_plane, np.arange(n + 1))  # the candidates are ordered by plane, then raster
    for p in np.unique(c_plane):
        lo, hi = int(cuts[p]), int(cuts[p + 1])
        rc = lib.tia_peak_resolve_host(C.c_void_p(c_yx[lo:hi].ctypes.data), hi - lo, w, d, C.c_void_p(accept[lo:hi].ctypes.data))
        _lib.check(rc, "tia_peak_resolve_host")
    keep = torch.ones(yx.shape[0], dtype=torch.bool, device=yx.device)
    keep[idx] = torch.from_numpy(accept.astype(bool)).to(yx.device)
    return keep


def _planes_cuda(planes: torch.Tensor, d: int, threshold_abs, threshold_rel, b: int, num_peaks: float):
    n, h, w = (int(s) for s in planes.shape)
    dev = planes.device
    planes = planes.detach().contiguous()
    lib = _lib.load()
    chunks = int(lib.tia_peak_chunks(h, w))
    minmax = torch.empty((n, 2), dtype=torch.int32, device=dev)
    flags = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    state = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    offsets = torch.empty((n, chunks), dtype=torch.int32, device=dev)
    totals = torch.empty(n, dtype=torch.int64, device=dev)
    t_abs = float(np.float32(threshold_abs)) if threshold_abs is not None else 0.0
    t_rel = float(np.float32(threshold_rel)) if threshold_rel is not None else 0.0
    with torch.cuda.device(dev):
        rc = lib.tia_peak_scan_f32(planes.data_ptr(), n, h, w, d, int(threshold_abs is not None), t_abs,
                                   int(threshold_rel is not None), t_rel, b, minmax.data_ptr(), flags.data_ptr(), state.data_ptr(),
                                   offsets.data_ptr(), totals.data_ptr(), _lib.current_stream())
        _lib.check(rc, "tia_peak_scan_f32")
        totals_h = totals.cpu().numpy()  # the one read between the count pass and the write pass
        cap = int(totals_h.sum())
        yx = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        value = torch.empty(cap, dtype=torch.float32, device=dev)
        contested = torch.empty(cap, dtype=torch.uint8, device=dev)
        if cap == 0:
            return yx.to(torch.int64), value, [0] * n
        bases = torch.from_numpy(np.concatenate([[0], np.cumsum(totals_h)[:-1]]).astype(np.int64)).to(dev)
        rc = lib.tia_peak_write_f32(planes.data_ptr(), state.data_ptr(), n, h, w, offsets.data_ptr(), bases.data_ptr(), cap,
                                    yx.data_ptr(), value.data_ptr(), contested.data_ptr(), _lib.current_stream())
        _lib.check(rc, "tia_peak_write_f32")
    del flags, state
    plane_id = torch.repeat_interleave(torch.arange(n, device=dev), totals, output_size=cap)
    if d > 1:  # at min_distance 1 the strict spacing test can reject nothing
        keep = _resolve_contested(yx, plane_id, contested, n, w, d)
        if keep is not None:
            yx, value, plane_id = yx[keep], value[keep], plane_id[keep]
    # descending value, stable in raster order, plane by plane: two stable sorts (-0 and +0 are one value)
    key = torch.where(value == 0, torch.zeros_like(value), value)
    by_value = torch.sort(key, descending=True, stable=True).indices
    order = by_value[torch.sort(plane_id[by_value], stable=True).indices]
    yx, value, plane_id = yx[order], value[order], plane_id[order]
    counts = torch.bincount(plane_id, minlength=n)
    if num_peaks != np.inf:
        first = torch.cumsum(counts, 0) - counts
        head = torch.arange(yx.shape[0], device=dev) - first[plane_id] < int(num_peaks)
        yx, value = yx[head], value[head]
        counts = torch.clamp(counts, max=int(num_peaks))
    return yx.to(torch.int64), value, [int(c) for c in counts.cpu()]


def peak_local_max_planes(planes: torch.Tensor, min_distance: int = 1, threshold_abs=None, threshold_rel=None,
                          exclude_border=False, num_peaks=np.inf):  # noqa: FBT002
    """:func:`peak_local_max` of a batch ``[n, h, w]`` in flat form: ``(coordinates int64 [K, 2] (row, col), values float32 [K],
    counts)`` on the planes' device -- plane after plane, each in the statement's order, ``counts[i]`` peaks for plane ``i``;
    ``values`` are the planes' values at the peaks."""
    planes = _checked_image(planes)
    if planes.ndim != 3:  # noqa: PLR2004
        msg = f"`planes` must be [n, h, w], got {tuple(planes.shape)}."
        raise ValueError(msg)
    d, b, k = _checked_options(min_distance, exclude_border, num_peaks)
    if planes.numel() == 0:
        return (torch.zeros((0, 2), dtype=torch.int64, device=planes.device), torch.zeros(0, dtype=torch.float32, device=planes.device),
                [0] * int(planes.shape[0]))
    if planes.is_cuda:
        return _planes_cuda(planes, d, threshold_abs, threshold_rel, b, k)
    return _planes_cpu(planes, d, threshold_abs, threshold_rel, b, k)


def peak_local_max(image: torch.Tensor, min_distance: int = 1, threshold_abs=None, threshold_rel=None, exclude_border=False,  # noqa: FBT002
                   num_peaks=np.inf):
    """Peaks of a float32 map ``[h, w]`` (returns ``int64 [K, 2]`` as ``(row, col)``) or of a batch ``[n, h, w]`` (returns a list
    of them), on the tensor's device, in the order of ``utils/_peaks.py``: descending value, ties in raster order.

    ``min_distance`` (1 .. 64): peaks are the maxima of their ``(2 min_distance + 1)^2`` window and accepted peaks keep a
    Chebyshev distance ``>= min_distance``.  ``threshold_abs`` / ``threshold_rel``: a peak is strictly above
    ``max(threshold_abs or the map's minimum, threshold_rel * the map's maximum)``.  ``exclude_border``: ``True`` =
    ``min_distance``, or a width in pixels.  ``num_peaks``: at most that many per map.  ``labels``, ``footprint`` and other
    ``p_norm`` are not covered.  NaN is outside the domain.  A ``ValueError`` before any launch: a wrong dtype or rank,
    ``min_distance`` outside 1 .. 64, a negative ``exclude_border``."""
    image = _checked_image(image)
    planes = image[None] if image.ndim == 2 else image  # noqa: PLR2004
    coords, _, counts = peak_local_max_planes(planes, min_distance, threshold_abs, threshold_rel, exclude_border, num_peaks)
    parts = list(torch.split(coords, counts))
    return parts[0] if image.ndim == 2 else parts  # noqa: PLR2004

"""Minimal in-memory whole-slide reader (the part of reference ``wsicore/wsireader.py`` the engines
need: ``VirtualWSIReader`` :3121-3694, ``slide_thumbnail``, ``tissue_mask`` :1735-1786).

File-format readers (OpenSlide, TIFF, DICOM, ...) are out of scope: a slide is an
``H x W x 3`` uint8 array (NumPy or CUDA tensor) with an objective power / mpp.  Reads happen on the
GPU: the level-0 image lives in HBM (a 20k x 20k slide is 1.2 GB of the 288 GB) and a batch of patches is
gathered by one kernel launch (``tia_gather_patches_u8``) that writes 255 wherever a region leaves the slide, exactly
as ``WSIPatchDataset.__getitem__`` pads (``dataset_abc.py:430-436``).

``ArrayWSIReader`` reads at the slide's own resolution only.  ``VirtualWSIReader`` (the reference's class name) also reads
below it, by an integer factor ``k`` (:func:`resolution_factor`) or, with ``fractional=True``, by any ratio ``s >= 1``
(:func:`resolution_scale`): ``read_bounds(..., resolution, units)`` and the light view ``at_resolution(resolution, units)``
take the baseline region, pad it with 255 outside the slide and shrink it with ``cv2.INTER_AREA`` in one launch
(``tia_gather_area_patches_u8`` at an integer scale, ``tia_gather_area_resize_u8`` at any other), which is what the
reference's ``read_bounds`` -> ``imresize`` does.  With ``upsample=True`` it also reads above the baseline resolution, by
any ratio ``s`` in ``[1/64, 1)``: the region is padded the same way and enlarged with ``cv2.INTER_CUBIC``
(``tia_gather_cubic_resize_u8``), as ``imresize(..., interpolation="optimise")`` does at a scale above 1.  Up-sampling is
opt-in; anisotropic mpp and multi-level pyramids are not supported.
"""

from __future__ import annotations

import logging

import numpy as np
import torch

from tiatoolbox_amd.utils import _tensors

logger = logging.getLogger(__name__)


class ArrayWSIReader:
    """ndarray-backed slide at a single (baseline) resolution."""

    def __init__(self, img, mpp: float | None = 0.25, power: float | None = 40.0, mode: str = "rgb") -> None:
        if isinstance(img, torch.Tensor):
            self._dev = img if img.is_cuda else img.to(_tensors.default_device())
        else:
            self._dev = torch.from_numpy(np.ascontiguousarray(img)).to(_tensors.default_device())
        self.mode = mode
        self.mpp = mpp
        self.power = power

    @property
    def img(self) -> np.ndarray:
        return self._dev.cpu().numpy()

    @property
    def device_image(self) -> torch.Tensor:
        return self._dev

    @property
    def slide_dimensions(self) -> tuple[int, int]:
        return int(self._dev.shape[1]), int(self._dev.shape[0])  # (width, height)

    # ------------------------------------------------------------------------------- reads
    def read_bounds_batch(self, bounds, pad_value: int = 255, *, size: tuple[int, int] | None = None) -> torch.Tensor:
        """Stack of equally-sized regions ``[x0, y0, x1, y1]`` (baseline pixels), ``pad_value`` outside the slide:
        one gather launch (``tia_gather_patches_u8``) writes the whole ``[M, ph, pw, C]`` batch.

        ``bounds`` may already be an ``int32 [M, 4]`` tensor on the slide's device (with ``size=(pw, ph)``): the WSI loops
        upload every patch's bounds once and pass slices, so that no batch waits on a host -> device copy."""
        from tiatoolbox_amd import _lib

        if isinstance(bounds, torch.Tensor) and bounds.is_cuda:
            if size is None or bounds.dtype != torch.int32 or bounds.dim() != 2 or bounds.shape[1] != 4 or not bounds.is_contiguous():  # noqa: PLR2004
                msg = "device bounds: a contiguous int32 [M, 4] tensor together with size=(pw, ph)."
                raise ValueError(msg)
            src = self._dev if self._dev.dim() == 3 else self._dev[..., None]  # noqa: PLR2004
            pw, ph = int(size[0]), int(size[1])
            if src.dtype != torch.uint8 or not src.is_contiguous() or (ph * pw * src.shape[2]) % 4 != 0 or len(bounds) > 65535:  # noqa: PLR2004
                return self.read_bounds_batch(bounds.cpu().numpy(), pad_value)
            sh, sw, c = src.shape
            out = torch.empty((len(bounds), ph, pw, c), dtype=torch.uint8, device=src.device)
            with torch.cuda.device(src.device):
                rc = _lib.load().tia_gather_patches_u8(src.data_ptr(), sh, sw, c, bounds.data_ptr(), len(bounds), ph, pw, int(pad_value),
                                                       out.data_ptr(), _lib.current_stream())
            _lib.check(rc, "tia_gather_patches_u8")
            return out if self._dev.dim() == 3 else out[..., 0]  # noqa: PLR2004
        bounds = np.ascontiguousarray(np.asarray(bounds).reshape(-1, 4), dtype=np.int32)
        sizes = np.unique(np.stack([bounds[:, 2] - bounds[:, 0], bounds[:, 3] - bounds[:, 1]], axis=1), axis=0)
        if len(sizes) != 1:
            msg = "read_bounds_batch expects regions of one size."
            raise ValueError(msg)
        pw, ph = int(sizes[0, 0]), int(sizes[0, 1])
        src = self._dev if self._dev.dim() == 3 else self._dev[..., None]  # noqa: PLR2004
        src = src.contiguous()
        if src.dtype == torch.bool:
            src = src.to(torch.uint8)
        if src.dtype != torch.uint8:
            msg = "device patch reads need a uint8 slide."
            raise TypeError(msg)
        sh, sw, c = src.shape
        m = len(bounds)
        out = torch.empty((m, ph, pw, c), dtype=torch.uint8, device=src.device)
        if (ph * pw * c) % 4 != 0:  # odd-sized patches: plain slicing of a padded copy (rare; keeps the contract)
            pad = max(0, -int(bounds[:, :2].min()), int(bounds[:, 2].max()) - sw, int(bounds[:, 3].max()) - sh)
            padded = torch.nn.functional.pad(src.permute(2, 0, 1), (pad, pad, pad, pad), value=pad_value).permute(1, 2, 0)
            for i, (x0, y0, x1, y1) in enumerate(bounds.tolist()):
                out[i] = padded[y0 + pad:y1 + pad, x0 + pad:x1 + pad]
        else:
            bt = torch.from_numpy(bounds).to(src.device)
            lib = _lib.load()
            with torch.cuda.device(src.device):
                for s in range(0, m, 65535):
                    k = min(65535, m - s)
                    rc = lib.tia_gather_patches_u8(src.data_ptr(), sh, sw, c, bt[s:s + k].data_ptr(), k, ph, pw, int(pad_value),
                                                   out[s:s + k].data_ptr(), _lib.current_stream())
                    _lib.check(rc, "tia_gather_patches_u8")
        return out if self._dev.dim() == 3 else out[..., 0]  # noqa: PLR2004

    def read_bounds(self, bounds) -> np.ndarray:
        return self.read_bounds_batch(np.asarray(bounds)[None])[0].cpu().numpy()

    # ---------------------------------------------------------------------- thumbnail / mask
    def slide_thumbnail(self, resolution: float = 1.25, units: str = "power") -> torch.Tensor:
        """Thumbnail at the requested objective power, uint8.  The reference reads it through ``imresize`` whose
        down-sampling interpolation is ``cv2.INTER_AREA`` (``utils/transforms.py:imresize``, ``wsireader.py:1735-1786``);
        for an integer factor that is the exact box mean rounded half-to-even (``cvRound``), which is what this does."""
        if units != "power" or self.power is None:
            msg = "ArrayWSIReader thumbnails are requested by objective power."
            raise ValueError(msg)
        ratio = self.power / resolution
        factor = max(1, int(round(ratio)))
        if abs(ratio - factor) > 1e-9:  # noqa: PLR2004
            msg = (f"ArrayWSIReader holds one (baseline) level: thumbnails need an integer down-sampling factor, got "
                   f"{self.power}/{resolution}.")
            raise ValueError(msg)
        h, w = self._dev.shape[:2]
        th, tw = h // factor, w // factor
        if th == 0 or tw == 0:
            msg = f"the slide ({h} x {w}) is smaller than one thumbnail pixel at factor {factor}."
            raise ValueError(msg)
        from tiatoolbox_amd import _lib

        src = self._dev if self._dev.dim() == 3 else self._dev[..., None]  # noqa: PLR2004
        src = (src.to(torch.uint8) if src.dtype != torch.uint8 else src).contiguous()
        c = src.shape[-1]
        out = torch.empty((th, tw, c), dtype=torch.uint8, device=src.device)
        with torch.cuda.device(src.device):  # integer box sums on the device: no float32 copy of the slide
            rc = _lib.load().tia_box_downsample_u8(src.data_ptr(), h, w, c, factor, out.data_ptr(), _lib.current_stream())
        _lib.check(rc, "tia_box_downsample_u8")
        return out if self._dev.dim() == 3 else out[..., 0]  # noqa: PLR2004

    def tissue_mask(self, method: str = "otsu", resolution: float = 1.25, units: str = "power", **masker_kwargs):
        """Tissue mask reader from the thumbnail (ref. ``wsireader.py:1735-1786``)."""
        from tiatoolbox_amd.tools import tissuemask

        thumb = self.slide_thumbnail(resolution, units)
        if method not in ("otsu", "morphological"):
            msg = f"Invalid tissue masking method: {method}."
            raise ValueError(msg)
        if method == "otsu":
            masker = tissuemask.OtsuTissueMasker(**masker_kwargs)
        else:
            masker = tissuemask.MorphologicalMasker(**({"power": resolution} | masker_kwargs))
        mask = masker.fit_transform(thumb[None])[0]
        return ArrayWSIReader(mask.to(torch.uint8) if isinstance(mask, torch.Tensor) else mask.astype(np.uint8),
                              mpp=None, power=resolution, mode="bool")


# ------------------------------------------------------------------------------------------- reads below baseline
_REL_TOL = 1e-6  # two resolutions are the same, and a ratio is an integer, within this relative tolerance
_MAX_UPSAMPLE = 64  # an up-sampling reader enlarges the slide by at most this ratio (scale >= 1 / 64)


def _close(a: float, b: float) -> bool:
    return abs(a - b) <= _REL_TOL * max(1.0, abs(a), abs(b))


def _resolution_ratio(resolution: float, units: str, mpp, power) -> float:
    """Down-sampling ratio from a slide at (``mpp``, ``power``) to ``(resolution, units)``: every check of
    :func:`resolution_factor` except the up-sampling and integer ones."""
    if units == "level":
        if not _close(float(resolution), 0.0):
            msg = f"the in-memory slide holds one level (level 0); level {resolution} was requested."
            raise ValueError(msg)
        return 1.0
    if units not in ("mpp", "power", "baseline"):
        msg = f"Invalid resolution units `{units}`: expected 'mpp', 'power', 'baseline' or 'level'."
        raise ValueError(msg)
    resolution = float(resolution)
    if not resolution > 0:
        msg = f"the requested resolution must be positive, got {resolution} {units}."
        raise ValueError(msg)
    if units == "baseline":
        return 1.0 / resolution
    native = mpp if units == "mpp" else power
    if native is None:
        msg = f"the slide's native {units} is None: a read at {resolution} {units} cannot be placed."
        raise ValueError(msg)
    comps = [float(v) for v in np.asarray(native, dtype=np.float64).ravel()]
    if not all(_close(v, comps[0]) for v in comps):
        msg = f"the slide's mpp differs between x and y ({tuple(comps)}): anisotropic slides are not resampled."
        raise ValueError(msg)
    return resolution / comps[0] if units == "mpp" else comps[0] / resolution


def resolution_factor(resolution: float, units: str, *, mpp=None, power: float | None = None) -> int:
    """Integer down-sampling factor ``k`` from a slide at (``mpp``, ``power``) to the requested ``(resolution, units)``.

    ``units``: ``"mpp"`` (k = resolution / mpp), ``"power"`` (k = power / resolution), ``"baseline"`` (a scale of the
    baseline: k = 1 / resolution) or ``"level"`` (only level 0, k = 1).  ``ValueError`` for up-sampling, a factor that is not an
    integer, a native value of ``None``, ``mpp_x != mpp_y`` and ``level > 0``."""
    ratio = _resolution_ratio(resolution, units, mpp, power)
    resolution = float(resolution)
    k = round(ratio)
    if ratio < 1.0 and not _close(ratio, 1.0):
        msg = (f"reading at {resolution} {units} up-samples the slide (factor {ratio:.6g} < 1); only down-sampling by an "
               "integer factor is supported.")
        raise ValueError(msg)
    if not _close(ratio, float(k)):
        msg = (f"reading at {resolution} {units} down-samples by {ratio:.6g}, not an integer factor; only integer factors "
               "(cv2.INTER_AREA's box average) are supported.")
        raise ValueError(msg)
    return int(k)


def resolution_scale(resolution: float, units: str, *, mpp=None, power: float | None = None) -> float:
    """Down-sampling scale ``s >= 1`` (baseline pixels per pixel at ``(resolution, units)``), integer or not.

    The checks and messages of :func:`resolution_factor` except its integer check.  A ratio within ``_REL_TOL`` of an
    integer is returned as that integer (a ``float``), so that integer scales keep the integer read."""
    ratio = _resolution_ratio(resolution, units, mpp, power)
    if ratio < 1.0 and not _close(ratio, 1.0):
        msg = (f"reading at {float(resolution)} {units} up-samples the slide (factor {ratio:.6g} < 1); only down-sampling is "
               "supported.")
        raise ValueError(msg)
    k = round(ratio)
    return float(k) if _close(ratio, float(k)) else float(ratio)


def _u8_source(base: ArrayWSIReader) -> torch.Tensor:
    src = base.device_image if base.device_image.dim() == 3 else base.device_image[..., None]  # noqa: PLR2004
    if src.dtype == torch.bool:
        src = src.to(torch.uint8)
    if src.dtype != torch.uint8:
        msg = "device patch reads need a uint8 slide."
        raise TypeError(msg)
    return src.contiguous()


def _area_read(base: ArrayWSIReader, bounds, size: tuple[int, int], k: int, pad_value: int) -> torch.Tensor:
    """``[M, ph, pw, C]`` area reads of baseline ``bounds`` (an int32 ``[M, 4]`` device tensor, ``size=(pw, ph)``, extents
    ``k * size``): one ``tia_gather_area_patches_u8`` call."""
    from tiatoolbox_amd import _lib

    src = _u8_source(base)
    sh, sw, c = src.shape
    pw, ph = int(size[0]), int(size[1])
    out = torch.empty((len(bounds), ph, pw, c), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        rc = _lib.load().tia_gather_area_patches_u8(src.data_ptr(), sh, sw, c, bounds.data_ptr(), len(bounds), ph, pw, int(k),
                                                    int(pad_value), out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_gather_area_patches_u8")
    return out if base.device_image.dim() == 3 else out[..., 0]  # noqa: PLR2004


def _resize_read(symbol: str, base: ArrayWSIReader, bounds, extent: tuple[int, int], size: tuple[int, int],
                 pad_value: int) -> torch.Tensor:
    """``[M, ph, pw, C]`` reads of the ``extent=(wb, hb)`` baseline regions whose top-left corners are ``bounds[:, :2]`` (an
    int32 ``[M, 4]`` device tensor), each resampled to ``size=(pw, ph)``: one call of the entry point ``symbol``."""
    from tiatoolbox_amd import _lib

    src = _u8_source(base)
    sh, sw, c = src.shape
    wb, hb = int(extent[0]), int(extent[1])
    pw, ph = int(size[0]), int(size[1])
    out = torch.empty((len(bounds), ph, pw, c), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        rc = getattr(_lib.load(), symbol)(src.data_ptr(), sh, sw, c, bounds.data_ptr(), len(bounds), hb, wb, ph, pw,
                                          int(pad_value), out.data_ptr(), _lib.current_stream())
    _lib.check(rc, symbol)
    return out if base.device_image.dim() == 3 else out[..., 0]  # noqa: PLR2004


def _area_resize_read(base: ArrayWSIReader, bounds, extent: tuple[int, int], size: tuple[int, int], pad_value: int) -> torch.Tensor:
    """:func:`_resize_read` with ``cv2.INTER_AREA`` at any down-sampling ratio (``tia_gather_area_resize_u8``)."""
    return _resize_read("tia_gather_area_resize_u8", base, bounds, extent, size, pad_value)


def _cubic_resize_read(base: ArrayWSIReader, bounds, extent: tuple[int, int], size: tuple[int, int], pad_value: int) -> torch.Tensor:
    """:func:`_resize_read` with ``cv2.INTER_CUBIC`` at an up-sampling ratio (``tia_gather_cubic_resize_u8``)."""
    return _resize_read("tia_gather_cubic_resize_u8", base, bounds, extent, size, pad_value)


def _host_bounds(bounds) -> tuple[np.ndarray, tuple[int, int]]:
    bounds = np.ascontiguousarray(np.asarray(bounds).reshape(-1, 4), dtype=np.int32)
    sizes = np.unique(np.stack([bounds[:, 2] - bounds[:, 0], bounds[:, 3] - bounds[:, 1]], axis=1), axis=0)
    if len(sizes) != 1:
        msg = "read_bounds_batch expects regions of one size."
        raise ValueError(msg)
    pw, ph = int(sizes[0, 0]), int(sizes[0, 1])
    if pw <= 0 or ph <= 0:
        msg = f"empty region {pw} x {ph}."
        raise ValueError(msg)
    return bounds, (pw, ph)


class VirtualWSIReader(ArrayWSIReader):
    """ndarray-backed slide that also reads below its baseline resolution (reference ``VirtualWSIReader``).  Same constructor
    as :class:`ArrayWSIReader`, plus ``fractional``: ``False`` (the default) down-samples by an integer factor only,
    ``True`` by any ratio >= 1 (:func:`resolution_scale`); and ``upsample``: ``True`` also reads above the baseline
    resolution, by any ratio in ``[1/64, 1)`` (``cv2.INTER_CUBIC``), ``False`` (the default) refuses it.  The two flags are
    independent.  Without a resolution every read is the ``ArrayWSIReader`` read."""

    fractional = False
    upsample = False

    def __init__(self, img, mpp: float | None = 0.25, power: float | None = 40.0, mode: str = "rgb", *,
                 fractional: bool = False, upsample: bool = False) -> None:
        super().__init__(img, mpp=mpp, power=power, mode=mode)
        self.fractional = bool(fractional)
        self.upsample = bool(upsample)

    def factor(self, resolution: float, units: str) -> int:
        return resolution_factor(resolution, units, mpp=self.mpp, power=self.power)

    def scale(self, resolution: float, units: str) -> float:
        """Baseline pixels per pixel at ``(resolution, units)``: :func:`resolution_scale` for a fractional reader, else the
        integer :meth:`factor`.  An up-sampling reader returns a ratio ``s`` in ``[1/64, 1)`` where the others refuse to
        up-sample."""
        if self.upsample:
            ratio = _resolution_ratio(resolution, units, self.mpp, self.power)
            if ratio < 1.0 and not _close(ratio, 1.0):
                if ratio < 1.0 / _MAX_UPSAMPLE and not _close(ratio, 1.0 / _MAX_UPSAMPLE):
                    msg = (f"reading at {float(resolution)} {units} up-samples the slide by {1.0 / ratio:.6g}; at most "
                           f"{_MAX_UPSAMPLE} is supported.")
                    raise ValueError(msg)
                return float(ratio)
        if self.fractional:
            return resolution_scale(resolution, units, mpp=self.mpp, power=self.power)
        return self.factor(resolution, units)

    def at_resolution(self, resolution: float, units: str) -> ResampledWSIView:
        """The slide as seen at ``(resolution, units)``: a light view (no copy of the slide) whose reads take bounds in its
        own pixel space.  Logs a warning when the view up-samples the slide."""
        s = self.scale(resolution, units)
        if s < 1.0:
            logger.warning("Read: the desired resolution %s %s is higher than the WSI baseline (maximum) resolution; the "
                           "slide is up-sampled by %.6g.", resolution, units, 1.0 / s)
        return ResampledWSIView(self, s)

    def read_bounds(self, bounds, resolution: float | None = None, units: str | None = None, coord_space: str = "baseline",
                    pad_constant_values: int = 255) -> np.ndarray:
        """One region ``[x0, y0, x1, y1]`` (the subset of the reference's signature users call).  With ``resolution``:
        ``coord_space="resolution"`` takes the bounds at that resolution; ``"baseline"`` takes baseline bounds, whose extents
        must be multiples of the factor unless the reader is fractional or the read up-samples (then the region is resampled
        to ``np.round(extent / scale)``).  The output is the padded baseline region area-resampled (bicubic when up-sampled)
        to the resolution."""
        if coord_space not in ("baseline", "resolution"):
            msg = f"Invalid coord_space `{coord_space}`: expected 'baseline' or 'resolution'."
            raise ValueError(msg)
        if resolution is None:
            return self.read_bounds_batch(np.asarray(bounds)[None], pad_constant_values)[0].cpu().numpy()
        if units is None:
            msg = "read_bounds with a resolution needs its units."
            raise ValueError(msg)
        view = self.at_resolution(resolution, units)
        if coord_space == "resolution":
            return view.read_bounds(bounds, pad_constant_values)
        k = view.factor
        b, (w, h) = _host_bounds(bounds)
        bt = torch.from_numpy(b).to(self.device_image.device)
        if isinstance(k, int) and not (w % k or h % k):
            return _area_read(self, bt, (w // k, h // k), k, pad_constant_values)[0].cpu().numpy()
        if k < 1:
            return _cubic_resize_read(self, bt, (w, h), (int(np.round(w / k)), int(np.round(h / k))),
                                      pad_constant_values)[0].cpu().numpy()
        if not self.fractional:
            msg = f"a {w} x {h} baseline region does not shrink by the integer factor {k}."
            raise ValueError(msg)
        pw, ph = int(np.round(w / k)), int(np.round(h / k))
        if pw <= 0 or ph <= 0:
            msg = f"a {w} x {h} baseline region is empty at 1 / {k:.6g} of the baseline resolution."
            raise ValueError(msg)
        return _area_resize_read(self, bt, (w, h), (pw, ph), pad_constant_values)[0].cpu().numpy()


class ResampledWSIView:
    """A :class:`VirtualWSIReader` seen at ``1 / factor`` of its baseline resolution (``VirtualWSIReader.at_resolution``).

    ``factor`` is the scale ``s`` (baseline pixels per view pixel): an ``int`` when it is an integer, else a ``float``.
    ``slide_dimensions`` follow the reference's ``np.round(baseline / s)`` (``WSIReader._find_read_bounds_params``:
    ``output_size = np.round(...)``, which rounds halves to even); ``mpp`` / ``power`` are scaled by ``s``; reads take
    bounds in this view's pixels.  At an integer ``s`` they go through ``tia_gather_area_patches_u8``; otherwise the view
    region ``[x0, y0, x0 + pw, y0 + ph]`` reads the baseline region at ``(np.round(x0 * s), np.round(y0 * s))`` of extent
    ``(np.round(pw * s), np.round(ph * s))`` and resamples it to ``pw x ph`` (``tia_gather_area_resize_u8``; at ``s < 1``,
    an up-sampling reader's view, ``tia_gather_cubic_resize_u8``).  The tissue mask comes from the base reader (the
    reference computes it from baseline)."""

    def __init__(self, base: VirtualWSIReader, factor: float) -> None:
        self.base = base
        s = float(factor)
        self.factor = round(s) if _close(s, round(s)) else s
        self.mode = base.mode
        k = self.factor
        self.mpp = None if base.mpp is None else (base.mpp * k if np.ndim(base.mpp) == 0 else tuple(float(v) * k for v in np.ravel(base.mpp)))
        self.power = None if base.power is None else base.power / k

    @property
    def slide_dimensions(self) -> tuple[int, int]:
        w, h = self.base.slide_dimensions
        return int(np.round(w / self.factor)), int(np.round(h / self.factor))

    def read_bounds_batch(self, bounds, pad_value: int = 255, *, size: tuple[int, int] | None = None) -> torch.Tensor:
        """``[M, ph, pw, C]`` regions ``[x0, y0, x1, y1]`` in this view's pixels, ``pad_value`` outside the slide.  ``bounds`` may
        be an int32 ``[M, 4]`` device tensor together with ``size=(pw, ph)``, as for ``ArrayWSIReader.read_bounds_batch``."""
        k = self.factor
        if isinstance(bounds, torch.Tensor) and bounds.is_cuda:
            if size is None or bounds.dtype != torch.int32 or bounds.dim() != 2 or bounds.shape[1] != 4 or not bounds.is_contiguous():  # noqa: PLR2004
                msg = "device bounds: a contiguous int32 [M, 4] tensor together with size=(pw, ph)."
                raise ValueError(msg)
            if isinstance(k, int):
                return _area_read(self.base, bounds * k if k != 1 else bounds, size, k, pad_value)
            top_left = torch.round(bounds[:, :2].double() * k).to(torch.int32)
        else:
            b, size = _host_bounds(bounds)
            if isinstance(k, int):
                bt = torch.from_numpy(b * np.int32(k)).to(self.base.device_image.device)
                return _area_read(self.base, bt, size, k, pad_value)
            top_left = torch.from_numpy(np.round(b[:, :2] * k).astype(np.int32)).to(self.base.device_image.device)
        pw, ph = int(size[0]), int(size[1])
        extent = (int(np.round(pw * k)), int(np.round(ph * k)))
        if extent[0] <= 0 or extent[1] <= 0:
            msg = f"a {pw} x {ph} region is empty at the baseline: its extent rounds to {extent[0]} x {extent[1]} at scale {k:.6g}."
            raise ValueError(msg)
        bt = torch.cat([top_left, top_left + torch.tensor(extent, dtype=torch.int32, device=top_left.device)], dim=1).contiguous()
        read = _cubic_resize_read if k < 1 else _area_resize_read
        return read(self.base, bt, extent, (pw, ph), pad_value)

    def read_bounds(self, bounds, pad_value: int = 255) -> np.ndarray:
        return self.read_bounds_batch(np.asarray(bounds)[None], pad_value)[0].cpu().numpy()

    def slide_thumbnail(self, resolution: float = 1.25, units: str = "power") -> torch.Tensor:
        return self.base.slide_thumbnail(resolution, units)

    def tissue_mask(self, method: str = "otsu", resolution: float = 1.25, units: str = "power", **masker_kwargs):
        return self.base.tissue_mask(method, resolution, units, **masker_kwargs)

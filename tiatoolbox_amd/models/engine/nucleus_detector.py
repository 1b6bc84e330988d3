"""Nucleus detection engine (API of reference ``tiatoolbox/models/engine/nucleus_detector.py``, for the covered path).

A detection model emits probability maps; its detections are the maps' local maxima -- ``peak_local_max``, which the reference's
detection models call in ``postproc``.  This engine takes ANY :class:`~tiatoolbox_amd.models.models_abc.ModelABC` whose
``infer_batch`` returns ``[N, h, w, C]`` (or ``[N, h, w]``) float32 maps, runs it as :class:`SemanticSegmentor` does and detects on
the device (``utils/peaks.py``, ``csrc/peaks.hip``); ``utils/_peaks.py`` states the result.  The zoo's detection architectures
(MapDe, SCCNN, MicroNet) are NOT registered here: bring the model.

Run kwargs, decided per call: ``min_distance`` and ``threshold_abs`` (default: the model's attributes of those names if it has
them, else 1 and ``None``), ``threshold_rel``, ``exclude_border=False``, ``num_peaks`` (per map), ``detection_channels=None`` (all
output channels; else the channel indices to detect on, in the order given).

Patch mode returns flat arrays ordered by patch, then channel (in ``detection_channels`` order), then the statement's order:
``coordinates`` ``[K, 2]`` int64 as ``(x, y)`` in the patch's output map, ``classes`` ``[K]`` int64 (the channel index),
``probabilities`` ``[K]`` float32 (the map's value at the peak) and ``patch_index`` ``[K]`` int64.  WSI mode stitches the probability
canvas on the device as :class:`SemanticSegmentor` does, detects per channel on the whole canvas and writes ``coordinates`` (canvas
pixels), ``classes`` and ``probabilities`` into the slide's ``.npz``.  A slide whose canvas would stream to the host
(``CanvasBand``) is refused with a ``ValueError`` that names ``memory_threshold``: banded detection is out of scope.
"""

from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from tiatoolbox_amd.models.engine.semantic_segmentor import SemanticSegmentor
from tiatoolbox_amd.utils import peaks

_UNSET = object()
_OPTIONS = ("min_distance", "threshold_abs", "threshold_rel", "exclude_border", "num_peaks", "detection_channels")


class NucleusDetector(SemanticSegmentor):
    """Detections = ``peak_local_max`` of a model's probability maps, in patch and WSI mode."""

    resident_canvas_only = True  # infer_wsi refuses a canvas that would stream to the host, before it infers the slide

    def _update_run_params(self, images, **kwargs):
        given = {k: kwargs.pop(k, _UNSET) for k in _OPTIONS}
        self._detection = self._checked_detection(given)  # refused before anything of the call is taken over
        out = super()._update_run_params(images, **kwargs)
        # "probabilities" are the peaks' values here and always returned; the maps themselves are not an output of this engine
        self.drop_keys = [k for k in self.drop_keys if k != "probabilities"]
        return out

    def _checked_detection(self, given: dict) -> dict:
        model = self.model.module if hasattr(self.model, "module") else self.model
        opts = {"min_distance": getattr(model, "min_distance", 1), "threshold_abs": getattr(model, "threshold_abs", None),
                "threshold_rel": None, "exclude_border": False, "num_peaks": np.inf, "detection_channels": None}
        opts.update({k: v for k, v in given.items() if v is not _UNSET})
        if opts["num_peaks"] is None:
            opts["num_peaks"] = np.inf
        peaks._checked_options(opts["min_distance"], opts["exclude_border"], opts["num_peaks"])  # noqa: SLF001
        for name in ("threshold_abs", "threshold_rel"):
            v = opts[name]
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or np.isnan(v)):
                msg = f"`{name}` must be a real number or None, got {v!r}."
                raise ValueError(msg)
        ch = opts["detection_channels"]
        if ch is not None:
            ch = [ch] if isinstance(ch, (int, np.integer)) and not isinstance(ch, bool) else list(ch)
            if not ch or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0 for c in ch):
                msg = f"`detection_channels` must be None or channel indices >= 0, got {opts['detection_channels']!r}."
                raise ValueError(msg)
            opts["detection_channels"] = [int(c) for c in ch]
        return opts

    def _detect(self, maps: torch.Tensor) -> dict:
        """``maps`` ``[N, C, h, w]`` float32 on any device -> the flat detection arrays (tensors on that device)."""
        opts = self._detection
        n_ch = int(maps.shape[1])
        channels = opts["detection_channels"] if opts["detection_channels"] is not None else list(range(n_ch))
        if any(c >= n_ch for c in channels):
            msg = f"`detection_channels` {channels} names a channel the model does not emit: its maps have {n_ch}."
            raise ValueError(msg)
        planes = maps[:, channels].reshape(-1, maps.shape[2], maps.shape[3]).contiguous()
        coords, values, counts = peaks.peak_local_max_planes(
            planes, opts["min_distance"], opts["threshold_abs"], opts["threshold_rel"], opts["exclude_border"], opts["num_peaks"])
        dev = coords.device
        per_plane = torch.as_tensor(counts, dtype=torch.int64, device=dev)
        plane = torch.repeat_interleave(torch.arange(len(counts), device=dev), per_plane, output_size=int(coords.shape[0]))
        return {"coordinates": coords.flip(1).contiguous(),  # (row, col) -> (x, y)
                "classes": torch.as_tensor(channels, dtype=torch.int64, device=dev)[plane % len(channels)],
                "probabilities": values, "patch_index": plane // len(channels)}

    @staticmethod
    def _as_maps(probs) -> torch.Tensor:
        if isinstance(probs, (tuple, list)):
            msg = "NucleusDetector needs a model with ONE output head of probability maps; this one returns several."
            raise ValueError(msg)  # noqa: TRY004
        probs = probs if isinstance(probs, torch.Tensor) else torch.from_numpy(np.asarray(probs))
        if probs.ndim == 3:  # noqa: PLR2004  [N, h, w]: one channel
            probs = probs[..., None]
        if probs.ndim != 4:  # noqa: PLR2004
            msg = f"NucleusDetector needs probability maps [N, h, w, C] from the model, got {tuple(probs.shape)}."
            raise ValueError(msg)
        return probs.to(torch.float32).permute(0, 3, 1, 2)

    def post_process_patches(self, raw_predictions: dict, **_) -> dict:
        out = {k: v for k, v in raw_predictions.items() if k != "probabilities"}
        out.update(self._detect(self._as_maps(raw_predictions["probabilities"])))
        return out

    def run(self, images, *, masks=None, input_resolutions=None, patch_input_shape=None, ioconfig=None,
            patch_mode: bool = True, save_dir=None, overwrite: bool = False, output_type: str = "dict", **kwargs):
        """Patch mode: the flat detection arrays.  WSI mode: per slide one ``<stem>.npz`` with ``coordinates``, ``classes`` and
        ``probabilities``; returns ``{image key: Path}``."""
        if patch_mode:
            return super().run(images, masks=masks, input_resolutions=input_resolutions, patch_input_shape=patch_input_shape,
                               ioconfig=ioconfig, patch_mode=True, save_dir=save_dir, overwrite=overwrite, output_type=output_type,
                               **kwargs)
        self._update_run_params(images=images, masks=masks, input_resolutions=input_resolutions,
                                patch_input_shape=patch_input_shape, save_dir=save_dir, ioconfig=ioconfig,
                                output_type=output_type, overwrite=overwrite, patch_mode=False, **kwargs)
        from tiatoolbox_amd.models.engine.engine_abc import prepare_engines_save_dir, write_outputs

        save_dir = prepare_engines_save_dir(save_dir, patch_mode=False, overwrite=overwrite, distributed=self.distributed)
        paths: dict = {}
        for i, image in enumerate(self.images):
            base = self._open_slide(image)
            mask_reader = None
            if self.masks is not None:
                mask_reader = self._open_slide(self.masks[i], as_mask=True)
            elif self.auto_get_mask:
                mask_reader = base.tissue_mask(resolution=1.25, units="power")
            reader = self._reader_at_input_resolution(base)
            arrays = {k: v.cpu().numpy() for k, v in self.detect_wsi(reader, mask_reader).items()}
            key = image if isinstance(image, (str, Path)) else i
            stem = Path(image).stem if isinstance(image, (str, Path)) else str(i)
            paths[key] = save_dir / f"{stem}.npz"
            write_outputs(self.distributed, lambda path=paths[key], arrays=arrays: np.savez(path, **arrays))
        return paths

    predict = run

    def detect_wsi(self, reader, mask_reader=None) -> dict:
        """The in-memory form of WSI mode: ``coordinates`` ``(x, y)`` in canvas pixels, ``classes`` and ``probabilities`` of one
        slide as device tensors, with the options of the last ``run`` (the defaults before any)."""
        if not hasattr(self, "_detection"):
            self._detection = self._checked_detection({})
        out = self.infer_wsi(reader, mask_reader, return_probabilities=True)
        canvas = out["probabilities"]  # [H, W, C] on the device: a streamed canvas was refused inside infer_wsi
        found = self._detect(canvas.permute(2, 0, 1)[None])
        del found["patch_index"]
        return found

"""Patch classification engine (API of reference ``tiatoolbox/models/engine/patch_predictor.py``)."""

from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from tiatoolbox_amd.models.engine import _attention_merge, _patch_merge
from tiatoolbox_amd.models.engine.engine_abc import EngineABC, open_slide
from tiatoolbox_amd.utils.misc import cast_to_min_dtype


class PatchPredictor(EngineABC):
    """Patch-level prediction: ``probabilities`` (optional) + ``predictions`` (ref. :88-679).

    Extra run-time kwargs on MI355X: ``compute_dtype`` ("float32" | "float16" | "bfloat16"; for Vision Transformer models on a CUDA
    device also "float8_e4m3": the bfloat16 graph with the qkv / fc1 / fc2 Linear layers on the FP8 GEMM, "int8": the same layers on the
    INT8 GEMM (W8A8, one scale per token and per output channel; closer than FP8 on activations without outlier channels, worse with
    one -- compare both with "bfloat16" on your own checkpoint; not beside ``residual_dtype``), and "bfloat16x3": the same
    graph in float32 with every Linear on the split-bf16 GEMM and attention on the float32 MFMA kernel; a ``ValueError`` elsewhere),
    ``residual_dtype`` (``None`` | "float32": Vision Transformer models on a CUDA device in "float16" / "bfloat16" keep their residual
    stream in float32, as the float32 module under ``torch.autocast`` does; a ``ValueError`` elsewhere), ``int8_smoothing`` (alpha in
    (0, 1]) with ``int8_calibration`` (patches as a run takes them, or a scales dict of ``calibrate_int8_smoothing`` /
    ``engine.int8_smoothing_scales``): per-input-channel smoothing of the INT8 layers beside "int8" only, calibrated once when the
    inference copy is built, for checkpoints with outlier channels -- unmeasured on real ones; a ``ValueError`` in every other
    combination), ``return_attention`` (``None`` | "class" | "rollout", patch mode, models whose ``feat_extract`` is a
    ``VisionTransformer``, every ``compute_dtype`` but "bfloat16x3"; decided per call like ``return_probabilities``: the result gets an
    ``"attention"`` key, float32, one map per patch on the patch grid -- "class" ``[N, heads, gh, gw]``, the class token's attention
    in the last block per head, NOT renormalised: a map sums to 1 minus the mass on the class and register tokens; "rollout"
    ``[N, gh, gw]``, attention rollout with mean head fusion -- while every other key is bit for bit that of the run without it;
    ``VisionTransformer.forward_with_attention`` states both; a ``ValueError`` elsewhere) and ``stain_normalizer`` (a fitted :class:`~tiatoolbox_amd.tools.stainnorm.StainNormalizer`; shorthand
    for ``model.preproc_func = StainNormPreproc(normalizer, default_preproc)``).

    WSI mode (``patch_mode=False``) also takes ``merge_predictions=True`` with ``merge_resolution`` (default 1.25) and
    ``merge_units`` (default ``"power"``): every slide's ``.npz`` then also holds ``merged_predictions``, the tissue-type map of
    :meth:`merge_predictions` at that resolution, and -- with ``return_probabilities=True`` -- ``merged_probabilities``, its raw
    map.  The per-patch probabilities are merged where ``infer_wsi`` left them, in HBM.  The three options are decided per
    call, like ``return_probabilities``; without the flag the files hold ``predictions``, ``coordinates`` and, on request,
    ``probabilities`` only.

    WSI mode also takes ``merge_attention`` (``None`` | "class" | "rollout"; what ``return_attention`` covers, with ``patch_mode=False``
    required -- ``return_attention`` itself stays a patch-mode option) with ``attention_interpolation`` ("bilinear" | "nearest") and the
    same ``merge_resolution`` / ``merge_units``: every slide's ``.npz`` then also holds ``attention`` (the per-patch maps, as
    ``return_attention`` returns them), ``merged_attention`` (:meth:`merge_attention` of them: ``[heads, H, W]`` or ``[H, W]`` float32) and
    ``attention_coverage`` (``[H, W]`` int32, the number of patches over each pixel).  The maps never leave HBM before the merge.  It may
    be combined with ``merge_predictions=True``; a ``ValueError`` before any launch where it does not apply.

    Rollout maps -- ``return_attention="rollout"`` in patch mode, ``merge_attention="rollout"`` in WSI mode, where the per-patch
    ``attention`` and the ``merged_attention`` built from it both follow -- also take ``attention_head_fusion`` ("mean" | "max" | "min",
    default "mean") and ``attention_discard_ratio`` (``0 <= r < 1``, default 0): the heads' maximum or minimum in place of their mean,
    and per block the ``min(int(r S^2), S^2 - 1)`` smallest entries of the fused ``S x S`` matrix set to 0 (ties with the last one
    included, entry (0, 0) never) before ``(F' + I) / 2`` is normalised by rows and multiplied into the rollout;
    ``engine/_rollout_options.py`` states the arithmetic.  Decided per call and never attributes; with the defaults the maps are bit for
    bit those of a call without the two kwargs.  A ``ValueError`` that names the option for a non-default value without a rollout
    request (beside "class" too), a fusion outside the three names, a ratio that is no real number in ``[0, 1)``.

    ``return_cam=True`` (patch mode; a ``bool`` decided per call, never an attribute) is the heat map of the ``CNNModel`` classifiers
    -- the ResNet, ResNeXt and Wide-ResNet kather100k models: the result gains ``"cam"``, float32 ``[N, K, h, w]`` on the trunk's output
    grid (7 x 7 at 224 x 224, 8 x 8 at 256 x 256), ``cam[n, k, y, x] = sum_c W[k, c] F[n, c, y, x]`` with ``F`` the feature map of the
    forward that ran and ``W`` the classifier weights of the inference copy (``engine/_cam.py`` states it): no bias, no ReLU, nothing
    renormalised, ``mean(cam) + b`` is the logit.  Raw logit contributions: comparable across classes within a patch, across patches
    only as logits are.  Every other key is bit for bit that of the run without it; on a CUDA device (``compute_dtype`` "float32",
    "float16", "bfloat16") one ``tia_cam_nhwc_f32`` / ``tia_cam_nhwc_h`` launch per batch is all that is added.  ``merge_cam=True``
    (WSI mode, with ``cam_interpolation`` "bilinear" | "nearest" and ``merge_resolution`` / ``merge_units``; may be combined with
    ``merge_predictions=True``): every slide's ``.npz`` also holds ``cam`` (the per-patch maps, as ``return_cam`` returns them),
    ``merged_cam`` (:meth:`merge_cam` of them, ``[K, H, W]`` float32) and ``cam_coverage`` (``[H, W]`` int32).  A ``ValueError`` before
    any launch that names the option for anything else: a ``TimmModel`` (``return_attention`` gives its maps), a feature extractor
    (no classifier), any other model class, the wrong ``patch_mode``, an unknown interpolation, a value that is no ``bool``.
    """

    def __init__(self, model, batch_size: int = 8, num_workers: int = 0, weights=None, *,
                 device: str = "cpu", verbose: bool = True) -> None:
        super().__init__(model=model, batch_size=batch_size, num_workers=num_workers, weights=weights,
                         device=device, verbose=verbose)
        self.return_probabilities = False
        self.stain_normalizer = None
        self._default_preproc = self._get_model_attr("preproc_func")

    def _update_run_params(self, images, **kwargs):
        """ref. :448-549: ``probabilities`` are dropped unless THIS call passes ``return_probabilities=True`` (ref. :535-537:
        ``kwargs.get("return_probabilities")`` -- per call, not sticky)."""
        # the merge options are this call's alone and never become attributes (``self.merge_predictions`` is the static method)
        self._merge_on = bool(kwargs.pop("merge_predictions", False))
        self._merge_resolution = kwargs.pop("merge_resolution", 1.25)
        self._merge_units = kwargs.pop("merge_units", "power")
        self._merge_attention = None
        attention_kind = kwargs.pop("merge_attention", None)
        self._attention_interpolation = kwargs.pop("attention_interpolation", "bilinear")
        # refused before anything of this call is taken over: the compute_dtype is the call's, else the one earlier runs left behind
        self._merge_attention = self._checked_merge_attention(
            attention_kind, self._attention_interpolation, patch_mode=bool(kwargs.get("patch_mode")),
            compute_dtype=kwargs.get("compute_dtype", getattr(self, "compute_dtype", "float32")))
        # return_cam / merge_cam / cam_interpolation likewise: this call's alone, refused before anything of the call is taken over
        self._return_cam = self._merge_cam = False
        return_cam, merge_cam = kwargs.pop("return_cam", False), kwargs.pop("merge_cam", False)
        self._cam_interpolation = "bilinear"
        cam_interpolation = kwargs.pop("cam_interpolation", "bilinear")
        self._return_cam = self._checked_cam("return_cam", return_cam, patch_mode=bool(kwargs.get("patch_mode")))
        self._merge_cam = self._checked_cam("merge_cam", merge_cam, patch_mode=bool(kwargs.get("patch_mode")),
                                            interpolation=cam_interpolation)
        self._cam_interpolation = cam_interpolation
        out = super()._update_run_params(images, **kwargs)
        if not self.return_probabilities:
            self.drop_keys.append("probabilities")
        elif "probabilities" in self.drop_keys:
            self.drop_keys = [k for k in self.drop_keys if k != "probabilities"]
        from tiatoolbox_amd.models.dataset.classification import StainNormPreproc

        model = self.model.module if hasattr(self.model, "module") else self.model
        if self.stain_normalizer is not None:
            model.preproc_func = StainNormPreproc(self.stain_normalizer, self._default_preproc)
        elif isinstance(model.preproc_func, StainNormPreproc) and getattr(self, "_installed_norm", False):
            model.preproc_func = self._default_preproc  # a later run(stain_normalizer=None) undoes the shorthand
        self._installed_norm = self.stain_normalizer is not None
        return out

    def post_process_patches(self, raw_predictions: dict, **_) -> dict:
        """``predictions = cast_to_min_dtype(argmax(probabilities))`` (ref. :321-380)."""
        postproc_func = self._get_model_attr("postproc_func")
        probs = raw_predictions["probabilities"]
        predictions = postproc_func(probs)
        if isinstance(predictions, torch.Tensor) and predictions.numel() == 0:
            raw_predictions["predictions"] = predictions.to(torch.uint8)
        else:
            raw_predictions["predictions"] = cast_to_min_dtype(predictions)
        return raw_predictions

    def post_process_wsi(self, processed: dict, *, base, reader) -> dict:
        """``merge_predictions=True``: the slide's patch rows merged into ``merged_predictions`` (and ``merged_probabilities``
        with ``return_probabilities``) at ``merge_resolution`` / ``merge_units``.  The patch space is that of ``reader``, the
        reader the grid was made on; the canvas is the slide ``base`` at the merge resolution.  Under ``torch.distributed``
        every rank holds all rows after the all-gather and merges them; rank 0 writes.  ``merge_attention=...``: the slide's
        per-patch maps, where ``infer_wsi`` left them, merged into ``merged_attention`` and ``attention_coverage`` on the same canvas.
        ``merge_cam=True``: the same merge of the class activation maps into ``merged_cam`` and ``cam_coverage``."""
        merge_on, attention_on = getattr(self, "_merge_on", False), getattr(self, "_merge_attention", None) is not None
        cam_on = bool(getattr(self, "_merge_cam", False))
        if not (merge_on or attention_on or cam_on):
            return processed
        from tiatoolbox_amd.wsicore import _resolution_ratio

        ratio = _resolution_ratio(self._merge_resolution, self._merge_units, base.mpp, base.power)
        canvas_wh = _patch_merge.canvas_size(base.slide_dimensions, ratio)
        if merge_on:
            merged = _merge_output(processed, reader.slide_dimensions, canvas_wh, want_raw=bool(self.return_probabilities))
            processed["merged_predictions"] = merged["labels"]
            if self.return_probabilities:
                processed["merged_probabilities"] = merged["raw"]
        if attention_on:
            merged = _merge_attention_output(processed, reader.slide_dimensions, canvas_wh, self._attention_interpolation)
            processed["merged_attention"], processed["attention_coverage"] = merged["raw"], merged["count"]
        if cam_on:
            merged = _merge_attention_output(processed, reader.slide_dimensions, canvas_wh, self._cam_interpolation, key="cam")
            processed["merged_cam"], processed["cam_coverage"] = merged["raw"], merged["count"]
        return processed

    @staticmethod
    def merge_attention(img, output, resolution: float = 1.25, units: str = "power", interpolation: str = "bilinear",
                        return_count: bool = False):  # noqa: FBT001, FBT002  (a sibling of merge_predictions)
        """Merge the per-patch attention maps of a run into a heat map of the slide at ``(resolution, units)``.

        ``img``: the slide, as :meth:`merge_predictions` takes it.  ``output``: a ``dict`` or the path of an ``.npz`` with
        ``coordinates`` ``[N, 4]``, ``attention`` (``[N, heads, gh, gw]`` of ``"class"`` or ``[N, gh, gw]`` of ``"rollout"``), plus
        ``resolution`` and ``units``: the resolution the patches were read at (their coordinates' pixel space).

        Canvas, patch space and coverage are those of :meth:`merge_predictions`.  Every covered pixel samples each covering patch's grid
        at its own centre (``align_corners=False``; ``interpolation``: "bilinear" or "nearest"), the samples are summed in float32 in
        patch order and divided by the coverage count (``+ 1e-8``, in float64); ``engine/_attention_merge.py`` states every operation.
        Nothing is renormalised: "class" maps are relative within a patch (each sums to 1 minus the mass on the class and register
        tokens), so the slide map compares patches only loosely; "rollout" rows are comparable in the same loose sense.

        Returns ``[heads, H, W]`` or ``[H, W]`` float32 of the kind of ``attention`` (0 where nothing covers); with
        ``return_count=True`` the pair ``(map, coverage [H, W] int32)``.  CUDA maps are merged on their device by
        ``tia_merge_patch_grids_f32`` and never visit the host."""
        return _merge_maps_of(img, output, "attention", "merge_attention", resolution, units, interpolation, return_count=return_count)

    @staticmethod
    def merge_cam(img, output, resolution: float = 1.25, units: str = "power", interpolation: str = "bilinear",
                  return_count: bool = False):  # noqa: FBT001, FBT002  (a sibling of merge_attention)
        """Merge the per-patch class activation maps of a run into a heat map of the slide at ``(resolution, units)``.

        ``img``: the slide, as :meth:`merge_predictions` takes it.  ``output``: a ``dict`` or the path of an ``.npz`` with
        ``coordinates`` ``[N, 4]``, ``cam`` ``[N, K, h, w]`` (what ``return_cam=True`` / ``merge_cam=True`` return), plus ``resolution``
        and ``units``: the resolution the patches were read at (their coordinates' pixel space).

        Canvas, patch space, coverage, sampling and averaging are those of :meth:`merge_attention`
        (``engine/_attention_merge.py`` states every operation).  Nothing is renormalised: the values are raw logit contributions
        (``engine/_cam.py``), comparable across classes within a patch and across patches only as logits are.

        Returns ``[K, H, W]`` float32 (0 where nothing covers); with ``return_count=True`` the pair ``(map, coverage [H, W] int32)``.
        CUDA maps are merged on their device by ``tia_merge_patch_grids_f32`` and never visit the host."""
        return _merge_maps_of(img, output, "cam", "merge_cam", resolution, units, interpolation, return_count=return_count)

    @staticmethod
    def merge_predictions(img, output, resolution: float = 1.25, units: str = "power", postproc_func=None,
                          return_raw: bool = False):  # noqa: FBT001, FBT002  (the reference's signature)
        """Merge the per-patch results of a WSI-mode run into a 2-D tissue-type map of the slide at ``(resolution, units)``
        (the reference's ``PatchPredictor.merge_predictions``).

        ``img``: the slide -- an ``ArrayWSIReader`` / ``VirtualWSIReader``, an array / tensor or a ``.npy`` path, as ``run()``
        takes them.  ``output``: a ``dict`` or the path of a WSI-mode ``.npz`` with ``coordinates`` ``[N, 4]`` and
        ``probabilities`` ``[N, C]`` and / or ``predictions`` ``[N]``, plus ``resolution`` and ``units``: the resolution the
        patches were read at (their coordinates' pixel space), which the files do not record themselves.

        Canvas and patch space measure ``np.round(slide_dimensions / s)`` pixels, ``s`` the down-sampling ratio from the slide's
        baseline (any positive ratio, up-sampling included).  Patch ``i`` covers the map rectangle ``ceil((x0, x1) * fx)`` x
        ``ceil((y0, y1) * fy)`` clipped to the canvas, ``fx = W / Ws``, ``fy = H / Hs`` (the reference multiplies the (x, y)
        bounds by a (y, x) factor; the two differ on non-proportional canvases only, and this method uses ``fx`` for x and
        ``fy`` for y).  Overlapping patches are averaged: the probabilities are summed in float32 in patch order and divided by
        the coverage count (``+ 1e-8``, in float64).

        Returns ``[H, W]`` labels: ``1 + argmax`` of the summed probabilities where a patch covers the pixel, 0 elsewhere
        (``uint8`` up to 254 classes, else ``int32``).  ``postproc_func`` replaces the argmax: it gets the raw map ``[H, W, C]``
        (a tensor or an array, as ``probabilities`` is) and returns ``[H, W]`` integers; 1 is added where a patch covers the pixel.
        ``return_raw=True`` returns the raw ``[H, W, C]`` float32 map instead (0 where nothing covers).  Without
        ``probabilities`` the map is the float32 sum of ``predictions + 1`` over the covering patches -- overlapping patches ADD,
        as in the reference, so pass probabilities for overlapping strides -- and ``return_raw=True`` is a ``ValueError``.
        CUDA probabilities are merged on their device by ``tia_merge_patch_rects_f32``; the result is of their kind."""
        if isinstance(output, (str, Path)):
            with np.load(output) as data:
                output = {k: data[k] for k in data.files}
        missing = [k for k in ("resolution", "units") if k not in output]
        if missing:
            msg = (f"`output` lacks {missing}: merge_predictions needs output['resolution'] and output['units'], the resolution "
                   "the patch coordinates are in (ioconfig.input_resolutions[0]).")
            raise ValueError(msg)
        if "coordinates" not in output or not ("probabilities" in output or "predictions" in output):
            msg = "`output` needs 'coordinates' and 'probabilities' and / or 'predictions'."
            raise ValueError(msg)
        from tiatoolbox_amd.wsicore import _resolution_ratio

        reader = img if hasattr(img, "slide_dimensions") else open_slide(img)
        dims = reader.slide_dimensions
        patch_units = output["units"]
        patch_units = patch_units.item() if isinstance(patch_units, np.ndarray) else patch_units
        patch_wh = _patch_merge.canvas_size(dims, _resolution_ratio(float(np.asarray(output["resolution"])), str(patch_units),
                                                                    reader.mpp, reader.power))
        canvas_wh = _patch_merge.canvas_size(dims, _resolution_ratio(resolution, units, reader.mpp, reader.power))
        if "probabilities" not in output and return_raw:
            msg = "return_raw=True needs output['probabilities']; this output holds predictions only."
            raise ValueError(msg)
        merged = _merge_output(output, patch_wh, canvas_wh, want_raw=return_raw or postproc_func is not None,
                               want_count=postproc_func is not None)
        if "probabilities" not in output:
            return merged["sum"][..., 0]
        if return_raw:
            return merged["raw"]
        if postproc_func is None:
            return merged["labels"]
        labels, covered = postproc_func(merged["raw"]), merged["count"] > 0
        if isinstance(labels, torch.Tensor):
            return labels + covered.to(labels.dtype)
        return np.asarray(labels) + np.asarray(covered.cpu() if isinstance(covered, torch.Tensor) else covered).astype(np.asarray(labels).dtype)


def _merge_output(output: dict, patch_wh, canvas_wh, *, want_raw: bool = False, want_count: bool = False) -> dict:
    """The outputs of :func:`_patch_merge.merge_patch_rects` for one slide's ``coordinates`` + ``probabilities`` (``labels``,
    ``raw`` / ``count`` on request) or, without probabilities, ``predictions`` (``sum`` of ``predictions + 1``, one channel)."""
    w, h = int(canvas_wh[0]), int(canvas_wh[1])
    if min(w, h, int(patch_wh[0]), int(patch_wh[1])) <= 0:
        msg = (f"the merged map ({w} x {h}) or the patch space ({patch_wh[0]} x {patch_wh[1]}) has a zero dimension at the "
               "requested resolution.")
        raise ValueError(msg)
    rects = _patch_merge.patch_rects(output["coordinates"], patch_wh, (h, w))
    if "probabilities" in output:
        values = output["probabilities"]
        values = values if isinstance(values, torch.Tensor) else np.asarray(values, dtype=np.float32)
        want = ("labels", *(("raw",) if want_raw else ()), *(("count",) if want_count else ()))
        return _patch_merge.merge_patch_rects(rects, values.reshape(len(rects), -1), (h, w), want=want)
    preds = output["predictions"]
    if isinstance(preds, torch.Tensor):
        values = (preds.reshape(-1, 1) + 1).to(torch.float32)
    else:
        values = (np.asarray(preds).reshape(-1, 1).astype(np.int64) + 1).astype(np.float32)
    return _patch_merge.merge_patch_rects(rects, values, (h, w), want=("sum",))


def _merge_maps_of(img, output, key: str, who: str, resolution, units, interpolation: str, *, return_count: bool):
    """The static ``merge_attention`` / ``merge_cam``: the maps ``output[key]`` of a dict or an ``.npz`` merged on the canvas of
    ``img`` at ``(resolution, units)``."""
    if isinstance(output, (str, Path)):
        with np.load(output) as data:
            output = {k: data[k] for k in data.files}
    missing = [k for k in ("resolution", "units") if k not in output]
    if missing:
        msg = (f"`output` lacks {missing}: {who} needs output['resolution'] and output['units'], the resolution "
               "the patch coordinates are in (ioconfig.input_resolutions[0]).")
        raise ValueError(msg)
    if "coordinates" not in output or key not in output:
        msg = f"`output` needs 'coordinates' and '{key}'."
        raise ValueError(msg)
    from tiatoolbox_amd.wsicore import _resolution_ratio

    reader = img if hasattr(img, "slide_dimensions") else open_slide(img)
    dims = reader.slide_dimensions
    patch_units = output["units"]
    patch_units = patch_units.item() if isinstance(patch_units, np.ndarray) else patch_units
    patch_wh = _patch_merge.canvas_size(dims, _resolution_ratio(float(np.asarray(output["resolution"])), str(patch_units),
                                                                reader.mpp, reader.power))
    canvas_wh = _patch_merge.canvas_size(dims, _resolution_ratio(resolution, units, reader.mpp, reader.power))
    merged = _merge_attention_output(output, patch_wh, canvas_wh, interpolation, key=key)
    return (merged["raw"], merged["count"]) if return_count else merged["raw"]


def _merge_attention_output(output: dict, patch_wh, canvas_wh, interpolation: str, *, key: str = "attention") -> dict:
    """``raw`` and ``count`` of :func:`_attention_merge.merge_patch_grids` for one slide's ``coordinates`` + ``attention`` (or the maps
    under another ``key``: ``cam``)."""
    w, h = int(canvas_wh[0]), int(canvas_wh[1])
    if min(w, h, int(patch_wh[0]), int(patch_wh[1])) <= 0:
        msg = (f"the merged map ({w} x {h}) or the patch space ({patch_wh[0]} x {patch_wh[1]}) has a zero dimension at the "
               "requested resolution.")
        raise ValueError(msg)
    maps = output[key]
    maps = maps if isinstance(maps, torch.Tensor) else np.asarray(maps, dtype=np.float32)
    return _attention_merge.merge_patch_grids(output["coordinates"], maps, patch_wh, (h, w), interpolation=interpolation,
                                              want=("raw", "count"))

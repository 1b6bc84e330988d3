"""Deep feature extraction engine (API of reference ``tiatoolbox/models/engine/deep_feature_extractor.py``).

Same inference path as :class:`PatchPredictor` (device-resident batches, BN-folded trunk, the hand-written MFMA
convolutions for float32 BasicBlock trunks); what differs is the tail: the model's output (``CNNBackbone``: the pooled
feature vector) is returned untouched under ``"probabilities"`` -- no arg-max, no ``"predictions"`` key -- together with
``"coordinates"`` in WSI mode (ref. :70-141 constructor, :142-260 ``infer_wsi``, :262-290 ``post_process_patches``).
The reference spills feature chunks to zarr when host memory runs short; here features of a run stay in one device
tensor until they are copied out (a 100k-patch slide of 2048-d float32 features is 0.8 GB of 288 GB).
"""

from __future__ import annotations

from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor


class DeepFeatureExtractor(PatchPredictor):
    """Patch / WSI feature extractor: ``run()`` returns ``{"probabilities": features[, "coordinates"]}``.

    The run kwargs are :class:`PatchPredictor`'s.  ``compute_dtype``: "float32" | "float16" | "bfloat16"; for Vision Transformer backbones
    on a CUDA device also "float8_e4m3" (the bfloat16 graph with the qkv / fc1 / fc2 Linear layers on the FP8 GEMM), "int8" (the same
    layers on the INT8 GEMM: W8A8 with one scale per token and per output channel; closer to float32 than FP8 where the activations
    have no outlier channel, further where they have one, and unmeasured on real checkpoints: compare "int8", "float8_e4m3" and
    "bfloat16" on your own; not beside ``residual_dtype``) and "bfloat16x3"
    (the hand-written graph in float32: every Linear on the split-bf16 GEMM, attention on the float32 MFMA kernel -- float32-class
    features, where "float32" itself keeps the torch module on library GEMMs); each is a ``ValueError`` anywhere else.
    ``residual_dtype``: ``None`` | "float32", for the same backbones in "float16" / "bfloat16" (not beside "bfloat16x3", whose stream
    is float32 already).
    ``int8_smoothing=alpha`` (0 < alpha <= 1, usually 0.5) with ``int8_calibration=`` (uint8 or float patches as a run takes them, or
    the scales dict of ``calibrate_int8_smoothing`` / of an earlier run's ``engine.int8_smoothing_scales``), beside "int8" only:
    per-input-channel smoothing of the three INT8 layers for checkpoints with outlier channels -- the patches are run once through
    the bfloat16 graph when the inference copy is built, and a later run with the same alpha and no new calibration reuses the copy.
    Either kwarg without the other, without "int8" or with alpha outside (0, 1] is a ``ValueError``.  Unmeasured on real checkpoints.
    ``return_attention``: ``None`` | "class" | "rollout" (patch mode, Vision Transformer backbones, every ``compute_dtype`` but
    "bfloat16x3"; per call): ``run()`` also returns ``"attention"``, float32 maps on the patch grid -- "class" ``[N, heads, gh, gw]``, the
    class token's attention in the last block (not renormalised: a map sums to 1 minus the mass on the class and register tokens),
    "rollout" ``[N, gh, gw]``, attention rollout with mean head fusion -- beside features that are bit for bit those of the run without
    it.  On the hand-written graph the maps come from ``tia_mha_probs_h`` / ``tia_rollout_step_f32`` on the qkv tensors attention
    itself read, so they describe the computation that ran, quantised routes included; a ``ValueError`` anywhere else.
    ``merge_attention``: ``None`` | "class" | "rollout", the same maps for WSI-mode runs (``patch_mode=False``; with
    ``attention_interpolation``, ``merge_resolution`` and ``merge_units``): every slide's ``.npz`` also holds ``attention``,
    ``merged_attention`` -- the slide-level heat map of :meth:`PatchPredictor.merge_attention`, merged on the device by
    ``tia_merge_patch_grids_f32`` -- and ``attention_coverage``.  ``merge_predictions`` stays refused here: features have no class map.
    ``attention_head_fusion``: "mean" | "max" | "min" and ``attention_discard_ratio``: ``0 <= r < 1`` shape the rollout maps of either
    option (per call; :class:`PatchPredictor` describes them, ``engine/_rollout_options.py`` states them; on the hand-written graph
    ``tia_mha_probs_fused_h``, ``tia_rollout_discard_normalize_f32`` and ``tia_rollout_product_f32``); the defaults are today's maps,
    a non-default value without a rollout request is a ``ValueError``.
    ``return_cam`` / ``merge_cam`` (the class activation maps of :class:`PatchPredictor`) are refused here: a feature extractor has no
    classifier to map."""

    def __init__(self, model, batch_size: int = 8, num_workers: int = 0, weights=None, *,
                 device: str = "cpu", verbose: bool = True) -> None:
        super().__init__(model=model, batch_size=batch_size, num_workers=num_workers, weights=weights,
                         device=device, verbose=verbose)
        self.process_prediction_per_batch = False
        self.return_probabilities = True

    def _update_run_params(self, images, **kwargs):
        kwargs["return_probabilities"] = True  # the features ARE the output (ref. :262-290 ignores the flag)
        if kwargs.get("merge_predictions"):
            msg = "merge_predictions merges class probabilities into a tissue-type map; feature vectors have no such map."
            raise ValueError(msg)
        for option in ("return_cam", "merge_cam"):
            if kwargs.get(option, False) is not False:
                msg = (f"{option} maps the classifier of a CNNModel over its trunk's last feature map (PatchPredictor); a feature "
                       f"extractor has no classifier; got {option}={kwargs[option]!r} for DeepFeatureExtractor.")
                raise ValueError(msg)
        return super()._update_run_params(images, **kwargs)

    def post_process_patches(self, raw_predictions: dict, **_) -> dict:
        """Features pass through unchanged (ref. :262-290)."""
        return raw_predictions

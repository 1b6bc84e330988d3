"""Pre-processing registry (API of reference ``tiatoolbox/models/dataset/classification.py``)."""

from __future__ import annotations

import numpy as np
import torch


class UnitUInt8:
    """A uint8 NHWC device batch whose ``ToTensor`` step (``float32 / 255``) has been DEFERRED into the consumer: the
    hand-written ResNet stem divides by 255 while it loads the bytes, so the 4x larger float32 copy of the batch is never
    written.  The engines unwrap it and call the model directly (``EngineABC._forward_batch``)."""

    __slots__ = ("data",)

    def __init__(self, data: torch.Tensor) -> None:
        if data.dtype != torch.uint8:
            msg = "UnitUInt8 wraps a uint8 batch."
            raise TypeError(msg)
        self.data = data

    def __len__(self) -> int:
        return self.data.shape[0]


class _TorchPreprocCaller:
    """``ToTensor()`` followed by ``permute(1, 2, 0)``: uint8 HWC -> float32 HWC in [0, 1] (ref. :15-32).

    ``device_batch`` is the batched on-device form the engines use; with ``defer_unit_scale=True`` a uint8 batch comes
    back wrapped in :class:`UnitUInt8` (same values, the division happens in the model's stem kernel).
    """

    supports_deferred_unit_scale = True

    def __init__(self, preprocs: list) -> None:
        self.preprocs = preprocs

    def __call__(self, img) -> torch.Tensor:
        arr = np.asarray(img)
        t = torch.from_numpy(np.ascontiguousarray(arr))
        if t.dtype == torch.uint8:
            return t.to(torch.float32).div(255)
        return t.to(torch.float32) if t.dtype != torch.float32 else t

    @staticmethod
    def device_batch(batch: torch.Tensor, dtype: torch.dtype, *, defer_unit_scale: bool = False):
        if batch.dtype == torch.uint8:
            if defer_unit_scale and batch.is_cuda:
                return UnitUInt8(batch.contiguous())
            return batch.to(torch.float32).div(255).to(dtype)
        return batch.to(dtype)


def predefined_preproc_func(dataset_name: str) -> _TorchPreprocCaller:
    """Pre-processing used by the pretrained models of a dataset (ref. :35-63)."""
    preproc_dict = {"kather100k": ["ToTensor"], "pcam": ["ToTensor"]}
    if dataset_name not in preproc_dict:
        msg = f"Predefined preprocessing for dataset `{dataset_name}` does not exist."
        raise ValueError(msg)
    return _TorchPreprocCaller(preproc_dict[dataset_name])


class NormUInt8:
    """A uint8 NHWC device batch whose ``ToTensor`` + ``Normalize`` step has been DEFERRED into the consumer, like
    :class:`UnitUInt8`: ``FusedViT.forward_uint8`` looks every byte up in ``hook``'s table while its im2col kernel lays the patches
    out as tokens, so neither a float32 nor a half copy of the batch is written.  The engines unwrap it
    (``EngineABC._forward_batch``)."""

    __slots__ = ("data", "hook")

    def __init__(self, data: torch.Tensor, hook: TimmNormPreproc) -> None:
        if data.dtype != torch.uint8:
            msg = "NormUInt8 wraps a uint8 batch."
            raise TypeError(msg)
        self.data, self.hook = data, hook

    def __len__(self) -> int:
        return self.data.shape[0]


class TimmNormPreproc:
    """``ToTensor()`` then ``Normalize(mean, std)``: uint8 HWC -> float32 HWC ``((x / 255) - mean) / std``, torchvision's order, every
    step rounded in float32 -- what each model the reference's ``TimmBackbone`` / ``TimmModel`` builds expects of its caller.

    A byte has 256 values, so the hook IS a table: ``table [256, 3]`` is worked out once, on the host CPU, in float32, in exactly
    that order (IEEE division; nothing is left to how a device divides -- a GPU's division by a host scalar is a multiplication by
    its reciprocal), and every form of the hook is a look-up in it:

    * ``hook(img)``: ``table[img, channel]`` per patch (the reference's per-item form; picklable for DataLoader workers);
    * ``device_batch(batch, dtype)``: ``table.to(dtype)[batch, channel]`` on the batch's device -- one rounding of the 768 entries, no
      arithmetic on the device;
    * deferred (``defer_norm=True``, a uint8 CUDA batch): the batch comes back as it is in :class:`NormUInt8` and
      ``tia_vit_patchify_norm_u8_h`` makes the same look-up inside the im2col.

    The three are equal bit for bit by construction.  A batch that is not uint8 is taken as already in ``ToTensor``'s range, as
    ``ToTensor`` itself takes a float array: ``(x - mean) / std`` in float32.
    """

    def __init__(self, mean, std) -> None:
        self.mean = np.broadcast_to(np.asarray(mean, dtype=np.float32), (3,)).copy()
        self.std = np.broadcast_to(np.asarray(std, dtype=np.float32), (3,)).copy()
        if not (np.all(np.isfinite(self.mean)) and np.all(np.isfinite(self.std)) and np.all(self.std > 0)):
            msg = f"TimmNormPreproc needs finite means and positive finite standard deviations; got {mean}, {std}."
            raise ValueError(msg)
        values = np.arange(256, dtype=np.float32)[:, None]
        self.table = torch.from_numpy(((values / np.float32(255)) - self.mean) / self.std)  # float32 [256, 3]; each step rounded
        self._tables: dict = {}

    def __getstate__(self) -> dict:
        return {"mean": self.mean, "std": self.std, "table": self.table, "_tables": {}}  # (device copies are not pickled)

    def device_table(self, device, dtype: torch.dtype) -> torch.Tensor:
        """``table`` rounded once to ``dtype`` on ``device`` (cached per device and dtype)."""
        key = (torch.device(device), dtype)
        if key not in self._tables:
            self._tables[key] = self.table.to(dtype).to(key[0]).contiguous()
        return self._tables[key]

    def _lookup(self, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        if x.shape[-1] != 3:  # noqa: PLR2004
            msg = f"TimmNormPreproc takes channel-last RGB; got shape {tuple(x.shape)}."
            raise ValueError(msg)
        if x.dtype == torch.uint8:
            return self.device_table(x.device, dtype)[x.long(), torch.arange(3, device=x.device)]
        mean, std = torch.from_numpy(self.mean).to(x.device), torch.from_numpy(self.std).to(x.device)
        return x.to(torch.float32).sub(mean).div(std).to(dtype)

    def __call__(self, img) -> torch.Tensor:
        return self._lookup(torch.from_numpy(np.ascontiguousarray(np.asarray(img))), torch.float32)

    def device_batch(self, batch: torch.Tensor, dtype: torch.dtype, *, defer_norm: bool = False):
        if defer_norm and batch.dtype == torch.uint8 and batch.is_cuda:
            return NormUInt8(batch.contiguous(), self)
        return self._lookup(batch, dtype)


# (mean, std) as each model's card publishes them for `transforms.Normalize` -- the MahmoodLab/UNI and UNI2-h, prov-gigapath and
# paige-ai/Virchow / Virchow2 cards (ImageNet's constants), the bioptimus/H-optimus-0 and H-optimus-1 cards (their own), and timm's
# `vit_*_patch16_224.augreg` pretrained configurations (0.5 / 0.5).  Written down from those cards; see DESIGN 4.33.
_IMAGENET_NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
_H_OPTIMUS_NORM = ((0.707223, 0.578729, 0.703617), (0.211883, 0.230117, 0.177517))
_INCEPTION_NORM = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
TIMM_NORM_CONSTANTS: dict[str, tuple[tuple[float, float, float], tuple[float, float, float]]] = {
    "UNI": _IMAGENET_NORM, "UNI2": _IMAGENET_NORM, "prov-gigapath": _IMAGENET_NORM, "Virchow": _IMAGENET_NORM, "Virchow2": _IMAGENET_NORM,
    "H-optimus-0": _H_OPTIMUS_NORM, "H-optimus-1": _H_OPTIMUS_NORM,
    "vit_small_patch16_224": _INCEPTION_NORM, "vit_base_patch16_224": _INCEPTION_NORM, "vit_large_patch16_224": _INCEPTION_NORM,
}


def timm_preproc_func(backbone: str) -> TimmNormPreproc:
    """The input normalisation of a ``TimmBackbone`` / ``TimmModel`` backbone: ``model.preproc_func = timm_preproc_func("UNI")``."""
    if backbone not in TIMM_NORM_CONSTANTS:
        msg = f"Predefined preprocessing for backbone `{backbone}` does not exist."
        raise ValueError(msg)
    return TimmNormPreproc(*TIMM_NORM_CONSTANTS[backbone])


class StainNormPreproc:
    """Stain-normalise, then apply the model's own pre-processing.

    The reference injects stain normalisation by *replacing* ``model.preproc_func``
    (``models_abc.py:168-171``), which drops the dataset's ``ToTensor`` step unless the user
    composes both.  This callable is that composition: picklable for DataLoader workers,
    and recognised by the engines, which run it batched on the GPU
    (``tia_stain_stats_u8`` + ``tia_stain_apply_u8`` writing the CNN input directly).
    """

    def __init__(self, normalizer, then: _TorchPreprocCaller | None = None) -> None:
        self.normalizer = normalizer
        self.then = then if then is not None else predefined_preproc_func("kather100k")

    def __call__(self, img):
        return self.then(self.normalizer.transform(img))

    @property
    def supports_deferred_unit_scale(self) -> bool:
        return isinstance(self.then, _TorchPreprocCaller)

    def device_batch(self, batch: torch.Tensor, dtype: torch.dtype, *, defer_unit_scale: bool = False):
        if defer_unit_scale and self.supports_deferred_unit_scale and batch.is_cuda:
            return UnitUInt8(self.normalizer.transform(batch, out="uint8"))  # the reference's uint8 result, 1 B / value
        kind = {torch.float16: "unit_float16", torch.bfloat16: "unit_bfloat16",
                torch.float32: "unit_float32"}[dtype]
        return self.normalizer.transform(batch, out=kind)

"""Patch-classification CNNs (API of reference ``tiatoolbox/models/architecture/vanilla.py``)."""

from __future__ import annotations

import numpy as np
import torch
from torch import nn

from tiatoolbox_amd.models.architecture.resnet import _CFG, resnet_trunk
from tiatoolbox_amd.models.architecture.utils import argmax_last_axis
from tiatoolbox_amd.models.architecture.vit import VIT_CONFIGS, create_vit
from tiatoolbox_amd.models.models_abc import ModelABC


def _get_architecture(arch_name: str, **_: dict) -> nn.Sequential:
    """Backbone without the final pooling / FC (ref. :112-164); the torchvision ResNet family only (ResNet, ResNeXt,
    Wide-ResNet)."""
    if arch_name not in _CFG:
        msg = f"Backbone `{arch_name}` is not supported."
        raise ValueError(msg)
    return resnet_trunk(arch_name)


def _infer_batch(model: nn.Module, batch_data, device: str):
    """Forward one NHWC batch (ref. :215-253): to device, float32, NCHW, eval + inference_mode.

    Returns NumPy for host input (reference behaviour); a batch that is already a CUDA tensor
    stays on the device (the engines keep results resident and copy back once).
    """
    on_device = isinstance(batch_data, torch.Tensor) and batch_data.is_cuda
    if not isinstance(batch_data, torch.Tensor):
        batch_data = torch.as_tensor(np.asarray(batch_data))
    param = next(model.parameters())
    x = batch_data.to(device=device)
    x = x.to(param.dtype) if param.dtype != torch.float32 else x.type(torch.float32)
    x = x.permute(0, 3, 1, 2)  # NHWC memory == channels_last NCHW view: no copy
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    model.eval()
    with torch.inference_mode():
        output = model(x)
    output = output.float()
    return output if on_device else output.cpu().numpy()


class CNNModel(ModelABC):
    """Backbone + global average pool + linear classifier + softmax (ref. :256-359)."""

    def __init__(self, backbone: str, num_classes: int = 1) -> None:
        super().__init__()
        self.num_classes = num_classes
        self.feat_extract = _get_architecture(backbone)
        self.pool = nn.AdaptiveAvgPool2d((1, 1))
        with torch.no_grad():
            prev_num_ch = self.feat_extract(torch.rand([2, 3, 96, 96])).shape[1]
        self.classifier = nn.Linear(prev_num_ch, num_classes)

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        feat = self.feat_extract(imgs)
        gap_feat = torch.flatten(self.pool(feat), 1)
        logit = self.classifier(gap_feat)
        return torch.softmax(logit.float(), -1)

    @staticmethod
    def postproc(image):
        return argmax_last_axis(image=image)

    @staticmethod
    def infer_batch(model: nn.Module, batch_data, device: str = "cpu"):
        return _infer_batch(model=model, batch_data=batch_data, device=device)


class CNNBackbone(ModelABC):
    """Feature extractor: backbone + global average pool (ref. :490-591)."""

    def __init__(self, backbone: str) -> None:
        super().__init__()
        self.feat_extract = _get_architecture(backbone)
        self.pool = nn.AdaptiveAvgPool2d((1, 1))

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        return torch.flatten(self.pool(self.feat_extract(imgs)), 1)

    @staticmethod
    def infer_batch(model: nn.Module, batch_data, device: str = "cpu"):
        return _infer_batch(model=model, batch_data=batch_data, device=device)


class TimmBackbone(ModelABC):
    """Feature extractor on a Vision Transformer (ref. ``TimmBackbone``): ``UNI``, the ``vit_*_patch16_224`` family and the foundation
    models ``UNI2``, ``H-optimus-0`` / ``H-optimus-1`` and ``prov-gigapath`` (``VIT_CONFIGS``), restated in plain torch with timm's
    parameter names (``architecture/vit.py``).  The features are the class token of the final norm,
    ``[B, D]``; input normalisation is the caller's ``preproc_func``, as in the reference
    (``models.dataset.classification.timm_preproc_func(backbone)`` is each model's).  ``pretrained=True`` loads
    ``<backbone>.pth`` (a timm state dict) from the local weight directories; the hub is never contacted."""

    def __init__(self, backbone: str, *, pretrained: bool = False) -> None:
        super().__init__()
        if backbone not in VIT_CONFIGS:
            msg = f"Backbone `{backbone}` is not supported."
            raise ValueError(msg)
        self.pretrained = pretrained
        self.feat_extract = create_vit(backbone)
        if pretrained:
            _load_local_vit_weights(self.feat_extract, backbone)

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        return torch.flatten(self.feat_extract(imgs), 1)

    @staticmethod
    def infer_batch(model: nn.Module, batch_data, device: str = "cpu"):
        return _infer_batch(model=model, batch_data=batch_data, device=device)


def _load_local_vit_weights(vit: nn.Module, backbone: str) -> None:
    """``pretrained=True`` of the Vision Transformer models: ``<backbone>.pth`` (a timm state dict) from the local weight
    directories, strictly; a warning and the seeded initialisation without one."""
    from tiatoolbox_amd.models.architecture import local_pretrained_weights, logger

    weights = local_pretrained_weights(backbone)
    if weights is not None:
        vit.load_state_dict(torch.load(weights, map_location="cpu"), strict=True)
    else:
        logger.warning("No local weights for `%s` (the HuggingFace hub is unreachable): using the seeded "
                       "random initialisation. Pass `weights=<path to .pth>` for the pretrained model.", backbone)


class TimmModel(ModelABC):
    """Vision Transformer + linear classifier + softmax (ref. ``TimmModel``): the linear probe on a foundation model that
    ``PatchPredictor`` runs.  ``feat_extract = create_vit(backbone)`` -- every name ``create_vit`` builds, ``Virchow`` / ``Virchow2``
    included -- and ``classifier = nn.Linear(F, num_classes)`` on its output, ``F = D`` or ``2 D`` for the class + mean-patch output of
    the Virchow models.  The state dict is ``feat_extract.<timm names>`` plus ``classifier.{weight,bias}``, so a probe trained against
    the reference loads with ``strict=True``.  ``pretrained=True`` reads the backbone's ``.pth`` as :class:`TimmBackbone` does.  Input
    normalisation is the caller's ``preproc_func``: ``models.dataset.classification.timm_preproc_func(backbone)``.

    On the GPU in fp16 / bf16 the engines run it as ``vit_fused.FusedViTClassifier``."""

    def __init__(self, backbone: str, num_classes: int = 1, *, pretrained: bool = False) -> None:
        super().__init__()
        self.pretrained = pretrained
        self.num_classes = num_classes
        self.feat_extract = create_vit(backbone)  # (an unknown name: ValueError("Backbone `X` is not supported."))
        if pretrained:
            _load_local_vit_weights(self.feat_extract, backbone)
        width = self.feat_extract.embed_dim * (2 if self.feat_extract.global_pool == "token_mean" else 1)
        self.classifier = nn.Linear(width, num_classes)

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        feat = torch.flatten(self.feat_extract(imgs), 1)
        logit = self.classifier(feat)
        return torch.softmax(logit.float(), -1)

    @staticmethod
    def postproc(image):
        return argmax_last_axis(image=image)

    @staticmethod
    def infer_batch(model: nn.Module, batch_data, device: str = "cpu"):
        return _infer_batch(model=model, batch_data=batch_data, device=device)

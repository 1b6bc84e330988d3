"""Class activation maps of a CNN classifier (``PatchPredictor.run(return_cam=True)`` / ``merge_cam=True``).

**The model.**  ``CNNModel.forward`` is trunk -> global average pool -> ``nn.Linear`` -> softmax.  With ``F`` ``[N, C, h, w]`` the
output of ``model.feat_extract`` in the dtype the run computes in, and ``W`` ``[K, C]``, ``b`` ``[K]`` the parameters of
``model.classifier`` as the inference copy holds them (in fp16 / bf16: the weights already rounded to the half type, widened to
float32 -- the maps describe the computation that ran), the class activation map (Zhou et al. 2016) is the classifier applied at
every position of ``F``::

    cam[n, k, y, x] = sum_c W[k, c] * F[n, c, y, x]

-- a float32 result of float32 multiply-adds on the widened values.  **No bias, no ReLU, nothing renormalised.**  The bias
convention: the map leaves ``b`` out, and mathematically ``logit[n, k] = mean_{y, x} cam[n, k] + b[k]``, so
``softmax(mean(cam) + b)`` is the run's probability up to the rounding of the two orders of summation (and, in half precision, of
the pooled features and the logit, which torch rounds to the half type once each).  For this head the map equals Grad-CAM on the
last layer up to Grad-CAM's ReLU and scale.  The values are raw logit contributions: comparable across classes within a patch,
across patches only as logits are.

:func:`class_activation_maps` is the statement in NumPy and :func:`logits_from_maps` its bias convention: the specification the
tests use.  :func:`cam_torch` is the same sum in plain torch, which the engines use without a HIP device; on a CUDA device they
launch ``tia_cam_nhwc_f32`` / ``tia_cam_nhwc_h`` (``architecture/fused.py``: ``hip_cam``, ``csrc/cnn_cam.hip``) on the feature map
the forward left in HBM.  The orders of summation differ: every order of ``C`` float32 multiply-adds stays within
``(C + 8) * 2^-24 * sum_c |W[k, c] F[n, c, y, x]|`` of the exact sum.
"""

from __future__ import annotations

import numpy as np
import torch


def _as_f32(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().float().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def class_activation_maps(features, weight) -> np.ndarray:
    """``cam[n, k, y, x] = sum_c weight[k, c] * features[n, c, y, x]`` in float32: ``features`` ``[N, C, h, w]`` (any float type,
    widened), ``weight`` ``[K, C]``; returns ``[N, K, h, w]`` float32."""
    f, w = _as_f32(features), _as_f32(weight)
    if f.ndim != 4 or w.ndim != 2 or f.shape[1] != w.shape[1]:  # noqa: PLR2004
        msg = f"features [N, C, h, w] and weight [K, C] must agree in C, got {f.shape} and {w.shape}."
        raise ValueError(msg)
    return np.einsum("kc,nchw->nkhw", w, f).astype(np.float32, copy=False)


def logits_from_maps(cam, bias) -> np.ndarray:
    """The bias convention: ``logit[n, k] = mean_{y, x} cam[n, k, y, x] + bias[k]`` (float64 from the float32 maps)."""
    cam = np.asarray(cam, dtype=np.float64)
    return cam.mean(axis=(2, 3)) + np.asarray(_as_f32(bias), dtype=np.float64)[None]


def cam_torch(features: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """:func:`class_activation_maps` in plain torch on the tensors' device (the engines' path without a HIP device)."""
    with torch.no_grad():
        return torch.einsum("kc,nchw->nkhw", weight.detach().float(), features.detach().float()).contiguous()


def is_cam_model(model) -> bool:
    """Whether ``model`` computes exactly ``softmax(classifier(flatten(pool(feat_extract(x)))))`` with a global average pool and an
    ``nn.Linear``: a :class:`CNNModel` with the stock ``forward``."""
    from tiatoolbox_amd.models.architecture.vanilla import CNNModel

    pool, head = getattr(model, "pool", None), getattr(model, "classifier", None)
    return (isinstance(model, CNNModel) and type(model).forward is CNNModel.forward and isinstance(head, torch.nn.Linear)
            and isinstance(pool, torch.nn.AdaptiveAvgPool2d) and pool.output_size in ((1, 1), 1))

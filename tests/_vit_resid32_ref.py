"""Host-only helpers of the ``residual_dtype="float32"`` tests: torch restatements of the three new wrappers (their stated arithmetic,
not their code), the model forms with their float64 references, the error figure and the autocast yardstick."""

from __future__ import annotations

import copy

import torch
import torch.nn.functional as F  # noqa: N812

import _vit_foundation_ref
import _vit_ref
import _vit_virchow_ref
from _vit_foundation_ref import TINY_REG, tiny_foundation
from _vit_ref import tiny_vit
from _vit_virchow_ref import TINY_V1, TINY_V2, tiny_virchow

NEW_WRAPPERS = ("hip_add_layernorm_rows_f32", "hip_vit_assemble_rows_f32", "hip_vit_cls_mean_pool_f32")

# name -> (builder, input side): the plain graph, register tokens without a class entry + packed SwiGLU at patch 14, and the
# Virchow forms (token_mean; V2 with prefix_pos_embed and a padded SwiGLU)
FORMS = {
    "tiny": (lambda: tiny_vit(layer_scale=True), 32),
    "tiny-reg-swiglu": (lambda: tiny_foundation(TINY_REG), 28),
    "tiny-v1": (lambda: tiny_virchow(TINY_V1), 28),
    "tiny-v2": (lambda: tiny_virchow(TINY_V2), 28),
}


def rel_error(got: torch.Tensor, ref: torch.Tensor) -> float:
    """``e = max |got - ref| / max(max |ref|, 1)``, the figure of the graph-level tests."""
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1.0)


def ref64(vit, x_nchw: torch.Tensor) -> torch.Tensor:
    """The form's own float64 restatement of the forward (``forward64`` of ``_vit_ref`` / ``_vit_foundation_ref`` / ``_vit_virchow_ref``)."""
    kw = {"heads": vit.num_heads, "patch": vit.patch_size, "native_grid": vit.native_grid}
    sd = vit.state_dict()
    if vit.global_pool == "token_mean":
        return _vit_virchow_ref.forward64(sd, x_nchw, **kw)
    if vit.reg_tokens or vit.no_embed_class or vit.mlp_layer == "swiglu_packed":
        return _vit_foundation_ref.forward64(sd, x_nchw, no_embed_class=vit.no_embed_class, **kw)
    return _vit_ref.forward64(sd, x_nchw, **kw)


def autocast_features(vit, x_nchw: torch.Tensor, dtype: torch.dtype, device: str) -> torch.Tensor:
    """The yardstick with a float32 residual stream: the float32 module under ``torch.autocast(device, dtype)``."""
    with torch.no_grad(), torch.autocast(device, dtype=dtype):
        return copy.deepcopy(vit).to(device)(x_nchw.to(device)).float().cpu()


def cast_features(vit, x_nchw: torch.Tensor, dtype: torch.dtype, device: str) -> torch.Tensor:
    """The yardstick with a half residual stream: the module cast to ``dtype``."""
    with torch.no_grad():
        return copy.deepcopy(vit).to(device).to(dtype)(x_nchw.to(device).to(dtype)).float().cpu()


def fused_graph(vit, dtype: torch.dtype, device: str, **prepare):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(copy.deepcopy(vit).to(device))
    fused.prepare(dtype, **prepare)
    return fused.to(dtype)


def scale_layer_scale(vit, factor: float):
    """Every ``*.gamma`` (LayerScale) multiplied by ``factor``, in place."""
    with torch.no_grad():
        for name, p in vit.named_parameters():
            if name.endswith("gamma"):
                p.mul_(factor)
    return vit


def _rows(t: torch.Tensor, rows: int, c: int, stride: int) -> torch.Tensor:
    return torch.as_strided(t.reshape(-1), (rows, c), (stride, 1))  # (a view of the contiguous tensor: writes land in `t`)


def torch_resid32_wrappers(calls: dict | None = None) -> dict:
    """Torch restatements of the three float32-stream wrappers, for any device: name -> function."""
    calls = {} if calls is None else calls

    def count(name):
        calls[name] = calls.get(name, 0) + 1

    def add_layernorm(x, branch, gamma, beta, *, eps, rows, row_stride, dtype, out_dtype=None):
        count("hip_add_layernorm_rows_f32")
        assert x.dtype == torch.float32 and x.is_contiguous() and (branch is None or (branch.dtype == dtype and branch.shape == x.shape))
        c = gamma.numel() if gamma is not None else x.shape[-1]
        xr = _rows(x, rows, c, row_stride)
        if branch is not None:
            xr.add_(_rows(branch, rows, c, row_stride).float())  # one float32 add, in place
        if gamma is None:
            return None
        return F.layer_norm(xr, (c,), gamma, beta, eps).to(out_dtype or dtype)

    def assemble(tok, cls, reg, pos, *, pos_has_cls):
        count("hip_vit_assemble_rows_f32")
        n, _, d = tok.shape
        pos = pos.reshape(-1, d)
        parts = [(cls.reshape(1, d) + (pos[:1] if pos_has_cls else 0.0)).expand(n, -1, -1)]
        if reg is not None:
            parts.append(reg.reshape(1, -1, d).expand(n, -1, -1))
        parts.append(tok.float() + pos[int(pos_has_cls):])
        return torch.cat(parts, 1).contiguous()

    def cls_mean_pool(x, branch, gamma, beta, *, eps, skip, dtype):
        count("hip_vit_cls_mean_pool_f32")
        assert x.dtype == torch.float32 and (branch is None or branch.dtype == dtype)
        xs = x if branch is None else x + branch.float()
        y = F.layer_norm(xs, (x.shape[-1],), gamma, beta, eps)
        return torch.cat([y[:, 0], y[:, skip:].mean(1)], -1)

    return dict(zip(NEW_WRAPPERS, (add_layernorm, assemble, cls_mean_pool)))

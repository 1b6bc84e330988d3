"""Host-only helpers of the ``compute_dtype="bfloat16x3"`` tests: torch restatements of the float32 route's wrappers (their stated
arithmetic, not their code), for any device, and the graph builder."""

from __future__ import annotations

import copy

import torch
import torch.nn.functional as F  # noqa: N812

from _vit_classifier_ref import patchify_ref

NEW_WRAPPERS = ("pack_linear_weights_split", "pack_linear_weights_f32", "hip_linear_f32", "hip_mha_fwd_f32", "hip_gelu_rows_f32_",
                "hip_swiglu_rows_f32", "hip_vit_patchify_f32", "hip_vit_assemble_f32")


def split_graph(vit, device: str):
    """``FusedViT`` of a copy of ``vit`` on ``device``, prepared for the float32 route."""
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(copy.deepcopy(vit).to(device))
    fused.prepare(torch.float32, linear_dtype="bfloat16x3")
    return fused


def torch_f32_wrappers(calls: dict | None = None) -> dict:
    """name -> function.  The split weights are handed over as the three planes ``[3, cout, cin]`` in bfloat16 (what the kernel
    multiplies by: their exact sum is the float32 weight), the float32 kernel's as ``[1, 1, cin, cout]``."""
    calls = {} if calls is None else calls

    def count(name):
        calls[name] = calls.get(name, 0) + 1

    def pack_split(weight):
        from tiatoolbox_amd.models.architecture.fused import split_stem_weights

        count("pack_linear_weights_split")
        cout, cin = weight.shape
        if cin % 16 or cout % 128:
            return None
        parts, usable = split_stem_weights(weight)
        return parts.to(torch.bfloat16) if usable else None

    def pack_f32(weight):
        count("pack_linear_weights_f32")
        cout, cin = weight.shape
        return weight.detach().float().T.reshape(1, 1, cin, cout).contiguous()

    def linear(x, w_packed, bias, residual=None, *, cout):
        count("hip_linear_f32")
        assert x.dtype == torch.float32 and (residual is None or (residual.dtype == torch.float32 and residual.shape[-1] == cout))
        if w_packed.dtype == torch.bfloat16:
            calls["split_calls"] = calls.get("split_calls", 0) + 1
            w = w_packed.double().sum(0).float()
        else:
            w = w_packed.reshape(x.shape[-1], cout).T
        y = F.linear(x, w, bias)
        return y if residual is None else y + residual

    def mha(qkv, heads, scale):
        count("hip_mha_fwd_f32")
        assert qkv.dtype == torch.float32
        n, s, c3 = qkv.shape
        hd = c3 // (3 * heads)
        q, k, v = (qkv.reshape(n, s, 3, heads, hd)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        return F.scaled_dot_product_attention(q, k, v, scale=scale).permute(0, 2, 1, 3).reshape(n, s, heads * hd).contiguous()

    def gelu_(x):
        count("hip_gelu_rows_f32_")
        return x.copy_(F.gelu(x))

    def swiglu(x):
        count("hip_swiglu_rows_f32")
        hidden = x.shape[-1] // 2
        return F.silu(x[..., :hidden]) * x[..., hidden:]

    def patchify(x_nhwc, patch, k_pad):
        count("hip_vit_patchify_f32")
        assert x_nhwc.dtype == torch.float32
        return patchify_ref(x_nhwc, patch, k_pad)

    def assemble(tok, cls, reg, pos, *, pos_has_cls):
        count("hip_vit_assemble_f32")
        assert tok.dtype == torch.float32
        n, _, d = tok.shape
        pos = pos.reshape(-1, d)
        parts = [(cls.reshape(1, d) + (pos[:1] if pos_has_cls else 0.0)).expand(n, -1, -1)]
        if reg is not None:
            parts.append(reg.reshape(1, -1, d).expand(n, -1, -1))
        parts.append(tok + pos[int(pos_has_cls):])
        return torch.cat(parts, 1).contiguous()

    return dict(zip(NEW_WRAPPERS, (pack_split, pack_f32, linear, mha, gelu_, swiglu, patchify, assemble)))

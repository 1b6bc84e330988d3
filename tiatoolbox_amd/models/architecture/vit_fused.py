"""Inference copy of :class:`~tiatoolbox_amd.models.architecture.vit.VisionTransformer` on the hand-written kernels, fp16 / bf16
activations (``FusedViT(vit)`` then ``prepare(dtype)``, in the manner of ``FusedUNet`` / ``FusedHoVerNet``).

Same arithmetic graph as the module's forward.  Every Linear -- the patch embedding included, after ``tia_vit_patchify_h`` has laid
the patches out as ``[n, g, p * p * 3]`` tokens -- is the half implicit-GEMM kernel with a 1x1 window (``tia_conv2d_nhwc_h`` on
the tokens as an ``[n, S, 1, C]`` NHWC map: float32 accumulation, bias and residual in the epilogue, one rounding).  Per block:

1. ``tia_layernorm_rows_h``            5. ``tia_layernorm_rows_h``
2. ``qkv`` GEMM (bias)                 6. ``fc1`` GEMM (bias)
3. ``tia_mha_fwd_h``                   7. ``tia_gelu_rows_h`` (in place)
4. ``proj`` GEMM (bias + residual)     8. ``fc2`` GEMM (bias + residual)

The foundation models (``UNI2``, ``H-optimus-0`` / ``-1``, ``prov-gigapath``) change three places of this graph and nothing else:

* ``mlp_layer="swiglu_packed"``: step 7 is ``tia_swiglu_rows_h`` (``[n, S, 2H] -> [n, S, H]``, the first half the gate) and ``fc2`` has
  ``cin = H``;
* a patch size that is no multiple of 8 (14): ``tia_vit_patchify_pad_h`` writes token rows of ``k_pad = ceil(3 p^2 / 32) * 32``
  columns (608), zeros beyond ``3 p^2``, and the permuted patch weight is zero-padded alike in float32 before packing -- the
  embedding is still ONE GEMM; multiples of 8 keep ``tia_vit_patchify_h``;
* register tokens or ``no_embed_class``: ``tia_vit_assemble_prefix_h`` (``cat([cls, reg, patches + pos])``) in place of
  ``tia_vit_assemble_tokens_h``.  The class token is still row 0, so the final norm reads the same rows.

LayerScale is folded EXACTLY in float32 before the one rounding of the weights: ``x + gamma * (W a + b) = x + (gamma W) a + gamma b``, so
the residual add is the GEMM's own ``d_residual`` and ``ls1`` / ``ls2`` cost nothing.  By default the residual stream stays in
``dtype`` (as in the torch module cast to ``dtype``); the final norm reads the class rows only (row stride ``S * D``) and writes float32
features.

``prepare(dtype, residual_dtype="float32")`` (the engines' run kwarg ``residual_dtype``) keeps the stream in float32 instead, as the
float32 module under ``torch.autocast`` does: ``tia_vit_assemble_rows_f32`` writes ``x`` unrounded, steps 4 and 8 lose their residual
and write a half branch, and steps 1 and 5 (and the final norm) become ``tia_add_layernorm_rows_f32`` -- ``x += float(branch)`` in
place and the LayerNorm of the sum in one pass; ``token_mean`` models end in ``tia_vit_cls_mean_pool_f32``.  A LayerScale update below
half a unit of ``dtype`` at ``x`` is rounded away by the default graph and kept by this one.

``Virchow`` / ``Virchow2`` (ViT-H/14, 1280 / 16 = 80 per head) change four more, all on the host in float32 before the one rounding:

* ``head_dim`` 80: the other instantiation of ``tia_mha_fwd_h``'s kernel; ``scale = 80 ** -0.5``;
* a packed SwiGLU whose half (3416) is off the GEMM's multiple of 32: each half of ``fc1`` is padded with zero rows and zero bias to
  3424 and ``fc2`` with zero columns (``pad_swiglu``; halves below 512 are not padded) -- a pad lane is ``silu(0) * 0 = 0`` exactly;
* ``prefix_pos_embed`` (register tokens with entries of their own in the position table): ``cls + pos[0]`` and ``reg + pos[1 : 1 + R]``
  are added per grid in float32 and handed to ``tia_vit_assemble_prefix_h`` with ``pos_has_cls = 0`` -- the same single add before the
  same single rounding;
* ``global_pool="token_mean"``: the last step is ``tia_vit_cls_mean_pool_h`` (``[n, 2D]``: the class row's LayerNorm beside the mean of
  the patch rows' LayerNorms, register rows left out) in place of the class-row LayerNorm.

Classifiers (``vanilla.TimmModel``) add the two ends: ``forward_uint8(x_u8_nhwc, table)`` takes the uint8 patches themselves --
``tia_vit_patchify_norm_u8_h`` is the padded im2col with ``ToTensor`` + ``Normalize`` looked up per byte in ``TimmNormPreproc``'s ``[256, 3]``
table, bit for bit ``forward`` of the hook's batched form -- and :class:`FusedViTClassifier` puts ``tia_linear_softmax_rows_f32`` (the
Linear and the softmax, float32 throughout) on the graph's float32 features.

``prepare(torch.bfloat16, linear_dtype="float8_e4m3")`` (the engines' ``compute_dtype="float8_e4m3"``) puts steps 2, 6 and 8 -- ``qkv``,
``fc1``, ``fc2``: 11/12 of a block's linear flops -- on the FP8 GEMM ``tia_linear_fp8_rows`` (row x column scaled OCP e4m3fn on the K = 128
matrix instruction) and steps 1, 5 and 7 on their quantising forms (``tia_layernorm_rows_q8``, ``tia_gelu_rows_q8`` /
``tia_swiglu_rows_q8``: codes and one scale per token from the float32 value, no extra pass).  The carrier stays bfloat16; attention,
``proj``, the patch embedding and the ends of the graph are unchanged.  :func:`quantize_rows_e4m3` states the recipe; DESIGN 4.34.

``prepare(torch.bfloat16, linear_dtype="int8")`` (the engines' ``compute_dtype="int8"``) routes the same three layers to the INT8 GEMM
``tia_linear_int8_rows`` (W8A8 on ``v_mfma_i32_16x16x64_i8``, one scale per token and per output channel, exact int32 accumulation)
and the same three steps to ``tia_layernorm_rows_qi8`` / ``tia_gelu_rows_qi8`` / ``tia_swiglu_rows_qi8``.  A uniform 8-bit grid in
place of e4m3's 3-bit mantissa: closer than FP8 on rows without extreme outliers, worse with an outlier channel.
:func:`quantize_rows_int8` states the recipe; DESIGN 4.38.  ``smoothing=scales`` beside it (the engines' ``int8_smoothing`` /
``int8_calibration``) divides each routed layer's input by a power of two per channel and multiplies the weight column by it
(:func:`int8_smoothing_scales` states the recipe, :func:`calibrate_int8_smoothing` measures the statistics on the bfloat16 graph with
``tia_*_rows_absmax_h``): folded into the LayerNorm affine for ``qkv`` / ``fc1``, ``tia_gelu_rows_qi8_smooth`` /
``tia_swiglu_rows_qi8_smooth`` in front of ``fc2``; DESIGN 4.41.

``prepare(torch.float32, linear_dtype="bfloat16x3")`` (the engines' ``compute_dtype="bfloat16x3"``) is the float32 route of the same
graph: activations, residual stream and row arithmetic in float32; every Linear on ``tia_conv2d_bf16x3_nhwc_f32`` (both operands
split into three bf16 numbers, six exact products per float32 product, float32 accumulation; the weights split once with
``fused.split_stem_weights``, bias and the float32 residual in the epilogue) or, off that kernel's shapes, ``tia_conv2d_nhwc_f32``;
attention on ``tia_mha_fwd_f32`` (``v_mfma_f32_16x16x4_f32``); ``tia_gelu_rows_f32`` / ``tia_swiglu_rows_f32``, ``tia_vit_patchify_f32``
and ``tia_vit_assemble_f32`` beside the float32 LayerNorm, pool and head that exist already.  The batch is the
normalised float32 tensor; there is no uint8 im2col on this route.

``return_attention`` (an attribute the engines set for a run: ``None`` | "class" | "rollout", their run kwarg of that name) makes every
half route return attention maps beside its output, in ``attention_maps`` after each ``forward`` / ``forward_uint8``: behind step 3 the
SAME qkv tensor goes to ``tia_mha_probs_h`` (the float32 probabilities attention never materialises: the class row per head in the last
block, or all rows with the head mean in every block) and, for the rollout, ``tia_rollout_step_f32``
(``R = (A R) / 2 + R / 2`` on ``v_mfma_f32_16x16x4_f32``).  They write buffers of their own, so the features are bit for bit those of the
run without maps, and with ``None`` nothing is launched.  ``VisionTransformer.forward_with_attention`` states both maps; DESIGN 4.42.
``attention_head_fusion`` ("mean" | "max" | "min") and ``attention_discard_ratio`` (attributes the engines set beside it) are the
rollout's other forms: with anything but ("mean", a discard count of 0) a block launches ``tia_mha_probs_fused_h``,
``tia_rollout_discard_normalize_f32`` and, after the first block, ``tia_rollout_product_f32`` in place of those two kernels -- and
with the defaults exactly those two.  ``models/engine/_rollout_options.py`` states the arithmetic; DESIGN 4.44.

There is no library fall-back: a model the kernels do not take (``D / heads`` other than 64 or 80, channel counts off the GEMM's
multiples) raises ``UnsupportedLayerError`` from the constructor.
"""

from __future__ import annotations

from typing import NamedTuple

import torch
from torch import nn

from tiatoolbox_amd.models.architecture.fused import _DT, _ptr
from tiatoolbox_amd.models.architecture.unet_fused import UnsupportedLayerError
from tiatoolbox_amd.models.architecture.vit import LN_EPS, LayerScale, VisionTransformer, resample_pos_embed

_HALF = (torch.float16, torch.bfloat16)


def _half_tokens(name: str, x: torch.Tensor, last: int | None = None) -> None:
    if not (x.is_cuda and x.dtype in _HALF and x.is_contiguous() and (last is None or x.shape[-1] == last)):
        msg = f"{name} expects a contiguous fp16 / bf16 CUDA tensor" + (f" with {last} channels" if last is not None else "") + \
              f"; got {tuple(x.shape)}, {x.dtype} on {x.device}."
        raise ValueError(msg)


def fold_layer_scale(linear: nn.Linear, scale: nn.Module | None) -> tuple[torch.Tensor, torch.Tensor]:
    """Float32 ``(W', b')`` with ``W' a + b' == gamma * (W a + b)``: ``gamma[:, None] * W`` and ``gamma * b`` (one float32 rounding each,
    before any rounding to half).  Without a LayerScale (``nn.Identity`` / ``None``) the Linear's own float32 weights."""
    w = linear.weight.detach().to(torch.float32)
    b = linear.bias.detach().to(torch.float32) if linear.bias is not None else torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
    if isinstance(scale, LayerScale):
        g = scale.gamma.detach().to(torch.float32)
        w, b = g[:, None] * w, g * b
    return w.contiguous(), b.contiguous()


def pack_linear_weights_h(weight: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Float32 ``[cout, cin]`` -> the half GEMM's operand ``[1, 1, cin / 8, cout, 8]`` of ``dtype`` (``tia_conv_pack_weights_h``)."""
    from tiatoolbox_amd import _lib

    w = weight.detach().to(torch.float32).contiguous()
    cout, cin = w.shape
    if not w.is_cuda or dtype not in _HALF:
        msg = f"pack_linear_weights_h packs CUDA weights for fp16 / bf16; got weights on {w.device} for {dtype}."
        raise ValueError(msg)
    out = torch.empty((1, 1, cin // 8, cout, 8), dtype=dtype, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_conv_pack_weights_h(w.data_ptr(), cout, cin, 1, 1, _DT[dtype], out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_conv_pack_weights_h")
    return out


def hip_linear_h(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None = None, *,
                 cout: int) -> torch.Tensor:
    """``x @ W^T + bias (+ residual)`` on ``[n, S, cin]`` fp16 / bf16 tokens: ``tia_conv2d_nhwc_h`` with a 1x1 window on the
    ``[n, S, 1, cin]`` map (float32 accumulation, float32 ``bias``, one rounding)."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_linear_h", x)
    n, s, cin = x.shape
    if residual is not None:
        _half_tokens("hip_linear_h (residual)", residual, cout)
        if residual.dtype != x.dtype or residual.shape[:2] != x.shape[:2]:
            msg = f"hip_linear_h: residual {tuple(residual.shape)}, {residual.dtype} beside tokens {tuple(x.shape)}, {x.dtype}."
            raise ValueError(msg)
    if w_packed.dtype != x.dtype or (bias is not None and bias.dtype != torch.float32):
        msg = f"hip_linear_h: weights packed for {w_packed.dtype} beside {x.dtype} tokens, or a bias that is not float32."
        raise ValueError(msg)
    y = torch.empty((n, s, cout), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_conv2d_nhwc_h(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), n, s, 1, cin, cout,
                                           1, 1, 1, 0, _DT[x.dtype], 0, _lib.current_stream())
    _lib.check(rc, "tia_conv2d_nhwc_h")
    return y


def hip_mha_fwd_h(qkv: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """Attention on the qkv Linear's output ``[n, S, 3 * heads * hd]`` -> ``[n, S, heads * hd]``, ``hd`` 64 or 80 (``tia_mha_fwd_h``)."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_mha_fwd_h", qkv)
    n, s, c3 = qkv.shape
    head_dim = c3 // (3 * heads)
    out = torch.empty((n, s, heads * head_dim), dtype=qkv.dtype, device=qkv.device)
    with torch.cuda.device(qkv.device):
        rc = _lib.load().tia_mha_fwd_h(qkv.data_ptr(), out.data_ptr(), n, s, heads, head_dim, float(scale), _DT[qkv.dtype],
                                       _lib.current_stream())
    _lib.check(rc, "tia_mha_fwd_h")
    return out


MHA_PROBS_MEAN_HEADS = 64  # `tia_mha_probs_h` with head_mean keeps every head's (max, sum) of a query tile in LDS: at most 64 heads


def hip_mha_probs_h(qkv: torch.Tensor, heads: int, scale: float, *, q_rows: int, head_mean: bool) -> torch.Tensor:
    """The attention probabilities of ``hip_mha_fwd_h``'s input ``[n, S, 3 * heads * hd]`` for the first ``q_rows`` queries, float32:
    ``[n, heads, q_rows, S]``, or with ``head_mean`` their mean over the heads ``[n, q_rows, S]`` (``tia_mha_probs_h``: float32
    softmax over all ``S`` keys, every value ``e_j / sum e`` rounded once; heads added in ascending order)."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_mha_probs_h", qkv)
    n, s, c3 = qkv.shape
    head_dim = c3 // (3 * heads)
    if not 1 <= q_rows <= s:
        msg = f"hip_mha_probs_h: q_rows is between 1 and the {s} tokens; got {q_rows}."
        raise ValueError(msg)
    if head_mean and heads > MHA_PROBS_MEAN_HEADS:
        msg = f"hip_mha_probs_h: the head mean takes at most {MHA_PROBS_MEAN_HEADS} heads; got {heads}."
        raise ValueError(msg)
    out = torch.empty((n, q_rows, s) if head_mean else (n, heads, q_rows, s), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        rc = _lib.load().tia_mha_probs_h(qkv.data_ptr(), out.data_ptr(), n, s, heads, head_dim, float(scale), q_rows, int(bool(head_mean)),
                                         _DT[qkv.dtype], _lib.current_stream())
    _lib.check(rc, "tia_mha_probs_h")
    return out


def hip_rollout_step_f32(a: torch.Tensor, r_in: torch.Tensor | None) -> torch.Tensor:
    """One step of attention rollout on float32 ``[n, S, S]`` matrices: ``(a @ r_in) / 2 + r_in / 2``, ``r_in=None`` the identity
    (``tia_rollout_step_f32``: one float32 fma chain per element, one final rounding)."""
    from tiatoolbox_amd import _lib

    for name, t in (("a", a), ("r_in", r_in)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3  # noqa: PLR2004
                                  and t.shape[1] == t.shape[2] and t.shape == a.shape and t.device == a.device):
            msg = f"hip_rollout_step_f32 expects contiguous float32 CUDA [n, S, S] matrices of one shape; got {name} {tuple(t.shape)}, " \
                  f"{t.dtype} on {t.device}."
            raise ValueError(msg)
    n, s, _ = a.shape
    out = torch.empty_like(a)
    with torch.cuda.device(a.device):
        rc = _lib.load().tia_rollout_step_f32(a.data_ptr(), _ptr(r_in), out.data_ptr(), n, s, _lib.current_stream())
    _lib.check(rc, "tia_rollout_step_f32")
    return out


def hip_mha_probs_fused_h(qkv: torch.Tensor, heads: int, scale: float, head_fusion: str) -> torch.Tensor:
    """The probabilities of all ``S`` query rows of ``hip_mha_fwd_h``'s input fused over the heads, float32 ``[n, S, S]``
    (``tia_mha_probs_fused_h``): "mean" is ``hip_mha_probs_h(head_mean=True)`` bit for bit, "max" / "min" the exact element-wise
    maximum / minimum of its per-head values."""
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.engine._rollout_options import FUSION_CODES

    _half_tokens("hip_mha_probs_fused_h", qkv)
    if head_fusion not in FUSION_CODES:
        msg = f"hip_mha_probs_fused_h: head_fusion is one of {tuple(FUSION_CODES)}; got {head_fusion!r}."
        raise ValueError(msg)
    if heads > MHA_PROBS_MEAN_HEADS:
        msg = f"hip_mha_probs_fused_h: a fused output takes at most {MHA_PROBS_MEAN_HEADS} heads; got {heads}."
        raise ValueError(msg)
    n, s, c3 = qkv.shape
    out = torch.empty((n, s, s), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        rc = _lib.load().tia_mha_probs_fused_h(qkv.data_ptr(), out.data_ptr(), n, s, heads, c3 // (3 * heads), float(scale),
                                               FUSION_CODES[head_fusion], _DT[qkv.dtype], _lib.current_stream())
    _lib.check(rc, "tia_mha_probs_fused_h")
    return out


def _rollout_matrices(who: str, **tensors: torch.Tensor | None) -> tuple[int, int]:
    first = next(iter(tensors.values()))
    for name, t in tensors.items():
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3  # noqa: PLR2004
                                  and t.shape[1] == t.shape[2] and t.shape == first.shape and t.device == first.device):
            msg = f"{who} expects contiguous float32 CUDA [n, S, S] matrices of one shape; got {name} {tuple(t.shape)}, {t.dtype} on {t.device}."
            raise ValueError(msg)
    return first.shape[0], first.shape[1]


def hip_rollout_discard_normalize_f32(f: torch.Tensor, k: int, *, return_threshold: bool = False):
    """``A^`` of the fused float32 ``[n, S, S]`` matrices ``f`` (``tia_rollout_discard_normalize_f32``): with ``k >= 1`` everything
    ``<=`` the ``k``-th smallest entry of an image is set to 0 (entry ``(0, 0)`` never); then ``(F' + I) / 2`` with every row divided
    by its sum.  ``return_threshold`` also returns the ``[n]`` order statistics (``None`` for ``k = 0``)."""
    from tiatoolbox_amd import _lib

    n, s = _rollout_matrices("hip_rollout_discard_normalize_f32", f=f)
    if not 0 <= k < s * s:
        msg = f"hip_rollout_discard_normalize_f32: k is between 0 and S * S - 1 = {s * s - 1}; got {k}."
        raise ValueError(msg)
    out = torch.empty_like(f)
    v = torch.empty((n,), dtype=torch.float32, device=f.device) if k else None
    with torch.cuda.device(f.device):
        rc = _lib.load().tia_rollout_discard_normalize_f32(f.data_ptr(), out.data_ptr(), _ptr(v), n, s, k, _lib.current_stream())
    _lib.check(rc, "tia_rollout_discard_normalize_f32")
    return (out, v) if return_threshold else out


def hip_rollout_product_f32(a: torch.Tensor, r_in: torch.Tensor | None) -> torch.Tensor:
    """``a @ r_in`` on float32 ``[n, S, S]`` matrices, ``r_in=None`` the identity (``tia_rollout_product_f32``: one float32 fma chain
    per element, ``k`` ascending)."""
    from tiatoolbox_amd import _lib

    n, s = _rollout_matrices("hip_rollout_product_f32", a=a, r_in=r_in)
    out = torch.empty_like(a)
    with torch.cuda.device(a.device):
        rc = _lib.load().tia_rollout_product_f32(a.data_ptr(), _ptr(r_in), out.data_ptr(), n, s, _lib.current_stream())
    _lib.check(rc, "tia_rollout_product_f32")
    return out


def hip_layernorm_rows_h(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, eps: float, rows: int, row_stride: int,
                         out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """LayerNorm of ``rows`` rows of ``c = gamma.numel()`` values that start ``row_stride`` elements apart in ``x``; float32 affine;
    the result ``[rows, c]`` in ``x``'s dtype or float32 (``tia_layernorm_rows_h``)."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_layernorm_rows_h", x)
    c = gamma.numel()
    if (rows - 1) * row_stride + c > x.numel() or gamma.dtype != torch.float32 or beta.dtype != torch.float32:
        msg = f"hip_layernorm_rows_h: {rows} rows of {c} at stride {row_stride} beyond {x.numel()} elements, or an affine that is not float32."
        raise ValueError(msg)
    out_dtype = out_dtype or x.dtype
    y = torch.empty((rows, c), dtype=out_dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_layernorm_rows_h(x.data_ptr(), row_stride, gamma.data_ptr(), beta.data_ptr(), float(eps), y.data_ptr(), rows, c,
                                              _DT[x.dtype], int(out_dtype == torch.float32), _lib.current_stream())
    _lib.check(rc, "tia_layernorm_rows_h")
    return y


def hip_gelu_rows_h_(x: torch.Tensor) -> torch.Tensor:
    """Exact GELU in place (``tia_gelu_rows_h``)."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_gelu_rows_h_", x)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_gelu_rows_h(x.data_ptr(), x.numel(), _DT[x.dtype], _lib.current_stream())
    _lib.check(rc, "tia_gelu_rows_h")
    return x


def hip_vit_patchify_h(x_nhwc: torch.Tensor, patch: int, dtype: torch.dtype) -> torch.Tensor:
    """``[n, h, w, 3]`` float32 (or ``dtype``) images -> ``[n, g, patch * patch * 3]`` tokens of ``dtype`` (``tia_vit_patchify_h``)."""
    from tiatoolbox_amd import _lib

    if not (x_nhwc.is_cuda and x_nhwc.dim() == 4 and x_nhwc.shape[-1] == 3 and x_nhwc.is_contiguous() and x_nhwc.dtype in (torch.float32, dtype)):
        msg = f"hip_vit_patchify_h expects a contiguous [n, h, w, 3] CUDA tensor in float32 or {dtype}; got {tuple(x_nhwc.shape)}, {x_nhwc.dtype}."
        raise ValueError(msg)
    n, h, w, _ = x_nhwc.shape
    out = torch.empty((n, (h // patch) * (w // patch), patch * patch * 3), dtype=dtype, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device):
        rc = _lib.load().tia_vit_patchify_h(x_nhwc.data_ptr(), _DT[x_nhwc.dtype], out.data_ptr(), n, h, w, patch, _DT[dtype],
                                            _lib.current_stream())
    _lib.check(rc, "tia_vit_patchify_h")
    return out


def hip_vit_assemble_tokens_h(tokens: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """``out[b, 0] = cls + pos[0]``, ``out[b, 1 + i] = tokens[b, i] + pos[1 + i]`` (float32 ``cls [D]`` / ``pos [1 + g, D]``)."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_vit_assemble_tokens_h", tokens)
    n, g, d = tokens.shape
    if cls.dtype != torch.float32 or pos.dtype != torch.float32 or cls.numel() != d or pos.numel() != (1 + g) * d or not (
            cls.is_contiguous() and pos.is_contiguous()):
        msg = f"hip_vit_assemble_tokens_h takes float32 cls [{d}] and pos [{1 + g}, {d}]; got {tuple(cls.shape)}, {tuple(pos.shape)}."
        raise ValueError(msg)
    out = torch.empty((n, 1 + g, d), dtype=tokens.dtype, device=tokens.device)
    with torch.cuda.device(tokens.device):
        rc = _lib.load().tia_vit_assemble_tokens_h(tokens.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), n, g, d,
                                                   _DT[tokens.dtype], _lib.current_stream())
    _lib.check(rc, "tia_vit_assemble_tokens_h")
    return out


def hip_swiglu_rows_h(x: torch.Tensor) -> torch.Tensor:
    """Packed SwiGLU ``silu(x[..., :H]) * x[..., H:]`` on ``[n, S, 2H]`` tokens -> ``[n, S, H]`` (``tia_swiglu_rows_h``)."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_swiglu_rows_h", x)
    if x.dim() < 2 or x.shape[-1] % 2 != 0:  # noqa: PLR2004
        msg = f"hip_swiglu_rows_h takes [..., 2H] tokens; got {tuple(x.shape)}."
        raise ValueError(msg)
    hidden = x.shape[-1] // 2
    y = torch.empty((*x.shape[:-1], hidden), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_swiglu_rows_h(x.data_ptr(), y.data_ptr(), x.numel() // (2 * hidden), hidden, _DT[x.dtype], _lib.current_stream())
    _lib.check(rc, "tia_swiglu_rows_h")
    return y


def padded_patch_columns(patch: int) -> int:
    """``k_pad``: ``3 * patch^2`` rounded up to the half GEMM's multiple of 32 input channels (patch 14: 588 -> 608)."""
    return -(-3 * patch * patch // 32) * 32


def hip_vit_patchify_pad_h(x_nhwc: torch.Tensor, patch: int, k_pad: int, dtype: torch.dtype) -> torch.Tensor:
    """``[n, h, w, 3]`` float32 (or ``dtype``) images -> ``[n, g, k_pad]`` tokens of ``dtype``, zeros from column ``3 * patch^2`` on
    (``tia_vit_patchify_pad_h``: any patch size)."""
    from tiatoolbox_amd import _lib

    if not (x_nhwc.is_cuda and x_nhwc.dim() == 4 and x_nhwc.shape[-1] == 3 and x_nhwc.is_contiguous() and x_nhwc.dtype in (torch.float32, dtype)):
        msg = f"hip_vit_patchify_pad_h expects a contiguous [n, h, w, 3] CUDA tensor in float32 or {dtype}; got {tuple(x_nhwc.shape)}, {x_nhwc.dtype}."
        raise ValueError(msg)
    n, h, w, _ = x_nhwc.shape
    out = torch.empty((n, (h // patch) * (w // patch), k_pad), dtype=dtype, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device):
        rc = _lib.load().tia_vit_patchify_pad_h(x_nhwc.data_ptr(), _DT[x_nhwc.dtype], out.data_ptr(), n, h, w, patch, k_pad, _DT[dtype],
                                                _lib.current_stream())
    _lib.check(rc, "tia_vit_patchify_pad_h")
    return out


def hip_vit_assemble_prefix_h(tokens: torch.Tensor, cls: torch.Tensor, reg: torch.Tensor | None, pos: torch.Tensor, *,
                              pos_has_cls: bool) -> torch.Tensor:
    """``out[b] = cat([cls (+ pos[0] if pos_has_cls), reg, tokens[b] + pos[pos_has_cls:]])`` (float32 ``cls [D]``, ``reg [R, D]`` or
    ``None``, ``pos [g + pos_has_cls, D]``): ``tia_vit_assemble_prefix_h``."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_vit_assemble_prefix_h", tokens)
    n, g, d = tokens.shape
    nreg = 0 if reg is None else reg.numel() // d
    rows = g + int(pos_has_cls)
    if cls.dtype != torch.float32 or pos.dtype != torch.float32 or cls.numel() != d or pos.numel() != rows * d or not (
            cls.is_contiguous() and pos.is_contiguous()) or (reg is not None and (
                reg.dtype != torch.float32 or not reg.is_contiguous() or nreg == 0 or reg.numel() != nreg * d)):
        msg = (f"hip_vit_assemble_prefix_h takes float32 cls [{d}], reg [R, {d}] or None and pos [{rows}, {d}]; got {tuple(cls.shape)}, "
               f"{None if reg is None else tuple(reg.shape)}, {tuple(pos.shape)}.")
        raise ValueError(msg)
    out = torch.empty((n, 1 + nreg + g, d), dtype=tokens.dtype, device=tokens.device)
    with torch.cuda.device(tokens.device):
        rc = _lib.load().tia_vit_assemble_prefix_h(tokens.data_ptr(), cls.data_ptr(), _ptr(reg), pos.data_ptr(), int(pos_has_cls),
                                                   out.data_ptr(), n, g, nreg, d, _DT[tokens.dtype], _lib.current_stream())
    _lib.check(rc, "tia_vit_assemble_prefix_h")
    return out


def hip_vit_cls_mean_pool_h(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, eps: float, skip: int) -> torch.Tensor:
    """``cat([LN(x[:, 0]), LN(x[:, skip:]).mean(1)], -1)`` of ``[n, S, D]`` tokens in float32, ``[n, 2D]`` (float32 affine; the
    normalised rows are not rounded to half): ``tia_vit_cls_mean_pool_h``."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_vit_cls_mean_pool_h", x)
    if x.dim() != 3 or gamma.dtype != torch.float32 or beta.dtype != torch.float32 or gamma.numel() != x.shape[-1] or \
            beta.numel() != x.shape[-1]:  # noqa: PLR2004
        msg = f"hip_vit_cls_mean_pool_h takes [n, S, D] tokens and a float32 affine of D values; got {tuple(x.shape)}, {tuple(gamma.shape)}."
        raise ValueError(msg)
    n, s, d = x.shape
    out = torch.empty((n, 2 * d), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_vit_cls_mean_pool_h(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(), n, s, skip, d,
                                                 _DT[x.dtype], _lib.current_stream())
    _lib.check(rc, "tia_vit_cls_mean_pool_h")
    return out


def hip_vit_patchify_norm_u8_h(x_u8_nhwc: torch.Tensor, table: torch.Tensor, patch: int, k_pad: int, dtype: torch.dtype) -> torch.Tensor:
    """``[n, h, w, 3]`` uint8 patches -> ``[n, g, k_pad]`` tokens of ``dtype`` with ``table[byte, channel]`` for every byte, zeros
    from column ``3 * patch^2`` on (``tia_vit_patchify_norm_u8_h``: ``ToTensor`` + ``Normalize`` as a ``[256, 3]`` table of ``dtype``).
    The batch may be a view that starts at any byte of a larger buffer."""
    from tiatoolbox_amd import _lib

    if not (x_u8_nhwc.is_cuda and x_u8_nhwc.dim() == 4 and x_u8_nhwc.shape[-1] == 3 and x_u8_nhwc.is_contiguous()  # noqa: PLR2004
            and x_u8_nhwc.dtype == torch.uint8):
        msg = f"hip_vit_patchify_norm_u8_h expects a contiguous [n, h, w, 3] uint8 CUDA tensor; got {tuple(x_u8_nhwc.shape)}, {x_u8_nhwc.dtype}."
        raise ValueError(msg)
    if not (dtype in _HALF and table.dtype == dtype and table.device == x_u8_nhwc.device and tuple(table.shape) == (256, 3)
            and table.is_contiguous()):
        msg = (f"hip_vit_patchify_norm_u8_h takes a contiguous [256, 3] fp16 / bf16 table of the tokens' dtype on the batch's device; got "
               f"{tuple(table.shape)}, {table.dtype} on {table.device} for {dtype}.")
        raise ValueError(msg)
    n, h, w, _ = x_u8_nhwc.shape
    out = torch.empty((n, (h // patch) * (w // patch), k_pad), dtype=dtype, device=x_u8_nhwc.device)
    with torch.cuda.device(x_u8_nhwc.device):
        rc = _lib.load().tia_vit_patchify_norm_u8_h(x_u8_nhwc.data_ptr(), table.data_ptr(), out.data_ptr(), n, h, w, patch, k_pad, _DT[dtype],
                                                    _lib.current_stream())
    _lib.check(rc, "tia_vit_patchify_norm_u8_h")
    return out


RESIDUAL_F32 = "float32"  # the one `residual_dtype` of `FusedViT.prepare` (and of the engines' run kwarg)


def _f32_stream(name: str, x: torch.Tensor) -> None:
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        msg = f"{name} expects a contiguous float32 CUDA tensor (the residual stream); got {tuple(x.shape)}, {x.dtype} on {x.device}."
        raise ValueError(msg)


def hip_add_layernorm_rows_f32(x: torch.Tensor, branch: torch.Tensor | None, gamma: torch.Tensor | None, beta: torch.Tensor | None, *,
                               eps: float, rows: int, row_stride: int, dtype: torch.dtype,
                               out_dtype: torch.dtype | None = None) -> torch.Tensor | None:
    """One pass over ``rows`` rows of ``c`` values that start ``row_stride`` elements apart in the float32 stream ``x`` (and in
    ``branch``, a half tensor of ``x``'s shape, or ``None``): ``x += branch.float()`` IN PLACE (one float32 add, never rounded), then
    the LayerNorm of the sum, ``[rows, c]`` in ``dtype`` (the graph's half type) or ``out_dtype=torch.float32``.  ``gamma=None``: the
    add alone, returns ``None``.  ``tia_add_layernorm_rows_f32``."""
    from tiatoolbox_amd import _lib

    _f32_stream("hip_add_layernorm_rows_f32", x)
    if dtype not in _HALF or (gamma is None) != (beta is None) or (gamma is None and branch is None):
        msg = f"hip_add_layernorm_rows_f32 takes a half `dtype`, and a branch, a float32 affine or both; got {dtype}."
        raise ValueError(msg)
    if branch is not None:
        _half_tokens("hip_add_layernorm_rows_f32 (branch)", branch)
        if branch.dtype != dtype or branch.shape != x.shape:
            msg = f"hip_add_layernorm_rows_f32: branch {tuple(branch.shape)}, {branch.dtype} beside a stream {tuple(x.shape)} for {dtype}."
            raise ValueError(msg)
    c = gamma.numel() if gamma is not None else x.shape[-1]  # (the add alone: rows of the stream's last dimension)
    if (rows - 1) * row_stride + c > x.numel() or (gamma is not None and (gamma.dtype != torch.float32 or beta.dtype != torch.float32
                                                                            or beta.numel() != c)):
        msg = f"hip_add_layernorm_rows_f32: {rows} rows of {c} at stride {row_stride} beyond {x.numel()} elements, or an affine that is not float32."
        raise ValueError(msg)
    out_dtype = out_dtype or dtype
    if out_dtype not in (dtype, torch.float32):
        msg = f"hip_add_layernorm_rows_f32 writes {dtype} or float32; got out_dtype {out_dtype}."
        raise ValueError(msg)
    y = torch.empty((rows, c), dtype=out_dtype, device=x.device) if gamma is not None else None
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_add_layernorm_rows_f32(x.data_ptr(), row_stride, _ptr(branch), row_stride, _ptr(gamma), _ptr(beta), float(eps),
                                                    _ptr(y), _DT[out_dtype], rows, c, _DT[dtype], _lib.current_stream())
    _lib.check(rc, "tia_add_layernorm_rows_f32")
    return y


def hip_vit_assemble_rows_f32(tokens: torch.Tensor, cls: torch.Tensor, reg: torch.Tensor | None, pos: torch.Tensor, *,
                              pos_has_cls: bool) -> torch.Tensor:
    """:func:`hip_vit_assemble_prefix_h` with a float32 result ``[n, 1 + R + g, D]``: ``tokens.float() + pos``, not rounded
    (``reg=None`` with ``pos_has_cls=True`` is the plain form).  ``tia_vit_assemble_rows_f32``."""
    from tiatoolbox_amd import _lib

    _half_tokens("hip_vit_assemble_rows_f32", tokens)
    n, g, d = tokens.shape
    nreg = 0 if reg is None else reg.numel() // d
    rows = g + int(pos_has_cls)
    if cls.dtype != torch.float32 or pos.dtype != torch.float32 or cls.numel() != d or pos.numel() != rows * d or not (
            cls.is_contiguous() and pos.is_contiguous()) or (reg is not None and (
                reg.dtype != torch.float32 or not reg.is_contiguous() or nreg == 0 or reg.numel() != nreg * d)):
        msg = (f"hip_vit_assemble_rows_f32 takes float32 cls [{d}], reg [R, {d}] or None and pos [{rows}, {d}]; got {tuple(cls.shape)}, "
               f"{None if reg is None else tuple(reg.shape)}, {tuple(pos.shape)}.")
        raise ValueError(msg)
    out = torch.empty((n, 1 + nreg + g, d), dtype=torch.float32, device=tokens.device)
    with torch.cuda.device(tokens.device):
        rc = _lib.load().tia_vit_assemble_rows_f32(tokens.data_ptr(), cls.data_ptr(), _ptr(reg), pos.data_ptr(), int(pos_has_cls),
                                                   out.data_ptr(), n, g, nreg, d, _DT[tokens.dtype], _lib.current_stream())
    _lib.check(rc, "tia_vit_assemble_rows_f32")
    return out


def hip_vit_cls_mean_pool_f32(x: torch.Tensor, branch: torch.Tensor | None, gamma: torch.Tensor, beta: torch.Tensor, *, eps: float,
                              skip: int, dtype: torch.dtype) -> torch.Tensor:
    """:func:`hip_vit_cls_mean_pool_h` of the float32 stream ``[n, S, D]`` with the last ``branch`` (half ``dtype``, same shape, or
    ``None``) added on load and not written back: ``tia_vit_cls_mean_pool_f32``."""
    from tiatoolbox_amd import _lib

    _f32_stream("hip_vit_cls_mean_pool_f32", x)
    if x.dim() != 3 or dtype not in _HALF or gamma.dtype != torch.float32 or beta.dtype != torch.float32 or \
            gamma.numel() != x.shape[-1] or beta.numel() != x.shape[-1]:  # noqa: PLR2004
        msg = (f"hip_vit_cls_mean_pool_f32 takes a [n, S, D] stream, a half `dtype` and a float32 affine of D values; got {tuple(x.shape)}, "
               f"{dtype}, {tuple(gamma.shape)}.")
        raise ValueError(msg)
    if branch is not None:
        _half_tokens("hip_vit_cls_mean_pool_f32 (branch)", branch)
        if branch.dtype != dtype or branch.shape != x.shape:
            msg = f"hip_vit_cls_mean_pool_f32: branch {tuple(branch.shape)}, {branch.dtype} beside a stream {tuple(x.shape)} for {dtype}."
            raise ValueError(msg)
    n, s, d = x.shape
    out = torch.empty((n, 2 * d), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_vit_cls_mean_pool_f32(x.data_ptr(), _ptr(branch), gamma.data_ptr(), beta.data_ptr(), float(eps), out.data_ptr(),
                                                   n, s, skip, d, _DT[dtype], _lib.current_stream())
    _lib.check(rc, "tia_vit_cls_mean_pool_f32")
    return out


HEAD_MAX_CLASSES, HEAD_MAX_FEATURES = 64, 8192  # what tia_linear_softmax_rows_f32 takes (one lane per class; the widest LayerNorm row)


def hip_linear_softmax_rows_f32(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """``softmax(x @ weight^T + bias, -1)`` of float32 rows ``[rows, f]`` (the rows may be a view at a stride) with ``weight [c, f]``,
    ``bias [c]`` or ``None``: float32 throughout, ``[rows, c]`` (``tia_linear_softmax_rows_f32``)."""
    from tiatoolbox_amd import _lib

    if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1 and weight.dim() == 2  # noqa: PLR2004
            and weight.dtype == torch.float32 and weight.is_contiguous() and weight.device == x.device and weight.shape[1] == x.shape[1]
            and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.device == x.device
                                  and bias.numel() == weight.shape[0]))):
        msg = (f"hip_linear_softmax_rows_f32 takes float32 CUDA rows [rows, f], a contiguous weight [c, f] and a bias [c] or None; got "
               f"{tuple(x.shape)}, {x.dtype} on {x.device}, {tuple(weight.shape)}, {None if bias is None else tuple(bias.shape)}.")
        raise ValueError(msg)
    rows, f = x.shape
    c = weight.shape[0]
    stride = x.stride(0) if rows > 1 else f
    out = torch.empty((rows, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_linear_softmax_rows_f32(x.data_ptr(), stride, weight.data_ptr(), _ptr(bias), out.data_ptr(), rows, f, c,
                                                     _lib.current_stream())
    _lib.check(rc, "tia_linear_softmax_rows_f32")
    return out


SWIGLU_PAD_FLOOR = 512  # halves narrower than this are not padded: the waste is bounded by 31 / 512, and narrow layers stay refused


def padded_swiglu_half(half: int) -> int:
    """The width each half of a packed SwiGLU ``fc1`` is padded to: ``half`` itself on the half GEMM's multiple of 32 or below
    ``SWIGLU_PAD_FLOOR``, else the next multiple of 32 (Virchow: 3416 -> 3424, ``fc1`` 6832 -> 6848)."""
    if half % 32 == 0 or half < SWIGLU_PAD_FLOOR:
        return half
    return -(-half // 32) * 32


def pad_swiglu(fc1_w: torch.Tensor, fc1_b: torch.Tensor, fc2_w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Float32 ``fc1 [2H, D]``, its bias and the (LayerScale-folded) ``fc2 [D, H]`` with each half padded to ``H_pad =
    padded_swiglu_half(H)``: gate rows ``[0, H)``, zero rows and zero bias ``[H, H_pad)``, value rows ``[H_pad, H_pad + H)``, zeros
    after; ``fc2`` gets zero columns.  A pad lane computes ``silu(0) * 0 = 0`` exactly and meets a zero weight."""
    half = fc2_w.shape[1]
    pad = padded_swiglu_half(half) - half
    if pad == 0:
        return fc1_w, fc1_b, fc2_w
    zw, zb = fc1_w.new_zeros((pad, fc1_w.shape[1])), fc1_b.new_zeros(pad)
    fc1_w = torch.cat([fc1_w[:half], zw, fc1_w[half:], zw], dim=0).contiguous()
    fc1_b = torch.cat([fc1_b[:half], zb, fc1_b[half:], zb]).contiguous()
    return fc1_w, fc1_b, torch.nn.functional.pad(fc2_w, (0, pad)).contiguous()


FP8_LINEAR = "float8_e4m3"  # the one `linear_dtype` of `FusedViT.prepare` (and the engines' `compute_dtype` that selects it)
E4M3_MAX = 448.0            # largest finite value of OCP e4m3fn


class QuantRows(NamedTuple):
    """Rows quantised by :func:`quantize_rows_e4m3`'s recipe: ``codes [..., K]`` (e4m3fn bytes as uint8) and ``scales`` (float32, one
    per row, flat) -- or by :func:`quantize_rows_int8`'s, with ``torch.int8`` codes: the dtype of ``codes`` tells the two apart."""

    codes: torch.Tensor
    scales: torch.Tensor


def quantize_rows_e4m3(v: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The FP8 route's recipe for one row ``v[..., :]`` of float32 values, in torch operations (the statement the kernels of
    ``vit_fp8.hip`` are tested against): ``amax = max |v|``; ``inv = 448 / amax`` and ``s = amax / 448``, one float32 division each
    (``amax == 0``: ``inv = s = 1``); ``q = e4m3(v * inv)`` with the product in float32 and the conversion to OCP ``e4m3fn`` rounding
    to nearest even and saturating at +-448 (torch's CPU conversion, which makes a NaN only beyond what the clamp leaves).
    Returns ``(q [..., K] torch.float8_e4m3fn, s [...] float32)``; ``q.float() * s[..., None]`` is the dequantised row."""
    v = v.to(torch.float32)
    amax = v.abs().amax(dim=-1, keepdim=True)
    top, one = torch.tensor(E4M3_MAX, dtype=torch.float32, device=v.device), torch.ones((), dtype=torch.float32, device=v.device)
    inv = torch.where(amax > 0, top / amax, one)
    s = torch.where(amax > 0, amax / top, one)
    q = (v * inv).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q, s.squeeze(-1)


class _QuantFormat(NamedTuple):
    """One 8-bit format of the quantised linear layers: its name in messages, the dtype of its codes, its ``linear_dtype`` and the
    module-level names of its five wrappers.  The wrappers' messages carry these names, and the graph finds a wrapper through ``fn``
    when it calls it: by its name in this module, so that a replaced module attribute is what runs."""

    name: str
    codes: torch.dtype
    linear_dtype: str
    serves: str
    pack: str
    linear: str
    layernorm: str
    act: str

    def fn(self, which: str):  # noqa: ANN201
        return globals()[getattr(self, which)]


def _linear_serves(entry: str, cout: int, cin: int) -> bool:
    from tiatoolbox_amd import _lib

    return getattr(_lib.load(), entry)(1, cout, cin) == 1


def _pack_linear_weights(fmt: _QuantFormat, entry: str, weight: torch.Tensor) -> QuantRows:
    from tiatoolbox_amd import _lib

    w = weight.detach().to(torch.float32).contiguous()
    if not w.is_cuda or w.dim() != 2:  # noqa: PLR2004
        msg = f"{fmt.pack} packs CUDA weights [cout, cin]; got {tuple(w.shape)} on {w.device}."
        raise ValueError(msg)
    cout, cin = w.shape
    codes = torch.empty((cout, cin), dtype=fmt.codes, device=w.device)
    scales = torch.empty((cout,), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = getattr(_lib.load(), entry)(w.data_ptr(), cout, cin, codes.data_ptr(), scales.data_ptr(), _lib.current_stream())
    _lib.check(rc, entry)
    return QuantRows(codes, scales)


def _linear_quant_rows(fmt: _QuantFormat, entry: str, a: QuantRows, w: QuantRows, bias: torch.Tensor | None,
                       residual: torch.Tensor | None, dtype: torch.dtype) -> torch.Tensor:
    from tiatoolbox_amd import _lib

    n, s, cin = a.codes.shape
    cout = w.codes.shape[0]
    if not (a.codes.is_cuda and a.codes.dtype == fmt.codes and a.codes.is_contiguous() and w.codes.dtype == fmt.codes
            and w.codes.shape[1] == cin and a.scales.dtype == torch.float32 and a.scales.numel() == n * s and dtype in _HALF
            and (bias is None or bias.dtype == torch.float32)):
        msg = (f"{fmt.linear} takes {str(fmt.codes).removeprefix('torch.')} CUDA codes [n, S, cin] with n * S float32 scales, weights "
               f"[cout, cin] and a float32 bias; "
               f"got {tuple(a.codes.shape)}, {a.codes.dtype} beside {tuple(w.codes.shape)}, {w.codes.dtype} for {dtype}.")
        raise ValueError(msg)
    if residual is not None:
        _half_tokens(f"{fmt.linear} (residual)", residual, cout)
        if residual.dtype != dtype or tuple(residual.shape[:2]) != (n, s):
            msg = f"{fmt.linear}: residual {tuple(residual.shape)}, {residual.dtype} beside tokens {(n, s, cin)} for {dtype}."
            raise ValueError(msg)
    y = torch.empty((n, s, cout), dtype=dtype, device=a.codes.device)
    with torch.cuda.device(y.device):
        rc = getattr(_lib.load(), entry)(a.codes.data_ptr(), a.scales.data_ptr(), w.codes.data_ptr(), w.scales.data_ptr(), _ptr(bias),
                                         _ptr(residual), y.data_ptr(), n * s, cout, cin, _DT[dtype], _lib.current_stream())
    _lib.check(rc, entry)
    return y


def _layernorm_quant_rows(fmt: _QuantFormat, entry: str, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> QuantRows:
    from tiatoolbox_amd import _lib

    _half_tokens(fmt.layernorm, x, gamma.numel())
    if x.dim() != 3 or gamma.dtype != torch.float32 or beta.dtype != torch.float32 or beta.numel() != gamma.numel():  # noqa: PLR2004
        msg = f"{fmt.layernorm} takes [n, S, D] tokens and a float32 affine of D values; got {tuple(x.shape)}, {tuple(gamma.shape)}."
        raise ValueError(msg)
    n, s, d = x.shape
    codes = torch.empty((n, s, d), dtype=fmt.codes, device=x.device)
    scales = torch.empty((n * s,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = getattr(_lib.load(), entry)(x.data_ptr(), d, gamma.data_ptr(), beta.data_ptr(), float(eps), codes.data_ptr(),
                                         scales.data_ptr(), n * s, d, _DT[x.dtype], _lib.current_stream())
    _lib.check(rc, entry)
    return QuantRows(codes, scales)


def _act_quant_rows(fmt: _QuantFormat, gelu_entry: str, swiglu_entry: str, x: torch.Tensor, swiglu: bool) -> QuantRows:  # noqa: FBT001
    from tiatoolbox_amd import _lib

    _half_tokens(fmt.act, x)
    if x.dim() != 3 or (swiglu and x.shape[-1] % 2 != 0):  # noqa: PLR2004
        msg = f"{fmt.act} takes [n, S, H] (GELU) or [n, S, 2H] (SwiGLU) tokens; got {tuple(x.shape)}."
        raise ValueError(msg)
    n, s, c = x.shape
    hidden = c // 2 if swiglu else c
    codes = torch.empty((n, s, hidden), dtype=fmt.codes, device=x.device)
    scales = torch.empty((n * s,), dtype=torch.float32, device=x.device)
    entry = swiglu_entry if swiglu else gelu_entry
    launch = getattr(_lib.load(), entry)
    with torch.cuda.device(x.device):
        rc = launch(x.data_ptr(), codes.data_ptr(), scales.data_ptr(), n * s, hidden, _DT[x.dtype], _lib.current_stream())
    _lib.check(rc, entry)
    return QuantRows(codes, scales)


class _LinearQuant:
    """One GEMM of the graph on a quantised kernel of format ``fmt``: weights quantised per output channel in ``prepare`` from the
    float32 (folded, padded) ones, the float32 bias throughout; called on :class:`QuantRows` from a quantising producer."""

    fmt: _QuantFormat

    def __init__(self, name: str, weight: torch.Tensor, bias: torch.Tensor) -> None:
        self.name, self.weight32, self.bias32 = name, weight, bias
        self.cout, self.cin = weight.shape
        self.packed: QuantRows | None = None
        self.dtype: torch.dtype | None = None

    def prepare(self, dtype: torch.dtype) -> None:
        self.packed, self.dtype = self.fmt.fn("pack")(self.weight32), dtype
        self.weight32 = None

    def __call__(self, a: QuantRows, residual: torch.Tensor | None = None) -> torch.Tensor:
        return self.fmt.fn("linear")(a, self.packed, self.bias32, residual, dtype=self.dtype)


_FP8 = _QuantFormat("FP8", torch.uint8, FP8_LINEAR, "linear_fp8_serves", "pack_linear_weights_fp8", "hip_linear_fp8_rows",
                    "hip_layernorm_rows_q8", "hip_act_rows_q8")


def linear_fp8_serves(cout: int, cin: int) -> bool:
    """Whether a ``cin -> cout`` Linear goes to the FP8 GEMM (``tia_linear_fp8_serves``, answered on the host)."""
    return _linear_serves("tia_linear_fp8_serves", cout, cin)


def pack_linear_weights_fp8(weight: torch.Tensor) -> QuantRows:
    """Float32 ``[cout, cin]`` -> ``tia_linear_fp8_rows``'s weight operand: codes ``[cout, cin]`` and one scale per output channel,
    quantised on the device (``tia_linear_fp8_pack_weights``)."""
    return _pack_linear_weights(_FP8, "tia_linear_fp8_pack_weights", weight)


def hip_linear_fp8_rows(a: QuantRows, w: QuantRows, bias: torch.Tensor | None, residual: torch.Tensor | None = None, *,
                        dtype: torch.dtype) -> torch.Tensor:
    """``half_rne(acc * sa * sw + bias (+ residual))`` of quantised tokens ``[n, S, cin]`` and weights ``[cout, cin]``:
    ``tia_linear_fp8_rows`` -> ``[n, S, cout]`` of ``dtype``."""
    return _linear_quant_rows(_FP8, "tia_linear_fp8_rows", a, w, bias, residual, dtype)


def hip_layernorm_rows_q8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, eps: float) -> QuantRows:
    """LayerNorm of every row of ``[n, S, D]`` tokens, quantised from its float32 values (``tia_layernorm_rows_q8``)."""
    return _layernorm_quant_rows(_FP8, "tia_layernorm_rows_q8", x, gamma, beta, eps)


def hip_act_rows_q8(x: torch.Tensor, *, swiglu: bool) -> QuantRows:
    """The activation between ``fc1`` and ``fc2`` on ``[n, S, H]`` (exact GELU) or ``[n, S, 2H]`` (packed SwiGLU, the first half the
    gate) tokens, quantised from its float32 values: ``[n, S, H]`` codes (``tia_gelu_rows_q8`` / ``tia_swiglu_rows_q8``)."""
    return _act_quant_rows(_FP8, "tia_gelu_rows_q8", "tia_swiglu_rows_q8", x, swiglu)


def pad_swiglu_to(fc1_w: torch.Tensor, fc1_b: torch.Tensor, fc2_w: torch.Tensor, target: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``pad_swiglu``'s zero lanes up to ``target`` columns per half (the FP8 GEMM's multiple of 128; Virchow: 3424 -> 3456), applied to
    an ``fc1 [2H, D]`` / ``fc2 [D, H]`` pair that may already carry that function's padding: a pad lane is exact either way."""
    half = fc2_w.shape[1]
    pad = target - half
    if pad <= 0:
        return fc1_w, fc1_b, fc2_w
    zw, zb = fc1_w.new_zeros((pad, fc1_w.shape[1])), fc1_b.new_zeros(pad)
    fc1_w = torch.cat([fc1_w[:half], zw, fc1_w[half:], zw], dim=0).contiguous()
    fc1_b = torch.cat([fc1_b[:half], zb, fc1_b[half:], zb]).contiguous()
    return fc1_w, fc1_b, torch.nn.functional.pad(fc2_w, (0, pad)).contiguous()


class _LinearFp8(_LinearQuant):
    """:class:`_LinearQuant` on the FP8 kernel."""

    fmt = _FP8


INT8_LINEAR = "int8"  # the other quantised `linear_dtype` of `FusedViT.prepare` (and the engines' `compute_dtype` that selects it)
INT8_MAX = 127.0      # the symmetric code range: -128 is never produced


def quantize_rows_int8(v: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The INT8 route's recipe for one row ``v[..., :]`` of float32 values, in torch operations (the statement the kernels of
    ``vit_int8.hip`` are tested against): ``amax = max |v|`` (a NaN in the row makes it NaN); ``inv = 127 / amax`` and
    ``s = amax / 127``, one float32 division each (``amax == 0``: ``inv = s = 1``); ``q = clamp(rne(v * inv), -127, 127)`` with the
    product in float32 and rounding to nearest even; a NaN product is code 0.  A row holding NaN so gets ``s = NaN``, a row holding
    ``+-inf`` ``s = inf``, and either way codes inside ``[-127, 127]``.
    Returns ``(q [..., K] torch.int8, s [...] float32)``; ``q.float() * s[..., None]`` is the dequantised row."""
    v = v.to(torch.float32)
    amax = v.abs().amax(dim=-1, keepdim=True)
    top, one = torch.tensor(INT8_MAX, dtype=torch.float32, device=v.device), torch.ones((), dtype=torch.float32, device=v.device)
    inv = torch.where(amax == 0, one, top / amax)
    s = torch.where(amax == 0, one, amax / top)
    q = torch.round(v * inv)
    q = torch.where(torch.isnan(q), torch.zeros_like(q), q).clamp(-INT8_MAX, INT8_MAX).to(torch.int8)
    return q, s.squeeze(-1)


_INT8 = _QuantFormat("INT8", torch.int8, INT8_LINEAR, "linear_int8_serves", "pack_linear_weights_int8", "hip_linear_int8_rows",
                     "hip_layernorm_rows_qi8", "hip_act_rows_qi8")


def linear_int8_serves(cout: int, cin: int) -> bool:
    """Whether a ``cin -> cout`` Linear goes to the INT8 GEMM (``tia_linear_int8_serves``, answered on the host)."""
    return _linear_serves("tia_linear_int8_serves", cout, cin)


def pack_linear_weights_int8(weight: torch.Tensor) -> QuantRows:
    """Float32 ``[cout, cin]`` -> ``tia_linear_int8_rows``'s weight operand: ``torch.int8`` codes ``[cout, cin]`` and one scale per
    output channel, quantised on the device (``tia_linear_int8_pack_weights``)."""
    return _pack_linear_weights(_INT8, "tia_linear_int8_pack_weights", weight)


def hip_linear_int8_rows(a: QuantRows, w: QuantRows, bias: torch.Tensor | None, residual: torch.Tensor | None = None, *,
                         dtype: torch.dtype) -> torch.Tensor:
    """``half_rne(float(acc) * sa * sw + bias (+ residual))`` of quantised tokens ``[n, S, cin]`` and weights ``[cout, cin]``, both
    ``torch.int8`` codes (the FP8 route's uint8 codes are refused): ``tia_linear_int8_rows`` -> ``[n, S, cout]`` of ``dtype``."""
    if a.codes.dtype != torch.int8 or w.codes.dtype != torch.int8:  # (before anything else: FP8 codes are another number format)
        msg = (f"hip_linear_int8_rows takes torch.int8 codes (quantize_rows_int8's recipe) for tokens and weights; got {a.codes.dtype} "
               f"beside {w.codes.dtype}.")
        raise ValueError(msg)
    return _linear_quant_rows(_INT8, "tia_linear_int8_rows", a, w, bias, residual, dtype)


def hip_layernorm_rows_qi8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, eps: float) -> QuantRows:
    """LayerNorm of every row of ``[n, S, D]`` tokens, quantised to int8 from its float32 values (``tia_layernorm_rows_qi8``)."""
    return _layernorm_quant_rows(_INT8, "tia_layernorm_rows_qi8", x, gamma, beta, eps)


def hip_act_rows_qi8(x: torch.Tensor, *, swiglu: bool) -> QuantRows:
    """The activation between ``fc1`` and ``fc2`` on ``[n, S, H]`` (exact GELU) or ``[n, S, 2H]`` (packed SwiGLU, the first half the
    gate) tokens, quantised to int8 from its float32 values: ``[n, S, H]`` codes (``tia_gelu_rows_qi8`` / ``tia_swiglu_rows_qi8``)."""
    return _act_quant_rows(_INT8, "tia_gelu_rows_qi8", "tia_swiglu_rows_qi8", x, swiglu)


def _smooth_vector(name: str, what: str, v: torch.Tensor, x: torch.Tensor, width: int) -> None:
    if not (v.is_cuda and v.device == x.device and v.dtype == torch.float32 and v.dim() == 1 and v.numel() == width and v.is_contiguous()):
        msg = f"{name} takes {what} as {width} contiguous float32 values on {x.device}; got {tuple(v.shape)}, {v.dtype} on {v.device}."
        raise ValueError(msg)


def hip_act_rows_qi8_smooth(x: torch.Tensor, inv_smooth: torch.Tensor, *, swiglu: bool) -> QuantRows:
    """:func:`hip_act_rows_qi8` with the float32 activation multiplied by ``inv_smooth[channel]`` (float32 ``[H]``) before the row
    maximum and the codes (``tia_gelu_rows_qi8_smooth`` / ``tia_swiglu_rows_qi8_smooth``): ``fc2``'s producer under smoothing."""
    from tiatoolbox_amd import _lib

    name = "hip_act_rows_qi8_smooth"
    _half_tokens(name, x)
    if x.dim() != 3 or (swiglu and x.shape[-1] % 2 != 0):  # noqa: PLR2004
        msg = f"{name} takes [n, S, H] (GELU) or [n, S, 2H] (SwiGLU) tokens; got {tuple(x.shape)}."
        raise ValueError(msg)
    n, s, c = x.shape
    hidden = c // 2 if swiglu else c
    _smooth_vector(name, "inv_smooth", inv_smooth, x, hidden)
    codes = torch.empty((n, s, hidden), dtype=torch.int8, device=x.device)
    scales = torch.empty((n * s,), dtype=torch.float32, device=x.device)
    entry = "tia_swiglu_rows_qi8_smooth" if swiglu else "tia_gelu_rows_qi8_smooth"
    with torch.cuda.device(x.device):
        rc = getattr(_lib.load(), entry)(x.data_ptr(), inv_smooth.data_ptr(), codes.data_ptr(), scales.data_ptr(), n * s, hidden,
                                         _DT[x.dtype], _lib.current_stream())
    _lib.check(rc, entry)
    return QuantRows(codes, scales)


def hip_layernorm_rows_absmax_h(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, amax: torch.Tensor, *, eps: float) -> torch.Tensor:
    """``amax[j] = max(amax[j], max |LayerNorm(x)[.., j]|)`` over every row of ``[n, S, D]`` tokens, of the float32 values
    :func:`hip_layernorm_rows_qi8` quantises (``tia_layernorm_rows_absmax_h``).  ``amax`` (float32 ``[D]``, zeroed by the caller) is
    updated in place and returned; a NaN stays in its column."""
    from tiatoolbox_amd import _lib

    name = "hip_layernorm_rows_absmax_h"
    _half_tokens(name, x, gamma.numel())
    if x.dim() != 3 or gamma.dtype != torch.float32 or beta.dtype != torch.float32 or beta.numel() != gamma.numel():  # noqa: PLR2004
        msg = f"{name} takes [n, S, D] tokens and a float32 affine of D values; got {tuple(x.shape)}, {tuple(gamma.shape)}."
        raise ValueError(msg)
    n, s, d = x.shape
    _smooth_vector(name, "amax", amax, x, d)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_layernorm_rows_absmax_h(x.data_ptr(), d, gamma.data_ptr(), beta.data_ptr(), float(eps), amax.data_ptr(), n * s, d,
                                                     _DT[x.dtype], _lib.current_stream())
    _lib.check(rc, "tia_layernorm_rows_absmax_h")
    return amax


def hip_act_rows_absmax_h(x: torch.Tensor, amax: torch.Tensor, *, swiglu: bool) -> torch.Tensor:
    """The same statistics of the float32 values :func:`hip_act_rows_qi8` quantises, on ``[n, S, H]`` (exact GELU) or ``[n, S, 2H]``
    (packed SwiGLU) tokens: ``amax`` float32 ``[H]`` (``tia_gelu_rows_absmax_h`` / ``tia_swiglu_rows_absmax_h``)."""
    from tiatoolbox_amd import _lib

    name = "hip_act_rows_absmax_h"
    _half_tokens(name, x)
    if x.dim() != 3 or (swiglu and x.shape[-1] % 2 != 0):  # noqa: PLR2004
        msg = f"{name} takes [n, S, H] (GELU) or [n, S, 2H] (SwiGLU) tokens; got {tuple(x.shape)}."
        raise ValueError(msg)
    n, s, c = x.shape
    hidden = c // 2 if swiglu else c
    _smooth_vector(name, "amax", amax, x, hidden)
    entry = "tia_swiglu_rows_absmax_h" if swiglu else "tia_gelu_rows_absmax_h"
    with torch.cuda.device(x.device):
        rc = getattr(_lib.load(), entry)(x.data_ptr(), amax.data_ptr(), n * s, hidden, _DT[x.dtype], _lib.current_stream())
    _lib.check(rc, entry)
    return amax


SMOOTH_EXP_MAX = 24  # the smoothing scales are 2^e with |e| <= 24


def int8_smoothing_scales(amax_x: torch.Tensor, amax_w: torch.Tensor, alpha: float = 0.5) -> torch.Tensor:
    """The smoothing scale of every input channel of one INT8 layer (SmoothQuant's balance between activation and weight ranges, on
    powers of two): ``s[j] = 2^clamp(round(alpha log2 a[j] - (1 - alpha) log2 w[j]), -24, 24)`` in float64, with
    ``a = amax_x`` the calibrated abs-max of the layer's float32 input per channel and ``w = amax_w = max_o |W[o, j]|`` of the
    float32 weights that are packed; ``s[j] = 1`` where ``a[j] == 0`` or ``w[j] == 0`` (a SwiGLU pad lane).  A power of two makes
    ``x / s`` and ``W * s`` exact in float32.  ``alpha`` in (0, 1]; a non-finite ``amax_x`` is a ``ValueError`` (the calibration data
    produced non-finite activations).  Returns float32 ``[K]`` on the CPU."""
    alpha = _checked_alpha(alpha)
    a, w = amax_x.detach().double().cpu().reshape(-1), amax_w.detach().double().cpu().reshape(-1)
    if a.numel() != w.numel():
        msg = f"int8_smoothing_scales: {a.numel()} activation maxima beside {w.numel()} weight columns."
        raise ValueError(msg)
    if not bool(torch.isfinite(a).all()) or bool((a < 0).any()):
        msg = (f"int8_smoothing_scales: {int((~torch.isfinite(a)).sum())} of {a.numel()} calibrated activation maxima are not finite "
               "(the calibration data produced non-finite activations).")
        raise ValueError(msg)
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        msg = "int8_smoothing_scales: the weight column maxima must be finite and non-negative."
        raise ValueError(msg)
    live = (a > 0) & (w > 0)
    one = torch.ones_like(a)
    e = alpha * torch.log2(torch.where(live, a, one)) - (1.0 - alpha) * torch.log2(torch.where(live, w, one))
    e = torch.round(e).clamp(-SMOOTH_EXP_MAX, SMOOTH_EXP_MAX)
    return torch.where(live, torch.exp2(e), one).to(torch.float32)


def _checked_alpha(alpha) -> float:  # noqa: ANN001
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 < float(alpha) <= 1.0:
        msg = f"int8 smoothing: alpha lies in (0, 1] (0.5 balances activations and weights); got {alpha!r}."
        raise ValueError(msg)
    return float(alpha)


def _checked_smoothing_scale(name: str, s: torch.Tensor, width: int) -> torch.Tensor:
    """One layer's entry of a ``smoothing`` dict as float32 ``[width]`` on the CPU, or the ``ValueError`` that names it."""
    if not isinstance(s, torch.Tensor) or s.dim() != 1 or s.numel() != width or not s.is_floating_point():
        got = f"{tuple(s.shape)}, {s.dtype}" if isinstance(s, torch.Tensor) else type(s).__name__
        msg = f"FusedViT.prepare: smoothing[{name!r}] must hold one floating-point scale per input channel, [{width}]; got {got}."
        raise ValueError(msg)
    s = s.detach().to(torch.float32).cpu().contiguous()
    mantissa, _ = torch.frexp(s)
    bad = ~(torch.isfinite(s) & (s > 0) & (mantissa == 0.5))  # noqa: PLR2004
    if bool(bad.any()):
        j = int(torch.nonzero(bad)[0])
        msg = (f"FusedViT.prepare: smoothing[{name!r}] must hold finite positive powers of two (they keep x / s and W * s exact); "
               f"channel {j} is {float(s[j])!r} ({int(bad.sum())} such of {width}).")
        raise ValueError(msg)
    return s


class _LinearInt8(_LinearQuant):
    """:class:`_LinearQuant` on the INT8 kernel, called on int8 :class:`QuantRows`.  ``inv_smooth`` (float32 ``[cin]``) is set on an
    ``fc2`` whose producer applies the layer's smoothing scales (``hip_act_rows_qi8_smooth``)."""

    fmt = _INT8
    inv_smooth: torch.Tensor | None = None


class _Linear:
    """One GEMM of the graph: the float32 (LayerScale-folded) weights until ``prepare`` packs them, the float32 bias throughout.
    Plain attributes: the cast of the surrounding module does not reach them."""

    def __init__(self, name: str, weight: torch.Tensor, bias: torch.Tensor) -> None:
        self.name, self.weight32, self.bias32 = name, weight, bias
        self.cout, self.cin = weight.shape
        self.packed: torch.Tensor | None = None
        if self.cin % 32 != 0 or self.cout % 64 != 0:
            msg = (f"FusedViT: the half GEMM takes cin % 32 == 0 and cout % 64 == 0; `{name}` is {self.cin} -> {self.cout}.")
            raise UnsupportedLayerError(msg)

    def prepare(self, dtype: torch.dtype) -> None:
        self.packed = pack_linear_weights_h(self.weight32, dtype)
        self.weight32 = None  # (the rounded, packed form is all the forward reads)

    def __call__(self, x: torch.Tensor, residual: torch.Tensor | None = None) -> torch.Tensor:
        return hip_linear_h(x, self.packed, self.bias32, residual, cout=self.cout)


SPLIT_LINEAR = "bfloat16x3"  # the `linear_dtype` of the float32 route (and the engines' `compute_dtype` that selects it)


def _f32_tokens(name: str, x: torch.Tensor, last: int | None = None) -> None:
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and (last is None or x.shape[-1] == last)):
        msg = f"{name} expects a contiguous float32 CUDA tensor" + (f" with {last} channels" if last is not None else "") + \
              f"; got {tuple(x.shape)}, {x.dtype} on {x.device}."
        raise ValueError(msg)


def pack_linear_weights_split(weight: torch.Tensor) -> torch.Tensor | None:
    """Float32 ``[cout, cin]`` -> the split GEMM's operand ``[1, 1, cin / 16, cout / 128, 3, 2, 128, 8]`` bf16: the planes ``hi``,
    ``mid``, ``lo`` of ``fused.split_stem_weights`` (``hi + mid + lo == w`` bit for bit) laid out by ``tia_conv_pack_weights_bf16x3``
    with a 1x1 window.  ``None`` when the shape is off that kernel's (``cin % 16``, ``cout % 128``) or the weights have no exact split
    into normal bf16 numbers (non-finite or extreme exponents): the caller then keeps the float32 GEMM."""
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.fused import split_stem_weights

    w = weight.detach().to(torch.float32).contiguous()
    cout, cin = w.shape
    if cin % 16 or cout % 128:
        return None
    parts, usable = split_stem_weights(w)
    if not usable:
        return None
    parts = parts.contiguous()  # [3, cout, cin] == [3, cout, cin, 1, 1]
    out = torch.empty((1, 1, cin // 16, cout // 128, 3, 2, 128, 8), dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_conv_pack_weights_bf16x3(parts.data_ptr(), cout, cin, 1, 1, out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_conv_pack_weights_bf16x3")
    return out


def pack_linear_weights_f32(weight: torch.Tensor) -> torch.Tensor:
    """Float32 ``[cout, cin]`` -> the float32 GEMM's operand ``[1, 1, cin, cout]`` (``tia_conv_pack_weights_f32``)."""
    from tiatoolbox_amd import _lib

    w = weight.detach().to(torch.float32).contiguous()
    cout, cin = w.shape
    out = torch.empty((1, 1, cin, cout), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        rc = _lib.load().tia_conv_pack_weights_f32(w.data_ptr(), cout, cin, 1, 1, out.data_ptr(), _lib.current_stream())
    _lib.check(rc, "tia_conv_pack_weights_f32")
    return out


def hip_linear_f32(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor | None, residual: torch.Tensor | None = None, *,
                   cout: int) -> torch.Tensor:
    """``x @ W^T + bias (+ residual)`` on ``[n, S, cin]`` float32 tokens, float32 out: a 1x1 window on the ``[n, S, 1, cin]`` map.
    bf16 weights from :func:`pack_linear_weights_split` go to ``tia_conv2d_bf16x3_nhwc_f32`` (both operands split into three bf16
    numbers, float32 accumulation), float32 weights from :func:`pack_linear_weights_f32` to ``tia_conv2d_nhwc_f32``."""
    from tiatoolbox_amd import _lib

    _f32_tokens("hip_linear_f32", x)
    n, s, cin = x.shape
    if residual is not None:
        _f32_tokens("hip_linear_f32 (residual)", residual, cout)
        if residual.shape[:2] != x.shape[:2]:
            msg = f"hip_linear_f32: residual {tuple(residual.shape)} beside tokens {tuple(x.shape)}."
            raise ValueError(msg)
    split = w_packed.dtype == torch.bfloat16
    want = (1, 1, cin // 16, cout // 128, 3, 2, 128, 8) if split else (1, 1, cin, cout)
    if tuple(w_packed.shape) != want or w_packed.dtype not in (torch.bfloat16, torch.float32) or not w_packed.is_contiguous() or (
            bias is not None and bias.dtype != torch.float32):
        msg = (f"hip_linear_f32: weights {tuple(w_packed.shape)}, {w_packed.dtype} are not pack_linear_weights_split's or "
               f"pack_linear_weights_f32's for {cin} -> {cout}, or a bias that is not float32.")
        raise ValueError(msg)
    y = torch.empty((n, s, cout), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        if split:
            rc = lib.tia_conv2d_bf16x3_nhwc_f32(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), n, s, 1, cin,
                                                cout, 1, 1, 1, 0, 0, 0, _lib.current_stream())
        else:
            rc = lib.tia_conv2d_nhwc_f32(x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), n, s, 1, cin, cout,
                                         1, 1, 1, 0, 0, _lib.current_stream())
    _lib.check(rc, "tia_conv2d_bf16x3_nhwc_f32" if split else "tia_conv2d_nhwc_f32")
    return y


def hip_mha_fwd_f32(qkv: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """Attention on the qkv Linear's float32 output ``[n, S, 3 * heads * hd]`` -> ``[n, S, heads * hd]`` float32, ``hd`` 64 or 80
    (``tia_mha_fwd_f32``: exact float32 products on ``v_mfma_f32_16x16x4_f32``)."""
    from tiatoolbox_amd import _lib

    _f32_tokens("hip_mha_fwd_f32", qkv)
    if qkv.dim() != 3 or heads <= 0 or qkv.shape[-1] % (3 * heads) != 0:  # noqa: PLR2004
        msg = f"hip_mha_fwd_f32 takes [n, S, 3 * heads * head_dim] tokens; got {tuple(qkv.shape)} for {heads} heads."
        raise ValueError(msg)
    n, s, c3 = qkv.shape
    head_dim = c3 // (3 * heads)
    out = torch.empty((n, s, heads * head_dim), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        rc = _lib.load().tia_mha_fwd_f32(qkv.data_ptr(), out.data_ptr(), n, s, heads, head_dim, float(scale), _DT[torch.float32],
                                         _lib.current_stream())
    _lib.check(rc, "tia_mha_fwd_f32")
    return out


def hip_gelu_rows_f32_(x: torch.Tensor) -> torch.Tensor:
    """Exact GELU in place on float32 tokens (``tia_gelu_rows_f32``)."""
    from tiatoolbox_amd import _lib

    _f32_tokens("hip_gelu_rows_f32_", x)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_gelu_rows_f32(x.data_ptr(), x.numel(), _lib.current_stream())
    _lib.check(rc, "tia_gelu_rows_f32")
    return x


def hip_swiglu_rows_f32(x: torch.Tensor) -> torch.Tensor:
    """Packed SwiGLU ``silu(x[..., :H]) * x[..., H:]`` on float32 ``[n, S, 2H]`` tokens -> ``[n, S, H]`` (``tia_swiglu_rows_f32``)."""
    from tiatoolbox_amd import _lib

    _f32_tokens("hip_swiglu_rows_f32", x)
    if x.dim() < 2 or x.shape[-1] % 2 != 0:  # noqa: PLR2004
        msg = f"hip_swiglu_rows_f32 takes [..., 2H] tokens; got {tuple(x.shape)}."
        raise ValueError(msg)
    hidden = x.shape[-1] // 2
    y = torch.empty((*x.shape[:-1], hidden), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib.load().tia_swiglu_rows_f32(x.data_ptr(), y.data_ptr(), x.numel() // (2 * hidden), hidden, _lib.current_stream())
    _lib.check(rc, "tia_swiglu_rows_f32")
    return y


def hip_vit_patchify_f32(x_nhwc: torch.Tensor, patch: int, k_pad: int) -> torch.Tensor:
    """``[n, h, w, 3]`` float32 images -> ``[n, g, k_pad]`` float32 token rows in ``(ky, kx, c)`` order, zeros from column
    ``3 * patch^2`` on (``tia_vit_patchify_f32``: any patch size, a pure gather)."""
    from tiatoolbox_amd import _lib

    if not (x_nhwc.is_cuda and x_nhwc.dim() == 4 and x_nhwc.shape[-1] == 3 and x_nhwc.is_contiguous() and x_nhwc.dtype == torch.float32):  # noqa: PLR2004
        msg = f"hip_vit_patchify_f32 expects a contiguous [n, h, w, 3] float32 CUDA tensor; got {tuple(x_nhwc.shape)}, {x_nhwc.dtype}."
        raise ValueError(msg)
    n, h, w, _ = x_nhwc.shape
    out = torch.empty((n, (h // patch) * (w // patch), k_pad), dtype=torch.float32, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device):
        rc = _lib.load().tia_vit_patchify_f32(x_nhwc.data_ptr(), out.data_ptr(), n, h, w, patch, k_pad, _lib.current_stream())
    _lib.check(rc, "tia_vit_patchify_f32")
    return out


def hip_vit_assemble_f32(tokens: torch.Tensor, cls: torch.Tensor, reg: torch.Tensor | None, pos: torch.Tensor, *,
                         pos_has_cls: bool) -> torch.Tensor:
    """:func:`hip_vit_assemble_rows_f32` for float32 tokens: ``cat([cls (+ pos[0] if pos_has_cls), reg, tokens[b] + pos[pos_has_cls:]])``,
    one float32 add per element (``tia_vit_assemble_f32``)."""
    from tiatoolbox_amd import _lib

    _f32_tokens("hip_vit_assemble_f32", tokens)
    n, g, d = tokens.shape
    nreg = 0 if reg is None else reg.numel() // d
    rows = g + int(pos_has_cls)
    if cls.dtype != torch.float32 or pos.dtype != torch.float32 or cls.numel() != d or pos.numel() != rows * d or not (
            cls.is_contiguous() and pos.is_contiguous()) or (reg is not None and (
                reg.dtype != torch.float32 or not reg.is_contiguous() or nreg == 0 or reg.numel() != nreg * d)):
        msg = (f"hip_vit_assemble_f32 takes float32 cls [{d}], reg [R, {d}] or None and pos [{rows}, {d}]; got {tuple(cls.shape)}, "
               f"{None if reg is None else tuple(reg.shape)}, {tuple(pos.shape)}.")
        raise ValueError(msg)
    out = torch.empty((n, 1 + nreg + g, d), dtype=torch.float32, device=tokens.device)
    with torch.cuda.device(tokens.device):
        rc = _lib.load().tia_vit_assemble_f32(tokens.data_ptr(), cls.data_ptr(), _ptr(reg), pos.data_ptr(), int(pos_has_cls),
                                              out.data_ptr(), n, g, nreg, d, _lib.current_stream())
    _lib.check(rc, "tia_vit_assemble_f32")
    return out


class _LinearF32:
    """One GEMM of the float32 route: ``prepare`` splits the float32 (folded, padded) weights into three bf16 planes for the split
    kernel, or -- a shape off that kernel's, or weights without an exact normal split -- packs them for the float32 kernel
    (``self.split`` says which); the float32 bias throughout.  Called on float32 tokens, with the float32 stream as ``residual``."""

    def __init__(self, name: str, weight: torch.Tensor, bias: torch.Tensor) -> None:
        self.name, self.weight32, self.bias32 = name, weight, bias
        self.cout, self.cin = weight.shape
        self.packed: torch.Tensor | None = None
        self.split: bool | None = None

    def prepare(self) -> None:
        self.packed = pack_linear_weights_split(self.weight32)
        self.split = self.packed is not None
        if not self.split:
            self.packed = pack_linear_weights_f32(self.weight32)
        self.weight32 = None

    def __call__(self, x: torch.Tensor, residual: torch.Tensor | None = None) -> torch.Tensor:
        return hip_linear_f32(x, self.packed, self.bias32, residual, cout=self.cout)


class FusedViT(nn.Module):
    """``forward(imgs)`` == ``VisionTransformer.forward(imgs)`` (float32 features ``[B, D]``) on a CUDA device with fp16 / bf16
    activations, after ``prepare(dtype)`` -- or with float32 activations on the split-bf16 GEMM and the float32 attention kernel,
    after ``prepare(torch.float32, linear_dtype="bfloat16x3")``.  Built from a loaded model (timm parameter names); the constructor
    only folds and checks (it runs on any device), ``prepare`` packs on the GPU."""

    accepts_uint8 = False  # input normalisation is the caller's: `infer_batch` hands the batch over in the parameters' dtype

    def __init__(self, vit: nn.Module) -> None:
        super().__init__()
        if not isinstance(vit, VisionTransformer):
            msg = f"FusedViT covers architecture.vit.VisionTransformer; got {type(vit).__name__}."
            raise UnsupportedLayerError(msg)
        vit = vit.eval()
        self.embed_dim, self.num_heads, self.patch_size = vit.embed_dim, vit.num_heads, vit.patch_size
        self.native_grid, self.dynamic_img_size = vit.native_grid, vit.dynamic_img_size
        head_dim = self.embed_dim // self.num_heads
        if head_dim not in (64, 80):
            msg = f"FusedViT: the attention kernel takes head_dim 64 or 80; this model has {self.embed_dim} / {self.num_heads} = {head_dim}."
            raise UnsupportedLayerError(msg)
        self.scale = head_dim ** -0.5
        self.reg_tokens, self.no_embed_class, self.swiglu = vit.reg_tokens, vit.no_embed_class, vit.mlp_layer == "swiglu_packed"
        self.pos_prefix, self.global_pool = vit.pos_prefix, vit.global_pool
        # register tokens with entries of their own in the table (timm's default form, Virchow2): folded into the prefix per grid
        self.prefix_pos_embed = bool(vit.prefix_pos_embed and vit.reg_tokens)
        self._prefix_cache: dict[tuple[int, int], tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        # patch sizes off the multiples of 8 (14) take the padded im2col: rows of k_pad columns, zeros beyond 3 p^2
        self.k_pad = padded_patch_columns(self.patch_size) if self.patch_size % 8 != 0 else None
        # the parameters the module keeps (small): they carry device and dtype for `infer_batch`; their float32 values are set aside
        self.cls_token, self.pos_embed = vit.cls_token, vit.pos_embed
        self._cls32 = vit.cls_token.detach().to(torch.float32).reshape(-1).contiguous()
        self._pos32 = vit.pos_embed.detach().to(torch.float32).contiguous()
        self.reg_token = vit.reg_token if self.reg_tokens else None
        self._reg32 = vit.reg_token.detach().to(torch.float32).reshape(self.reg_tokens, -1).contiguous() if self.reg_tokens else None
        self._pos_cache: dict[tuple[int, int], torch.Tensor] = {}
        f32 = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        proj = vit.patch_embed.proj
        # [D, 3, p, p] -> [D, p, p, 3]: the (ky, kx, c) order of tia_vit_patchify_h
        patch_w = f32(proj.weight).permute(0, 2, 3, 1).reshape(self.embed_dim, -1)
        if self.k_pad is not None:  # zero columns (exact, in float32, before the one rounding) under the zero columns of the tokens
            patch_w = torch.nn.functional.pad(patch_w, (0, self.k_pad - patch_w.shape[1]))
        self.patch = _Linear("patch_embed.proj", patch_w.contiguous(), f32(proj.bias))
        self.layers: list[dict] = []
        for i, blk in enumerate(vit.blocks):
            qkv_w, qkv_b = fold_layer_scale(blk.attn.qkv, None)
            proj_w, proj_b = fold_layer_scale(blk.attn.proj, blk.ls1)
            fc1_w, fc1_b = fold_layer_scale(blk.mlp.fc1, None)
            fc2_w, fc2_b = fold_layer_scale(blk.mlp.fc2, blk.ls2)
            if self.swiglu:  # halves off the GEMM's multiple of 32 (Virchow: 3416) get exact zero lanes, after the fold
                fc1_w, fc1_b, fc2_w = pad_swiglu(fc1_w, fc1_b, fc2_w)
            self.layers.append({
                "norm1": (f32(blk.norm1.weight), f32(blk.norm1.bias)), "norm2": (f32(blk.norm2.weight), f32(blk.norm2.bias)),
                "qkv": _Linear(f"blocks.{i}.attn.qkv", qkv_w, qkv_b), "proj": _Linear(f"blocks.{i}.attn.proj", proj_w, proj_b),
                "fc1": _Linear(f"blocks.{i}.mlp.fc1", fc1_w, fc1_b), "fc2": _Linear(f"blocks.{i}.mlp.fc2", fc2_w, fc2_b)})
        self._norm = (f32(vit.norm.weight), f32(vit.norm.bias))
        self.half_dtype: torch.dtype | None = None
        self.linear_dtype: str | None = None
        self.residual_dtype: str | None = None
        self.smoothing: dict[str, torch.Tensor] | None = None  # the per-input-channel scales `prepare` applied (layer name -> [cin])
        self._taps: dict[str, torch.Tensor] | None = None      # calibration: layer name -> abs-max of its float32 input, per channel
        self._amax_w: dict[str, torch.Tensor] = {}             # calibration: layer name -> max_o |W[o, j]| of the weights to pack
        # maps beside the output: the engine sets `return_attention` ("class" | "rollout") before a run and reads `attention_maps` after
        # each forward (`forward` and `forward_uint8` alike); None: not one additional launch
        self.return_attention: str | None = None
        # the rollout's other forms (the engines' `attention_head_fusion` / `attention_discard_ratio`); the defaults are today's path
        self.attention_head_fusion: str = "mean"
        self.attention_discard_ratio: float = 0.0
        self.attention_maps: torch.Tensor | None = None
        self._rollout: torch.Tensor | None = None

    def prepare(self, dtype: torch.dtype, linear_dtype: str | None = None, residual_dtype: str | None = None,
                smoothing: dict[str, torch.Tensor] | None = None) -> None:
        """Pack every GEMM's float32 (folded) weights for ``tia_conv2d_nhwc_h`` in ``dtype`` (rounded once, after the folding): call
        this on the device, BEFORE ``.to(dtype)``.  Biases, LayerNorm affines, the class token and the position table stay float32
        in plain attributes that the cast does not reach.

        ``linear_dtype="float8_e4m3"`` (bfloat16 carrier only) puts ``attn.qkv``, ``mlp.fc1`` and ``mlp.fc2`` of every block on the
        FP8 GEMM (``tia_linear_fp8_rows``; the numeric contract is in ``include/tiatoolbox_amd.h`` and DESIGN 4.34): their weights are
        quantised per output channel from the same float32 weights, and the LayerNorm / activation in front of each becomes its
        quantising form.  A layer off that kernel's shapes stays on the half kernel (one ``info`` line names them); ``attn.proj``,
        the patch embedding, attention, the residual stream and the final norm are the half graph's, unchanged.

        ``linear_dtype="int8"`` (bfloat16 carrier only) is the same routing on the INT8 GEMM (``tia_linear_int8_rows``: W8A8, one
        scale per token and per output channel, an exact int32 accumulator; the contract is in ``include/tiatoolbox_amd.h`` and
        DESIGN 4.38) with the ``_qi8`` producers; its codes are ``torch.int8`` tensors, the FP8 route's ``torch.uint8``, and neither
        layer takes the other's.  A float16 carrier, a ``residual_dtype`` beside it and a float32 carrier are refused, each with a
        message of its own, before any device work.

        ``smoothing=scales`` beside ``linear_dtype="int8"`` (``scales`` from :func:`calibrate_int8_smoothing`, layer
        name -> float32 ``[cin]`` powers of two) divides the input of every routed layer by ``s`` per channel and multiplies its
        weight columns by ``s`` in float32 before they are packed -- both exact, so the layer's real-valued function is unchanged
        while an outlier channel no longer sets the token's scale.  For ``qkv`` / ``fc1`` the division is folded into the float32
        LayerNorm affine; ``fc2``'s producer becomes ``hip_act_rows_qi8_smooth``.  ``None`` is the unsmoothed path; all-ones scales
        reproduce it bit for bit.  Beside any other ``linear_dtype``, with a key missing for a routed layer, a wrong length or a scale
        that is no finite positive power of two it is a ``ValueError``, raised before anything is padded or packed; keys of layers
        that stay on the half kernel are ignored with one ``info`` line.  ``self.smoothing`` holds what was applied.

        ``residual_dtype="float32"`` keeps the residual stream ``x`` in float32 from token assembly to the final norm, as the float32
        module under ``torch.autocast`` does: ``proj`` and ``fc2`` write half branches without a residual, and one pass
        (``tia_add_layernorm_rows_f32``) adds the branch to ``x`` in float32 and normalises the sum.  ``None`` (the
        default) is the graph above, bit for bit.  Not together with ``linear_dtype="float8_e4m3"``: the quantising LayerNorm has no
        float32-input form, and no other precision is put in its place.

        ``prepare(torch.float32, linear_dtype="bfloat16x3")`` (the engines' ``compute_dtype="bfloat16x3"``) is the float32 route:
        float32 activations, residual stream and row arithmetic, every Linear on the split-bf16 GEMM
        (``tia_conv2d_bf16x3_nhwc_f32``: the float32 weights as three bf16 planes, ``hi + mid + lo == w`` exactly -- no other
        rounding of the weights) with the residual add in its epilogue, attention on ``tia_mha_fwd_f32``.  A layer off
        that kernel's shapes (``cin % 16``, ``cout % 128``) or without an exact normal split goes on ``tia_conv2d_nhwc_f32`` (one
        ``info`` line names them); a packed SwiGLU whose ``fc1`` is off the multiple is first padded with exact zero lanes.
        ``half_dtype`` stays ``None``.  ``torch.float32`` without that keyword, with ``"float8_e4m3"`` or with ``residual_dtype`` is
        refused as before; ``"bfloat16x3"`` with a half ``dtype`` is refused too."""
        if smoothing is not None and linear_dtype != INT8_LINEAR:
            msg = (f"FusedViT.prepare: smoothing= scales the inputs and weight columns of the layers on the INT8 GEMM and goes with "
                   f"linear_dtype={INT8_LINEAR!r} only (the FP8 route's floating grid does not need it, the half and float32 routes do "
                   f"not quantise); got linear_dtype={linear_dtype!r}.")
            raise ValueError(msg)
        if linear_dtype == SPLIT_LINEAR and dtype == torch.float32 and residual_dtype is None:
            if self.half_dtype is not None or self.linear_dtype is not None:
                msg = "FusedViT.prepare packs once, from the float32 weights; build a new FusedViT for another dtype."
                raise ValueError(msg)
            self._route_split()
            self.linear_dtype = SPLIT_LINEAR
            return
        if linear_dtype == INT8_LINEAR and dtype == torch.float32:  # (the new option's own refusals; the pinned ones follow unchanged)
            msg = (f"FusedViT.prepare: linear_dtype={INT8_LINEAR!r} quantises the bfloat16 graph's qkv / fc1 / fc2 layers and has no float32 "
                   f"carrier; call prepare(torch.bfloat16, linear_dtype={INT8_LINEAR!r}), or prepare(torch.float32, "
                   f"linear_dtype={SPLIT_LINEAR!r}) for the float32 route.")
            raise ValueError(msg)
        if dtype not in _HALF:
            msg = (f"FusedViT runs in float16 or bfloat16, or in float32 with linear_dtype={SPLIT_LINEAR!r} and nothing else (the float32 "
                   f"route); got {dtype} with linear_dtype={linear_dtype!r}, residual_dtype={residual_dtype!r}.")
            raise ValueError(msg)
        if self.half_dtype is not None or self.linear_dtype == SPLIT_LINEAR:
            msg = "FusedViT.prepare packs once, from the float32 weights; build a new FusedViT for another dtype."
            raise ValueError(msg)
        if linear_dtype == SPLIT_LINEAR:  # (checked before any device work)
            msg = (f"FusedViT.prepare: linear_dtype={SPLIT_LINEAR!r} is the float32 route, prepare(torch.float32, "
                   f"linear_dtype={SPLIT_LINEAR!r}) without a residual_dtype (its stream is float32 already); got {dtype}, "
                   f"residual_dtype={residual_dtype!r}.")
            raise ValueError(msg)
        if residual_dtype is not None:  # (checked before any device work)
            if residual_dtype != RESIDUAL_F32:
                msg = f"FusedViT.prepare: residual_dtype is None (the stream in `dtype`) or {RESIDUAL_F32!r}; got {residual_dtype!r}."
                raise ValueError(msg)
            if linear_dtype == INT8_LINEAR:
                msg = (f"FusedViT.prepare: linear_dtype={INT8_LINEAR!r} runs on the bfloat16 residual stream only: there is no "
                       f"tia_layernorm_rows_qi8 that reads a float32 stream, so residual_dtype={residual_dtype!r} is refused beside it; "
                       "choose one.")
                raise ValueError(msg)
            if linear_dtype is not None:
                msg = (f"FusedViT.prepare: residual_dtype={RESIDUAL_F32!r} beside linear_dtype={linear_dtype!r} needs a float32-input "
                       "quantising LayerNorm (a tia_layernorm_rows_q8 that reads the float32 stream), which does not exist; choose one.")
                raise ValueError(msg)
        if linear_dtype == INT8_LINEAR:
            if dtype != torch.bfloat16:
                msg = (f"FusedViT.prepare: linear_dtype={INT8_LINEAR!r} runs on the bfloat16 carrier only (an fp16 carrier is not built); "
                       f"got {dtype}.")
                raise ValueError(msg)
            self._route_int8(smoothing)
        elif linear_dtype is not None:
            if linear_dtype != FP8_LINEAR:
                msg = f"FusedViT.prepare: linear_dtype is None or {FP8_LINEAR!r}; got {linear_dtype!r}."
                raise ValueError(msg)
            if dtype != torch.bfloat16:
                msg = f"FusedViT.prepare: linear_dtype={FP8_LINEAR!r} runs on the bfloat16 carrier only (there is no fp16 form); got {dtype}."
                raise ValueError(msg)
            self._route_fp8()
        self.patch.prepare(dtype)
        for layer in self.layers:
            for name in ("qkv", "proj", "fc1", "fc2"):
                layer[name].prepare(dtype)
        self.half_dtype, self.linear_dtype = dtype, linear_dtype
        self.residual_dtype = residual_dtype

    def _route_fp8(self) -> None:
        """``qkv`` / ``fc1`` / ``fc2`` of every block to :class:`_LinearFp8` where ``tia_linear_fp8_serves`` takes the shape
        (``_route_quant``)."""
        self._route_quant(_LinearFp8)

    def _route_int8(self, smoothing: dict[str, torch.Tensor] | None = None) -> None:
        """``qkv`` / ``fc1`` / ``fc2`` of every block to :class:`_LinearInt8` where ``tia_linear_int8_serves`` takes the shape
        (``_route_quant``), with the ``smoothing`` scales applied where given."""
        self._route_quant(_LinearInt8, smoothing)

    def _quant_padded_half(self, fc2: _Linear) -> int | None:
        """The width the quantised routes pad a packed SwiGLU half to (the kernels' multiple of 128), or ``None`` where they leave
        it: at or above ``SWIGLU_PAD_FLOOR`` only, as ``pad_swiglu`` does."""
        target = -(-fc2.cin // 128) * 128
        return target if self.swiglu and target != fc2.cin and fc2.cin >= SWIGLU_PAD_FLOOR else None

    def _pad_swiglu_for_quant(self) -> None:
        for layer in self.layers:
            fc1, fc2 = layer["fc1"], layer["fc2"]
            target = self._quant_padded_half(fc2)
            if target is not None:
                fc1_w, fc1_b, fc2_w = pad_swiglu_to(fc1.weight32, fc1.bias32, fc2.weight32, target)
                layer["fc1"], layer["fc2"] = _Linear(fc1.name, fc1_w, fc1_b), _Linear(fc2.name, fc2_w, fc2.bias32)

    def _checked_smoothing(self, fmt: _QuantFormat, smoothing: dict[str, torch.Tensor]) -> dict[str, torch.Tensor]:
        """The entries of ``smoothing`` for the layers ``_route_quant`` will route, checked, as float32 CPU tensors -- worked out from
        the shapes alone, before anything is padded or packed."""
        if not isinstance(smoothing, dict):
            msg = (f"FusedViT.prepare: smoothing is a dict of layer name -> scales [cin] (calibrate_int8_smoothing's result); got "
                   f"{type(smoothing).__name__}.")
            raise ValueError(msg)
        scales: dict[str, torch.Tensor] = {}
        for layer in self.layers:
            half = self._quant_padded_half(layer["fc2"])
            for name in ("qkv", "fc1", "fc2"):
                lin = layer[name]
                cout = 2 * half if half is not None and name == "fc1" else lin.cout
                cin = half if half is not None and name == "fc2" else lin.cin
                if not fmt.fn("serves")(cout, cin):
                    continue
                if lin.name not in smoothing:
                    msg = (f"FusedViT.prepare: smoothing has no scales for `{lin.name}` ({cin} -> {cout}), which goes on the {fmt.name} "
                           f"GEMM; calibrate_int8_smoothing returns one entry per routed layer.")
                    raise ValueError(msg)
                scales[lin.name] = _checked_smoothing_scale(lin.name, smoothing[lin.name], cin)
        ignored = sorted(str(k) for k in smoothing if k not in scales)
        if ignored:
            import logging

            logging.getLogger("tiatoolbox_amd").info(
                "FusedViT: smoothing scales of %d layer(s) that stay on the half kernel (neither smoothed nor quantised) are ignored: %s.",
                len(ignored), ", ".join(ignored))
        return scales

    def _route_quant(self, linear_cls: type[_LinearQuant], smoothing: dict[str, torch.Tensor] | None = None) -> None:
        """``qkv`` / ``fc1`` / ``fc2`` of every block to ``linear_cls`` where its format's ``serves`` takes the shape.  A packed SwiGLU
        half off the kernels' multiple of 128 is first padded up to it with ``pad_swiglu``'s exact zero lanes (at or above
        ``SWIGLU_PAD_FLOOR`` only, as there).  With ``smoothing``, a routed layer's weight columns are multiplied by its scales ``s``
        in float32 (exact: powers of two) and its input divided by them: folded into the LayerNorm affine in front of ``qkv`` /
        ``fc1`` (``gamma / s``, ``beta / s``), handed to ``fc2``'s producer as ``inv_smooth = 1 / s``."""
        fmt = linear_cls.fmt
        scales = self._checked_smoothing(fmt, smoothing) if smoothing is not None else None
        kept: list[str] = []
        self._pad_swiglu_for_quant()
        for layer in self.layers:
            for name in ("qkv", "fc1", "fc2"):
                lin = layer[name]
                if fmt.fn("serves")(lin.cout, lin.cin):
                    weight, inv = lin.weight32, None
                    if scales is not None:
                        s = scales[lin.name].to(weight.device)
                        weight, inv = weight * s, (1.0 / s).contiguous()
                        if name != "fc2":
                            norm = "norm1" if name == "qkv" else "norm2"
                            layer[norm] = tuple((t * inv).contiguous() for t in layer[norm])
                    layer[name] = linear_cls(lin.name, weight, lin.bias32)
                    if inv is not None and name == "fc2":
                        layer[name].inv_smooth = inv
                else:
                    kept.append(f"{lin.name} ({lin.cin} -> {lin.cout})")
        self.smoothing = scales
        if kept:
            import logging

            logging.getLogger("tiatoolbox_amd").info(
                f"FusedViT: the {fmt.name} GEMM takes cin %% 128 == 0 and cout %% 16 == 0; %d layer(s) stay on the half kernel: %s.",  # noqa: G004
                len(kept), ", ".join(kept))

    def _route_split(self) -> None:
        """Every GEMM of the graph to :class:`_LinearF32`, packed.  A packed SwiGLU whose ``fc1`` is off the split kernel's multiple
        of 128 output channels gets ``pad_swiglu``'s exact zero lanes up to the next multiple of 64 per half (at or above
        ``SWIGLU_PAD_FLOOR`` only, as there; Virchow: 3424 -> 3456, ``fc1`` 6912)."""
        kept: list[str] = []

        def routed(lin: _Linear) -> _LinearF32:
            new = _LinearF32(lin.name, lin.weight32, lin.bias32)
            new.prepare()
            if not new.split:
                kept.append(f"{new.name} ({new.cin} -> {new.cout})")
            return new

        self.patch = routed(self.patch)
        for layer in self.layers:
            fc1, fc2 = layer["fc1"], layer["fc2"]
            if self.swiglu and fc1.cout % 128 != 0 and fc2.cin >= SWIGLU_PAD_FLOOR:
                fc1_w, fc1_b, fc2_w = pad_swiglu_to(fc1.weight32, fc1.bias32, fc2.weight32, -(-fc2.cin // 64) * 64)
                layer["fc1"], layer["fc2"] = _Linear(fc1.name, fc1_w, fc1_b), _Linear(fc2.name, fc2_w, fc2.bias32)
            for name in ("qkv", "proj", "fc1", "fc2"):
                layer[name] = routed(layer[name])
        if kept:
            import logging

            logging.getLogger("tiatoolbox_amd").info(
                "FusedViT: the split-bf16 GEMM takes cin %% 16 == 0, cout %% 128 == 0 and weights with an exact split into normal bf16 "
                "numbers; %d layer(s) run on the float32 GEMM (tia_conv2d_nhwc_f32): %s.", len(kept), ", ".join(kept))

    def begin_int8_calibration(self) -> None:
        """Make this (unprepared) graph the calibration graph of :func:`calibrate_int8_smoothing`: the bfloat16 hand-written graph
        (``prepare(torch.bfloat16)``) with the INT8 route's SwiGLU padding, whose forward also accumulates, for every layer the INT8
        GEMM will serve, the per-channel abs-max of the float32 value its producer holds (``hip_layernorm_rows_absmax_h`` /
        ``hip_act_rows_absmax_h``).  The weight column maxima are taken here, from the float32 weights ``prepare`` would pack."""
        if self.half_dtype is not None or self.linear_dtype is not None:
            msg = "FusedViT.begin_int8_calibration starts from the float32 weights: build a new FusedViT (prepare packs once)."
            raise ValueError(msg)
        self._pad_swiglu_for_quant()
        taps: dict[str, torch.Tensor] = {}
        for layer in self.layers:
            for name in ("qkv", "fc1", "fc2"):
                lin = layer[name]
                if _INT8.fn("serves")(lin.cout, lin.cin):
                    self._amax_w[lin.name] = lin.weight32.abs().amax(dim=0).cpu()
                    taps[lin.name] = torch.zeros(lin.cin, dtype=torch.float32, device=lin.weight32.device)
        self.prepare(torch.bfloat16)
        self._taps = taps

    def int8_calibration_scales(self, alpha: float = 0.5) -> dict[str, torch.Tensor]:
        """:func:`int8_smoothing_scales` of every tapped layer from what the forwards since ``begin_int8_calibration`` have seen."""
        alpha = _checked_alpha(alpha)
        if not self._taps:
            msg = ("FusedViT.int8_calibration_scales: no layer of this model goes on the INT8 GEMM (or begin_int8_calibration was not "
                   "called): there is nothing to smooth.")
            raise ValueError(msg)
        scales = {}
        for name, tap in self._taps.items():
            try:
                scales[name] = int8_smoothing_scales(tap, self._amax_w[name], alpha)
            except ValueError as exc:
                msg = f"calibrate_int8_smoothing: `{name}`: {exc}"
                raise ValueError(msg) from exc
        return scales

    def _forward_f32(self, imgs: torch.Tensor) -> torch.Tensor:
        """The float32 route (``linear_dtype="bfloat16x3"``): the module's block sequence on float32 tensors --
        LN -> qkv -> ``tia_mha_fwd_f32`` -> proj (+ x) -> LN -> fc1 -> GELU / SwiGLU -> fc2 (+ x), then the final norm or pool.  The
        residual adds are the GEMMs' ``d_residual``; the LayerNorm is ``tia_add_layernorm_rows_f32`` without a branch and with
        float32 output, the pooled end ``tia_vit_cls_mean_pool_f32`` without a branch."""
        if self.return_attention is not None:
            msg = "FusedViT: the float32 route (linear_dtype=\"bfloat16x3\") has no attention-map kernel; return_attention must be None."
            raise ValueError(msg)
        p = self.patch_size
        _, _, h, w = imgs.shape
        if h % p != 0 or w % p != 0:
            msg = f"FusedViT: the input size {h} x {w} is no multiple of the patch size {p}."
            raise ValueError(msg)
        grid = (h // p, w // p)
        pos = self._pos_for(grid)  # (refuses an off-grid size before any launch)
        x = imgs.permute(0, 2, 3, 1).to(torch.float32).contiguous()  # the NHWC batch under the NCHW view
        cols = hip_vit_patchify_f32(x, p, self.k_pad if self.k_pad is not None else 3 * p * p)
        n, d = cols.shape[0], self.embed_dim
        tok = self.patch(cols)
        if self.prefix_pos_embed:
            cls, reg, pos_grid = self._prefix_for(grid)
            x = hip_vit_assemble_f32(tok, cls, reg, pos_grid, pos_has_cls=False)
        elif self.reg_tokens or self.no_embed_class:
            x = hip_vit_assemble_f32(tok, self._cls32, self._reg32, pos, pos_has_cls=not self.no_embed_class)
        else:
            x = hip_vit_assemble_f32(tok, self._cls32, None, pos, pos_has_cls=True)
        s = x.shape[1]

        def norm(norm: tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:  # (`dtype` names the absent branch's type: not looked at)
            return hip_add_layernorm_rows_f32(x, None, *norm, eps=LN_EPS, rows=n * s, row_stride=d, dtype=torch.bfloat16,
                                              out_dtype=torch.float32).view(n, s, d)

        for layer in self.layers:
            a = hip_mha_fwd_f32(layer["qkv"](norm(layer["norm1"])), self.num_heads, self.scale)
            x = layer["proj"](a, residual=x)
            a = layer["fc1"](norm(layer["norm2"]))
            a = hip_swiglu_rows_f32(a) if self.swiglu else hip_gelu_rows_f32_(a)
            x = layer["fc2"](a, residual=x)
        if self.global_pool == "token_mean":
            return hip_vit_cls_mean_pool_f32(x, None, *self._norm, eps=LN_EPS, skip=1 + self.reg_tokens, dtype=torch.bfloat16)
        return hip_add_layernorm_rows_f32(x, None, *self._norm, eps=LN_EPS, rows=n, row_stride=s * d, dtype=torch.bfloat16,
                                          out_dtype=torch.float32)

    def _pos_for(self, grid: tuple[int, int]) -> torch.Tensor:
        if grid not in self._pos_cache:
            self._pos_cache[grid] = resample_pos_embed(self._pos32, self.native_grid, grid, dynamic=self.dynamic_img_size,
                                                       num_prefix=self.pos_prefix).reshape(-1, self.embed_dim).contiguous()
        return self._pos_cache[grid]

    def _prefix_for(self, grid: tuple[int, int]) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``prefix_pos_embed``: ``(cls + pos[0], reg + pos[1 : 1 + R], pos[1 + R :])`` for ``grid`` -- the float32 adds the
        assembly kernel would make, made once on the host side of the one rounding, so that ``tia_vit_assemble_prefix_h`` with
        ``pos_has_cls = 0`` writes ``cat([cls, reg, patches]) + pos``."""
        if grid not in self._prefix_cache:
            pos, r = self._pos_for(grid), self.reg_tokens
            self._prefix_cache[grid] = ((self._cls32 + pos[0]).contiguous(), (self._reg32 + pos[1:1 + r]).contiguous(),
                                        pos[1 + r:].contiguous())
        return self._prefix_cache[grid]

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        if self.linear_dtype == SPLIT_LINEAR:
            return self._forward_f32(imgs)
        half = self.half_dtype
        if half is None:
            msg = "FusedViT.forward needs prepare(dtype) first."
            raise RuntimeError(msg)
        p = self.patch_size
        _, _, h, w = imgs.shape
        if h % p != 0 or w % p != 0:
            msg = f"FusedViT: the input size {h} x {w} is no multiple of the patch size {p}."
            raise ValueError(msg)
        pos = self._pos_for((h // p, w // p))  # (refuses an off-grid size before any launch)
        x = imgs.permute(0, 2, 3, 1)  # the NHWC batch under the NCHW view
        if x.dtype not in (torch.float32, half):
            x = x.to(torch.float32)
        if self.k_pad is None:
            cols = hip_vit_patchify_h(x.contiguous(), p, half)
        else:
            cols = hip_vit_patchify_pad_h(x.contiguous(), p, self.k_pad, half)
        return self._from_patch_columns(cols, pos, (h // p, w // p))

    def forward_uint8(self, x_u8_nhwc: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
        """``forward`` of ``table[x, channel]`` for a uint8 NHWC batch (``ToTensor`` + ``Normalize`` as ``TimmNormPreproc``'s
        ``[256, 3]`` table in the graph's dtype): ``tia_vit_patchify_norm_u8_h`` makes the look-up while it lays the patches out, and
        the graph runs from the token GEMM on as in ``forward`` -- bit for bit ``forward(hook.device_batch(x, dtype))``."""
        half = self.half_dtype
        if self.linear_dtype == SPLIT_LINEAR:
            msg = "FusedViT.forward_uint8: the float32 route has no uint8 im2col; hand `forward` the normalised float32 batch."
            raise RuntimeError(msg)
        if half is None:
            msg = "FusedViT.forward_uint8 needs prepare(dtype) first."
            raise RuntimeError(msg)
        if x_u8_nhwc.dim() != 4 or x_u8_nhwc.shape[-1] != 3 or x_u8_nhwc.dtype != torch.uint8:  # noqa: PLR2004
            msg = f"FusedViT.forward_uint8 takes a uint8 [n, h, w, 3] batch; got {tuple(x_u8_nhwc.shape)}, {x_u8_nhwc.dtype}."
            raise ValueError(msg)
        p = self.patch_size
        _, h, w, _ = x_u8_nhwc.shape
        if h % p != 0 or w % p != 0:
            msg = f"FusedViT: the input size {h} x {w} is no multiple of the patch size {p}."
            raise ValueError(msg)
        pos = self._pos_for((h // p, w // p))  # (refuses an off-grid size before any launch)
        k_pad = self.k_pad if self.k_pad is not None else 3 * p * p
        cols = hip_vit_patchify_norm_u8_h(x_u8_nhwc.contiguous(), table, p, k_pad, half)
        return self._from_patch_columns(cols, pos, (h // p, w // p))

    def _from_patch_columns(self, cols: torch.Tensor, pos: torch.Tensor, grid: tuple[int, int]) -> torch.Tensor:
        """The graph from the token GEMM on: ``cols`` ``[n, g, 3 p^2 or k_pad]`` are the im2col rows of either input form."""
        self._rollout = None  # (a forward that raised half way leaves nothing behind for the next one's recursion)
        if self.residual_dtype is not None:
            return self._from_patch_columns_f32(cols, pos, grid)
        n, d = cols.shape[0], self.embed_dim
        tok = self.patch(cols)
        if self.prefix_pos_embed:
            cls, reg, pos_grid = self._prefix_for(grid)
            x = hip_vit_assemble_prefix_h(tok, cls, reg, pos_grid, pos_has_cls=False)
        elif self.reg_tokens or self.no_embed_class:
            x = hip_vit_assemble_prefix_h(tok, self._cls32, self._reg32, pos, pos_has_cls=not self.no_embed_class)
        else:
            x = hip_vit_assemble_tokens_h(tok, self._cls32, pos)
        s = x.shape[1]
        taps = self._taps if self._taps is not None else {}  # (calibration only: the float32 inputs of the layers to smooth)

        def norm_for(linear: _Linear | _LinearQuant, norm: tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor | QuantRows:
            if linear.name in taps:
                hip_layernorm_rows_absmax_h(x, *norm, taps[linear.name], eps=LN_EPS)
            if isinstance(linear, _LinearQuant):  # the same pass over x, codes + scales out
                return linear.fmt.fn("layernorm")(x, *norm, eps=LN_EPS)
            return hip_layernorm_rows_h(x, *norm, eps=LN_EPS, rows=n * s, row_stride=d).view(n, s, d)

        for layer in self.layers:
            a = self._attend(layer["qkv"](norm_for(layer["qkv"], layer["norm1"])), layer is self.layers[-1])
            x = layer["proj"](a, residual=x)
            a = layer["fc1"](norm_for(layer["fc1"], layer["norm2"]))
            if layer["fc2"].name in taps:
                hip_act_rows_absmax_h(a, taps[layer["fc2"].name], swiglu=self.swiglu)
            if getattr(layer["fc2"], "inv_smooth", None) is not None:  # smoothing: 1 / s per input channel before the row is quantised
                a = hip_act_rows_qi8_smooth(a, layer["fc2"].inv_smooth, swiglu=self.swiglu)
            elif isinstance(layer["fc2"], _LinearQuant):
                a = layer["fc2"].fmt.fn("act")(a, swiglu=self.swiglu)
            else:
                a = hip_swiglu_rows_h(a) if self.swiglu else hip_gelu_rows_h_(a)
            x = layer["fc2"](a, residual=x)
        self._finish_attention(grid)
        if self.global_pool == "token_mean":
            return hip_vit_cls_mean_pool_h(x, *self._norm, eps=LN_EPS, skip=1 + self.reg_tokens)
        return hip_layernorm_rows_h(x, *self._norm, eps=LN_EPS, rows=n, row_stride=s * d, out_dtype=torch.float32)

    def _attend(self, qkv: torch.Tensor, last: bool) -> torch.Tensor:  # noqa: FBT001
        """``hip_mha_fwd_h`` of a block and -- only with ``return_attention`` -- the map kernels on the SAME ``qkv`` tensor, after it: they
        read what attention read and write buffers of their own, so the maps describe the computation that ran, on every half
        route.  "class": one ``tia_mha_probs_h`` launch in the last block (the class row, per head); "rollout": per block the head
        mean of all rows and one ``tia_rollout_step_f32`` -- or, with another ``attention_head_fusion`` or a discard count ``k >= 1``,
        ``tia_mha_probs_fused_h``, ``tia_rollout_discard_normalize_f32`` and (from the second block on) ``tia_rollout_product_f32``."""
        kind = self.return_attention
        if kind not in (None, "class", "rollout"):
            msg = f"FusedViT.return_attention is None, 'class' or 'rollout'; got {kind!r}."
            raise ValueError(msg)
        a = hip_mha_fwd_h(qkv, self.num_heads, self.scale)
        if kind == "class":
            if last:
                self._rollout = hip_mha_probs_h(qkv, self.num_heads, self.scale, q_rows=1, head_mean=False)
        elif kind == "rollout":
            from tiatoolbox_amd.models.engine import _rollout_options as ro

            fusion, ratio = ro.check_options(self.attention_head_fusion, self.attention_discard_ratio, who="FusedViT")
            k = ro.discard_count(ratio, qkv.shape[1])
            if fusion == "mean" and k == 0:  # today's launches and no other
                mean = hip_mha_probs_h(qkv, self.num_heads, self.scale, q_rows=qkv.shape[1], head_mean=True)
                self._rollout = hip_rollout_step_f32(mean, self._rollout)
            else:  # R_1 = A^_1 needs no product
                a_hat = hip_rollout_discard_normalize_f32(hip_mha_probs_fused_h(qkv, self.num_heads, self.scale, fusion), k)
                self._rollout = a_hat if self._rollout is None else hip_rollout_product_f32(a_hat, self._rollout)
        return a

    def _finish_attention(self, grid: tuple[int, int]) -> None:
        """``attention_maps`` of the forward that just ran: the patch columns (``[1 + R:]``) of the class row on the grid --
        ``[n, H, gh, gw]`` of the last block's probabilities, or ``[n, gh, gw]`` of the rollout matrix."""
        r, self._rollout = self._rollout, None
        if self.return_attention is None:
            self.attention_maps = None
            return
        prefix = 1 + self.reg_tokens
        if self.return_attention == "class":
            self.attention_maps = r[:, :, 0, prefix:].reshape(r.shape[0], self.num_heads, *grid).contiguous()
        else:
            self.attention_maps = r[:, 0, prefix:].reshape(r.shape[0], *grid).contiguous()

    def _from_patch_columns_f32(self, cols: torch.Tensor, pos: torch.Tensor, grid: tuple[int, int]) -> torch.Tensor:
        """``_from_patch_columns`` under ``residual_dtype="float32"``: ``x`` is a float32 ``[n, S, D]`` tensor that only
        ``tia_add_layernorm_rows_f32`` writes.  Every GEMM, attention and the activation are the half graph's; ``proj`` and ``fc2`` get
        NO residual and write the half branch ``b = round(gamma (W a + b))``, and the pass in front of the next GEMM is
        ``x += float(b); a = LN(x)`` -- the branch rounded once, the sum never: the float32 module under ``torch.autocast``."""
        n, d, half = cols.shape[0], self.embed_dim, self.half_dtype
        tok = self.patch(cols)
        if self.prefix_pos_embed:
            cls, reg, pos_grid = self._prefix_for(grid)
            x = hip_vit_assemble_rows_f32(tok, cls, reg, pos_grid, pos_has_cls=False)
        elif self.reg_tokens or self.no_embed_class:
            x = hip_vit_assemble_rows_f32(tok, self._cls32, self._reg32, pos, pos_has_cls=not self.no_embed_class)
        else:
            x = hip_vit_assemble_rows_f32(tok, self._cls32, None, pos, pos_has_cls=True)
        s = x.shape[1]

        def add_norm(branch: torch.Tensor | None, norm: tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
            return hip_add_layernorm_rows_f32(x, branch, *norm, eps=LN_EPS, rows=n * s, row_stride=d, dtype=half).view(n, s, d)

        b = None  # the branch not yet added to x (block 0's first pass has none: LayerNorm only)
        for layer in self.layers:
            a = self._attend(layer["qkv"](add_norm(b, layer["norm1"])), layer is self.layers[-1])
            b = layer["proj"](a)
            a = layer["fc1"](add_norm(b, layer["norm2"]))
            a = hip_swiglu_rows_h(a) if self.swiglu else hip_gelu_rows_h_(a)
            b = layer["fc2"](a)
        self._finish_attention(grid)
        if self.global_pool == "token_mean":
            return hip_vit_cls_mean_pool_f32(x, b, *self._norm, eps=LN_EPS, skip=1 + self.reg_tokens, dtype=half)
        # the class rows only: the last branch is added to them (both strides S * D) and the final norm is written in float32
        return hip_add_layernorm_rows_f32(x, b, *self._norm, eps=LN_EPS, rows=n, row_stride=s * d, dtype=half, out_dtype=torch.float32)


class FusedViTClassifier(nn.Module):
    """The inference form of a ``vanilla.TimmModel``: its backbone as :class:`FusedViT` and the classifier on the graph's float32
    features as ``tia_linear_softmax_rows_f32`` -- ``forward(imgs)`` == ``TimmModel.forward(imgs)``, float32 probabilities
    ``[n, num_classes]``; ``forward_uint8(x, table)`` the same from a uint8 NHWC batch (``FusedViT.forward_uint8``).

    The head stays float32, as the module's ``softmax(logit.float())`` means it: its weights are plain attributes that the cast of
    the surrounding module does not reach.  Built from a loaded model on its device; ``FusedViT``'s refusals (``UnsupportedLayerError``)
    pass through.  More than ``HEAD_MAX_CLASSES`` classes (or features beyond ``HEAD_MAX_FEATURES``) are outside the head kernel:
    ``classifier`` and the softmax then stay torch operations on the same float32 features, with one warning."""

    def __init__(self, model: nn.Module) -> None:
        super().__init__()
        classifier = getattr(model, "classifier", None)
        if not isinstance(classifier, nn.Linear):
            msg = f"FusedViTClassifier covers a TimmModel (feat_extract + an nn.Linear classifier); got {type(model).__name__}."
            raise UnsupportedLayerError(msg)
        self.feat_extract = FusedViT(model.feat_extract)
        self.num_classes, self.num_features = classifier.out_features, classifier.in_features
        self._w32 = classifier.weight.detach().to(torch.float32).contiguous()
        self._b32 = classifier.bias.detach().to(torch.float32).contiguous() if classifier.bias is not None else None
        self.head_kernel = self.num_classes <= HEAD_MAX_CLASSES and self.num_features <= HEAD_MAX_FEATURES and self.num_features % 4 == 0
        if not self.head_kernel:
            import logging

            logging.getLogger("tiatoolbox_amd").warning(
                "FusedViTClassifier: the head kernel takes at most %d classes on at most %d features (a multiple of 4); this classifier "
                "is %d -> %d, so the Linear and the softmax run as torch operations (a library GEMM) on the float32 features.",
                HEAD_MAX_CLASSES, HEAD_MAX_FEATURES, self.num_features, self.num_classes)

    @property
    def half_dtype(self) -> torch.dtype | None:
        return self.feat_extract.half_dtype

    @property
    def smoothing(self) -> dict[str, torch.Tensor] | None:
        return self.feat_extract.smoothing

    @property
    def return_attention(self) -> str | None:
        return self.feat_extract.return_attention

    @return_attention.setter
    def return_attention(self, kind: str | None) -> None:
        self.feat_extract.return_attention = kind

    @property
    def attention_maps(self) -> torch.Tensor | None:
        """The backbone's maps of the forward that just ran (``FusedViT.attention_maps``); the head adds nothing to them."""
        return self.feat_extract.attention_maps

    def prepare(self, dtype: torch.dtype, linear_dtype: str | None = None, residual_dtype: str | None = None,
                smoothing: dict[str, torch.Tensor] | None = None) -> None:
        """``FusedViT.prepare`` of the backbone, every argument passed through (the head stays float32)."""
        self.feat_extract.prepare(dtype, linear_dtype=linear_dtype, residual_dtype=residual_dtype, smoothing=smoothing)

    def _head(self, feat: torch.Tensor) -> torch.Tensor:
        feat = torch.flatten(feat, 1)
        if self.head_kernel:
            return hip_linear_softmax_rows_f32(feat, self._w32, self._b32)
        return torch.softmax(torch.nn.functional.linear(feat, self._w32, self._b32), -1)

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        return self._head(self.feat_extract(imgs))

    def forward_uint8(self, x_u8_nhwc: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
        return self._head(self.feat_extract.forward_uint8(x_u8_nhwc, table))


def calibrate_int8_smoothing(vit_or_model: nn.Module, batches, *, alpha: float = 0.5) -> dict[str, torch.Tensor]:  # noqa: ANN001
    """The smoothing scales of ``prepare(torch.bfloat16, linear_dtype="int8", smoothing=...)`` for a loaded model on a CUDA device
    (a ``VisionTransformer``, or a ``TimmBackbone`` / ``TimmModel`` around one), calibrated on ``batches`` -- one batch or an iterable
    of them: normalised NCHW float tensors, or uint8 NHWC patches, which go through ``forward_uint8`` with the table of the model's
    ``preproc_func`` (a ``TimmNormPreproc``) as a run's batches do.

    A temporary :class:`FusedViT` runs the bfloat16 hand-written graph on them (``begin_int8_calibration``); the abs-max kernels tap
    the LayerNorm in front of ``qkv`` and ``fc1`` and the activation in front of ``fc2`` of every block, and
    :func:`int8_smoothing_scales` turns the statistics and the weight column maxima into powers of two.  Returns float32 CPU
    tensors ``[cin]`` under ``blocks.{i}.attn.qkv``, ``blocks.{i}.mlp.fc1`` and ``blocks.{i}.mlp.fc2`` (``fc2`` at its padded
    width) for the layers the INT8 GEMM serves: a plain dict that ``torch.save`` keeps -- how a deployment pins its calibration.
    Non-finite activations on the calibration data are a ``ValueError`` that names the layer."""
    import numpy as np

    alpha = _checked_alpha(alpha)
    vit = getattr(vit_or_model, "feat_extract", vit_or_model)
    fused = FusedViT(vit)
    fused.begin_int8_calibration()
    device = fused._cls32.device  # noqa: SLF001
    if isinstance(batches, (torch.Tensor, np.ndarray)):
        batches = [batches]
    hook = getattr(vit_or_model, "preproc_func", None)
    with torch.inference_mode():
        for batch in batches:
            t = torch.as_tensor(batch).to(device)
            if t.dtype == torch.uint8:
                if not hasattr(hook, "device_table"):
                    msg = ("calibrate_int8_smoothing: uint8 patches need the model's preproc_func (a TimmNormPreproc, whose table the "
                           "im2col looks the bytes up in); pass normalised NCHW float batches for a bare VisionTransformer.")
                    raise ValueError(msg)
                fused.forward_uint8(t, hook.device_table(device, torch.bfloat16))
            else:
                fused(t)
    return fused.int8_calibration_scales(alpha)

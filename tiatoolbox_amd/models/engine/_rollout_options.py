"""Head fusion and discard ratio of the attention rollout maps (the run kwargs ``attention_head_fusion`` and
``attention_discard_ratio``), stated once in NumPy.  ``VisionTransformer.forward_with_attention`` (plain torch) and ``FusedViT``
(``tia_mha_probs_fused_h``, ``tia_rollout_discard_normalize_f32``, ``tia_rollout_product_f32``) compute what is written here.

Per image and per block, everything float32; ``P`` ``[H, S, S]`` are the probabilities of the ``H`` heads:

1. ``F = fuse(P)``: "mean" adds the heads in ascending order and divides by ``H`` once; "max" / "min" are exact.
2. ``k = discard_count(r, S)``.  With ``k >= 1``, ``v`` is the ``k``-th smallest of the ``S * S`` entries of ``F`` (1-based, duplicates
   counted) and ``F'`` is ``F`` with zeros where ``F <= v``, except at ``(0, 0)`` -- every entry tied with ``v`` goes, so no sort's
   tie-break matters; flat index 0 is never discarded (the rule of the widely used ``vit-explain`` implementation).
3. "mean" with ``k == 0`` is the rollout as it was: ``R_l = (A_l R_{l-1}) / 2 + R_{l-1} / 2``, nothing renormalised.  Otherwise
   ``A^ = (F' + I) / 2``, every row divided by its sum (``row_sums``: a fixed order of float32 additions), ``R_1 = A^_1`` and
   ``R_l = A^_l R_{l-1}`` with every element one float32 fma chain over ``k = 0 .. S - 1`` in ascending order (``fma_matmul``).
4. The map is ``R_L[0, P:]`` on the patch grid.  Nothing else is renormalised (no division by the maximum).
"""

from __future__ import annotations

import numbers

import numpy as np

HEAD_FUSIONS = ("mean", "max", "min")
FUSION_CODES = {"mean": 0, "max": 1, "min": 2}  # TIA_FUSE_MEAN / _MAX / _MIN
LANES = 64  # partial sums of a row sum: one per lane of the wave that owns the row


def check_options(head_fusion, discard_ratio, *, who: str) -> tuple[str, float]:
    """``(fusion, ratio)`` as given, or a ``ValueError`` that names the option: a fusion outside the three names, a ratio that is not
    a real number in ``[0, 1)``."""
    if not isinstance(head_fusion, str) or head_fusion not in HEAD_FUSIONS:
        msg = f"{who}: attention_head_fusion is one of {HEAD_FUSIONS}; got {head_fusion!r}."
        raise ValueError(msg)
    real = isinstance(discard_ratio, numbers.Real) and not isinstance(discard_ratio, bool)
    if not real or not 0.0 <= float(discard_ratio) < 1.0:  # (NaN fails both comparisons)
        msg = f"{who}: attention_discard_ratio is a real number r with 0 <= r < 1; got {discard_ratio!r}."
        raise ValueError(msg)
    return head_fusion, float(discard_ratio)


def is_default(head_fusion: str, discard_ratio: float) -> bool:
    return head_fusion == "mean" and float(discard_ratio) == 0.0


def discard_count(discard_ratio: float, tokens: int) -> int:
    """``k = min(int(r * S^2), S^2 - 1)``, the product in float64."""
    total = tokens * tokens
    return min(int(float(discard_ratio) * float(total)), total - 1)


def fuse_heads(p: np.ndarray, head_fusion: str) -> np.ndarray:
    """``[..., H, S, S]`` float32 -> ``[..., S, S]``."""
    p = np.asarray(p, dtype=np.float32)
    if head_fusion == "max":
        return p.max(axis=-3)
    if head_fusion == "min":
        return p.min(axis=-3)
    acc = p[..., 0, :, :].copy()
    for h in range(1, p.shape[-3]):
        acc = acc + p[..., h, :, :]
    return acc / np.float32(p.shape[-3])


def kth_smallest(f: np.ndarray, k: int) -> np.ndarray:
    """The ``k``-th smallest (1-based) of the last two axes, ``[...]``."""
    flat = np.asarray(f, dtype=np.float32).reshape(*f.shape[:-2], -1)
    return np.partition(flat, k - 1, axis=-1)[..., k - 1]


def discard(f: np.ndarray, k: int) -> np.ndarray:
    f = np.asarray(f, dtype=np.float32)
    if k == 0:
        return f
    v = kth_smallest(f, k)[..., None, None]
    drop = f <= v
    drop[..., 0, 0] = False
    return np.where(drop, np.float32(0.0), f)


def row_sums(a: np.ndarray) -> np.ndarray:
    """``[..., S, S]`` -> ``[..., S]``: partial sum ``l`` (of 64) adds the entries ``j = l, l + 64, ...`` in ascending order to 0; the
    partial sums fold by ``p[l] += p[l ^ 32]``, then ``^ 16, 8, 4, 2, 1``; the sum is ``p[0]``."""
    a = np.asarray(a, dtype=np.float32)
    s = a.shape[-1]
    parts = np.zeros((*a.shape[:-1], LANES), dtype=np.float32)
    for j0 in range(0, s, LANES):
        chunk = a[..., j0:j0 + LANES]
        parts[..., :chunk.shape[-1]] += chunk
    lanes = np.arange(LANES)
    off = LANES // 2
    while off:
        parts = parts + parts[..., lanes ^ off]
        off //= 2
    return parts[..., 0]


def normalise(f_kept: np.ndarray) -> np.ndarray:
    """``A^ = (F' + I) / 2`` and every row divided by its :func:`row_sums`."""
    f_kept = np.asarray(f_kept, dtype=np.float32)
    a = (f_kept + np.eye(f_kept.shape[-1], dtype=np.float32)) * np.float32(0.5)
    return a / row_sums(a)[..., None]


def _fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """``round32(a * b + c)`` with one rounding, for float32 arrays with ``c >= 0`` and ``a * b >= 0``: the product is exact in
    float64, the float64 sum is rounded to odd (its error from the two-sum), and 53 bits rounded to odd then to 24 round once."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    bits = s.view(np.int64).copy()
    even = (bits & 1) == 0
    bits = np.where((err > 0) & even, bits + 1, np.where((err < 0) & even, bits - 1, bits))  # (s > 0 wherever err != 0)
    return bits.view(np.float64).astype(np.float32)


def fma_matmul(a: np.ndarray, r: np.ndarray) -> np.ndarray:
    """``a @ r`` on ``[..., S, S]`` float32 matrices of non-negative values, every element ``acc = fma(a[i, k], r[k, j], acc)`` from
    0 over ``k = 0 .. S - 1`` in ascending order."""
    a, r = np.asarray(a, dtype=np.float32), np.asarray(r, dtype=np.float32)
    acc = np.zeros(np.broadcast_shapes(a.shape, r.shape), dtype=np.float32)
    for k in range(a.shape[-1]):
        acc = _fma32(a[..., :, k:k + 1], r[..., k:k + 1, :], acc)
    return acc


def rollout(fused: list[np.ndarray], head_fusion: str, discard_ratio: float) -> np.ndarray:
    """``R_L`` ``[..., S, S]`` from the fused matrices ``F_1 .. F_L`` of the blocks (item 3 of the module's statement)."""
    s = fused[0].shape[-1]
    k = discard_count(discard_ratio, s)
    r = None
    if head_fusion == "mean" and k == 0:
        half = np.float32(0.5)
        for f in fused:
            f = np.asarray(f, dtype=np.float32)
            prev = np.broadcast_to(np.eye(s, dtype=np.float32), f.shape) if r is None else r
            r = half * fma_matmul(f, prev) + half * prev
        return r
    for f in fused:
        a = normalise(discard(f, k))
        r = a if r is None else fma_matmul(a, r)
    return r

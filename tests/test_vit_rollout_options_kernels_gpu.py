"""The kernels behind ``attention_head_fusion`` / ``attention_discard_ratio`` (``csrc/vit_attention_maps.hip``), every case compared
with ``np.array_equal``: ``tia_mha_probs_fused_h`` against ``tia_mha_probs_h``; ``tia_rollout_discard_normalize_f32`` against the
NumPy restatement in ``_vit_rollout_options_ref`` on inputs made to tie; ``tia_rollout_product_f32`` on integer-valued operands;
the entry points' refusals."""

from __future__ import annotations

import numpy as np
import pytest
import torch
from _vit_rollout_options_ref import SELECTION_KINDS, TIED_KINDS, a_hat, discard_count, selection_input, threshold

pytestmark = pytest.mark.gpu

EINVAL, ESIZE = -1, -3
DTYPES = [torch.float16, torch.bfloat16]


def _qkv(n: int, heads: int, s: int, hd: int, dtype: torch.dtype) -> torch.Tensor:
    g = torch.Generator().manual_seed(s * 131 + hd * 7 + heads)
    qkv = torch.randn((n, s, 3, heads, hd), generator=g)
    qkv[:, :, 0] *= 0.6
    return qkv.to(dtype).reshape(n, s, 3 * heads * hd).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize(("n", "heads", "s"), [(2, 3, 1), (2, 3, 2), (2, 3, 17), (2, 3, 65), (2, 3, 197), (1, 16, 197)])
def test_fused_probabilities_equal_the_existing_entry(n, heads, s, hd, dtype):
    """"mean" is ``tia_mha_probs_h(head_mean=1)`` and "max" / "min" the element-wise maximum / minimum of ``head_mean=0``: bit for bit."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_mha_probs_fused_h, hip_mha_probs_h

    qkv, scale = _qkv(n, heads, s, hd, dtype), hd ** -0.5
    per_head = hip_mha_probs_h(qkv, heads, scale, q_rows=s, head_mean=False).cpu().numpy()
    mean = hip_mha_probs_h(qkv, heads, scale, q_rows=s, head_mean=True).cpu().numpy()
    want = {"mean": mean, "max": per_head.max(axis=1), "min": per_head.min(axis=1)}
    for fusion, ref in want.items():
        got = hip_mha_probs_fused_h(qkv, heads, scale, fusion)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, s, s)
        assert np.array_equal(got.cpu().numpy(), ref), (fusion, int((got.cpu().numpy() != ref).sum()))
    if s > 1:
        assert not np.array_equal(want["max"], want["min"])


def _counts(s: int) -> list[int]:
    return sorted({discard_count(r, s) for r in (0.5, 0.9, 0.999)} | {min(1, s * s - 1), s * s - 1})


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("s", [1, 2, 5, 17, 65, 197, 257])
def test_discard_and_normalise_equal_the_reference(s, n):
    """``r`` in {0.5, 0.9, 0.999} and the edges ``k = 1``, ``k = S^2 - 1`` (``k = 0`` where ``S = 1`` leaves nothing else), on five
    kinds of input.  On the tied inputs the reference alone first shows that ``<`` in place of ``<=`` changes the output for some
    ``k``, so that equality with it tests the rule."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_rollout_discard_normalize_f32

    for kind in SELECTION_KINDS:
        f = selection_input(kind, n, s)
        dev = torch.from_numpy(f).cuda()
        told = False
        for k in _counts(s):
            ref = a_hat(f, k)
            if kind in TIED_KINDS and k:
                told = told or not np.array_equal(ref, a_hat(f, k, strict=True))
            got, v = hip_rollout_discard_normalize_f32(dev, k, return_threshold=True)
            if k:
                assert np.array_equal(v.cpu().numpy(), threshold(f, k)), (kind, k)
            assert np.array_equal(got.cpu().numpy(), ref), (kind, k, int((got.cpu().numpy() != ref).sum()))
        assert torch.equal(dev.cpu(), torch.from_numpy(f))  # the input is not written
        if kind in TIED_KINDS and s >= 5:  # noqa: PLR2004  (from 25 entries on every tied input has a k with a tie at v)
            assert told, kind


@pytest.mark.parametrize("s", [1, 5, 17, 65, 197])
def test_product_of_integer_valued_operands_is_exact(s):
    """Operands of integers 0 .. 15: every product and partial sum is an integer below 2^24, so any correct fma chain gives the exact
    ``A R``; ``d_r_in`` NULL gives ``A`` itself."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_rollout_product_f32

    rng = np.random.default_rng(s)
    a, r = rng.integers(0, 16, (2, s, s)), rng.integers(0, 16, (2, s, s))
    da, dr = torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(r.astype(np.float32)).cuda()
    got = hip_rollout_product_f32(da, dr)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), (a @ r).astype(np.float32))
    assert np.array_equal(hip_rollout_product_f32(da, None).cpu().numpy(), a.astype(np.float32))
    soft = torch.softmax(torch.randn((2, s, s), generator=torch.Generator().manual_seed(s)), -1).cuda()
    assert torch.equal(hip_rollout_product_f32(soft, None), soft)


def test_refusals_launch_nothing():
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.vit_fused import (MHA_PROBS_MEAN_HEADS, hip_mha_probs_fused_h, hip_rollout_discard_normalize_f32,
                                                               hip_rollout_product_f32)

    lib, stream = _lib.load(), _lib.current_stream()
    n, s, heads, hd, sentinel = 2, 5, 2, 64, 77.0
    qkv = torch.zeros((n, s, 3 * heads * hd), dtype=torch.bfloat16, device="cuda")
    f = torch.rand((n, s, s), device="cuda")
    out = torch.full((n * s * s + 8,), sentinel, device="cuda")
    v = torch.full((n + 2,), sentinel, device="cuda")
    q, pf, po, pv, bf = qkv.data_ptr(), f.data_ptr(), out.data_ptr(), v.data_ptr(), 2

    def probs(q=q, o=po, n=n, s=s, heads=heads, hd=hd, scale=0.125, fusion=1, dtype=bf):  # noqa: PLR0913
        return lib.tia_mha_probs_fused_h(q, o, n, s, heads, hd, scale, fusion, dtype, stream)

    assert probs(q=0) == EINVAL and probs(o=0) == EINVAL and probs(q=q + 2) == EINVAL and probs(o=po + 4) == EINVAL
    assert probs(fusion=3) == EINVAL and probs(fusion=-1) == EINVAL and probs(dtype=0) == EINVAL
    assert probs(scale=0.0) == EINVAL and probs(n=0) == EINVAL and probs(s=0) == EINVAL
    assert probs(hd=96) == ESIZE
    for fusion in (0, 1, 2):
        assert probs(heads=MHA_PROBS_MEAN_HEADS + 1, fusion=fusion) == ESIZE

    def select(f=pf, o=po, v=pv, n=n, s=s, k=3):  # noqa: PLR0913
        return lib.tia_rollout_discard_normalize_f32(f, o, v, n, s, k, stream)

    assert select(f=0) == EINVAL and select(o=0) == EINVAL and select(v=0) == EINVAL
    assert select(f=pf + 2) == EINVAL and select(o=po + 1) == EINVAL and select(v=pv + 2) == EINVAL
    assert select(n=0) == EINVAL and select(s=0) == EINVAL and select(k=-1) == EINVAL
    assert select(k=s * s) == EINVAL and select(k=s * s + 7) == EINVAL
    assert select(s=1, k=1) == EINVAL                                # k >= S^2 at S = 1
    assert select(s=65536, k=1) == ESIZE
    assert select(o=pf) == EINVAL and select(o=pf + 4 * s * s) == EINVAL  # the output on the input, and on its second matrix
    assert select(v=pf + 4) == EINVAL and select(v=po + 4 * (n * s * s - 1)) == EINVAL  # the thresholds inside either

    def product(a=pf, r=pf, o=po, n=n, s=s):
        return lib.tia_rollout_product_f32(a, r, o, n, s, stream)

    assert product(a=0) == EINVAL and product(o=0) == EINVAL and product(a=pf + 2) == EINVAL
    assert product(n=0) == EINVAL and product(s=0) == EINVAL
    assert product(o=pf) == EINVAL and product(r=po) == EINVAL and product(o=pf + 4 * s * s) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((v == sentinel).all())  # no refusal launched anything
    assert select(v=0, k=0) == 0 and select() == 0 and product(r=0) == 0 and probs() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="head_fusion is one of"):
        hip_mha_probs_fused_h(qkv, heads, 0.125, "sum")
    wide = torch.zeros((1, 2, 3 * (MHA_PROBS_MEAN_HEADS + 1) * 64), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match=f"at most {MHA_PROBS_MEAN_HEADS} heads"):
        hip_mha_probs_fused_h(wide, MHA_PROBS_MEAN_HEADS + 1, 0.125, "max")
    with pytest.raises(ValueError, match="k is between 0 and"):
        hip_rollout_discard_normalize_f32(f, s * s)
    with pytest.raises(ValueError, match="contiguous float32 CUDA"):
        hip_rollout_discard_normalize_f32(f.half(), 1)
    with pytest.raises(ValueError, match="contiguous float32 CUDA"):
        hip_rollout_product_f32(f, f[:, :4, :4])

"""The two kernels of the Vision Transformer classifiers: ``tia_vit_patchify_norm_u8_h`` (uint8 patches -> normalised half tokens, a
gather: compared bit for bit with the existing im2col of the hook's batched form) and ``tia_linear_softmax_rows_f32`` (the head:
against float64 with the summation bound of ``_vit_classifier_ref.head64``); their refusals."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _vit_classifier_ref import all_bytes_batch, head64

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


def _lib():
    from tiatoolbox_amd import _lib as lib

    return lib


def _dt(dtype: torch.dtype) -> int:
    from tiatoolbox_amd.models.architecture.fused import _DT

    return _DT[dtype]


def _hook():
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    return timm_preproc_func("H-optimus-0")  # three different means and deviations: a channel mix-up shows


def _expected(x: torch.Tensor, p: int, k_pad: int, dtype: torch.dtype) -> torch.Tensor:
    """The existing im2col kernels on the hook's batched device form (a torch gather in ``dtype``)."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_patchify_h, hip_vit_patchify_pad_h

    normed = _hook().device_batch(x, dtype).contiguous()
    if k_pad == 3 * p * p and p % 8 == 0:
        return hip_vit_patchify_h(normed, p, dtype)
    return hip_vit_patchify_pad_h(normed, p, k_pad, dtype)


def _patchify_norm(x: torch.Tensor, p: int, k_pad: int, dtype: torch.dtype) -> torch.Tensor:
    """The entry point into a buffer pre-filled with NaN: every element of it has to be written."""
    lib = _lib()
    n, h, w, _ = x.shape
    table = _hook().device_table(x.device, dtype)
    out = torch.full((n, (h // p) * (w // p), k_pad), float("nan"), dtype=dtype, device="cuda")
    rc = lib.load().tia_vit_patchify_norm_u8_h(x.data_ptr(), table.data_ptr(), out.data_ptr(), n, h, w, p, k_pad, _dt(dtype), lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize(("h", "w", "p", "k_pad"), [(32, 32, 16, 768), (48, 64, 16, 768), (28, 42, 14, 608)])
@pytest.mark.parametrize("n", [1, 3])
def test_normalising_patchify_is_the_gather_bit_for_bit(n, h, w, p, k_pad, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_patchify_norm_u8_h

    x = torch.from_numpy(all_bytes_batch(n, h, w, seed=h + w + n)).cuda()
    exp = _expected(x, p, k_pad, dtype)
    tok = _patchify_norm(x, p, k_pad, dtype)
    assert tok.dtype == dtype and tok.shape == exp.shape and torch.equal(tok.view(torch.int16), exp.view(torch.int16))
    assert bool((tok[:, :, 3 * p * p:].view(torch.int16) == 0).all())  # +0, bit for bit (28 x 42: columns 588 .. 607)
    wrapped = hip_vit_patchify_norm_u8_h(x, _hook().device_table("cuda", dtype), p, k_pad, dtype)
    assert torch.equal(wrapped.view(torch.int16), exp.view(torch.int16))
    if p == 14:  # noqa: PLR2004  the same batch as a view 1 and 3 bytes into a larger buffer: a row pitch of 126 bytes off every alignment
        for off in (1, 3):
            buf = torch.zeros(x.numel() + 8, dtype=torch.uint8, device="cuda")
            view = buf[off:off + x.numel()].view(x.shape)
            view.copy_(x)
            assert view.data_ptr() % 4 == off and view.is_contiguous()
            assert torch.equal(_patchify_norm(view, p, k_pad, dtype).view(torch.int16), exp.view(torch.int16)), off
            assert torch.equal(hip_vit_patchify_norm_u8_h(view, _hook().device_table("cuda", dtype), p, k_pad, dtype).view(torch.int16),
                               exp.view(torch.int16)), off


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_normalising_patchify_at_224(dtype):
    x = torch.from_numpy(all_bytes_batch(2, 224, 224, seed=224)).cuda()
    assert torch.equal(_patchify_norm(x, 16, 768, dtype).view(torch.int16), _expected(x, 16, 768, dtype).view(torch.int16))
    assert torch.equal(_patchify_norm(x, 14, 608, dtype).view(torch.int16), _expected(x, 14, 608, dtype).view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------------------
# the head
# ------------------------------------------------------------------------------------------------------------------------------------
def _head(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None, rows: int, stride: int) -> torch.Tensor:
    lib = _lib()
    c, f = w.shape
    out = torch.full((rows, c), float("nan"), device="cuda")
    rc = lib.load().tia_linear_softmax_rows_f32(x.data_ptr(), stride, w.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(),
                                                rows, f, c, lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _head_case(rows: int, f: int, c: int, stride: int | None = None):
    g = torch.Generator().manual_seed(f * 1000 + c)
    stride = stride or f
    x = torch.randn((257, stride), generator=g)[:rows].contiguous()  # (the first rows of ONE draw: row r is the same in every launch)
    w = torch.randn((c, f), generator=g) * (2.0 / f ** 0.5)
    b = torch.randn(c, generator=g) * 0.1
    return x, w, b


@pytest.mark.parametrize("c", [1, 2, 9, 64])
@pytest.mark.parametrize("f", [128, 384, 1024, 1536, 2560])
def test_head_matches_float64(f, c):
    full = None
    for rows in (257, 3, 1):
        x, w, b = _head_case(rows, f, c)
        got = _head(x.cuda(), w.cuda(), b.cuda(), rows, f).cpu()
        p64, bound = head64(x, w, b)
        err = (got.double() - p64).abs().max(dim=1).values
        print(f"head f={f} c={c} rows={rows}: max err {float(err.max()):.3e}  bound {float(bound.max()):.3e}")
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (float(err.max()), float(bound.min()))
        if c == 1:
            assert bool((got == 1.0).all())
        else:
            # one division each by a sum folded in 6 steps: the exact sum of a row is within 7 units of 1
            assert float(got.max()) <= 1.0 and float((got.double().sum(-1) - 1).abs().max()) <= (c + 8) * 2.0 ** -24
        if full is None:
            full = got
        else:  # a row's result does not depend on the batch it is in
            assert torch.equal(got, full[:rows])
    x, w, b = _head_case(257, f, c)
    for r in (5, 256):
        assert torch.equal(_head(x[r:r + 1].cuda(), w.cuda(), b.cuda(), 1, f).cpu(), full[r:r + 1]), r


def test_head_at_a_row_stride_without_a_bias_and_through_the_wrapper():
    from tiatoolbox_amd.models.architecture.vit_fused import hip_linear_softmax_rows_f32

    f, c, stride, rows = 384, 9, 1000, 7
    x, w, b = _head_case(rows, f, c, stride)
    dense = x[:, :f].contiguous()
    for bias in (b, None):
        p64, bound = head64(dense, w, bias)
        got = _head(x.cuda(), w.cuda(), bias.cuda() if bias is not None else None, rows, stride).cpu()
        assert bool(((got.double() - p64).abs().max(dim=1).values <= bound).all())
        assert torch.equal(got, _head(dense.cuda(), w.cuda(), bias.cuda() if bias is not None else None, rows, f).cpu())
        view = x.cuda()[:, :f]  # the rows as a strided view
        assert torch.equal(hip_linear_softmax_rows_f32(view, w.cuda(), bias.cuda() if bias is not None else None).cpu(), got)
    with pytest.raises(ValueError, match="float32 CUDA rows"):
        hip_linear_softmax_rows_f32(dense.cuda().half(), w.cuda(), None)
    with pytest.raises(_lib().HipLibraryError, match="tia_linear_softmax_rows_f32"):
        hip_linear_softmax_rows_f32(torch.zeros((2, 128), device="cuda"), torch.zeros((65, 128), device="cuda"), None)


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_launching():
    lib_mod = _lib()
    lib, stream = lib_mod.load(), lib_mod.current_stream()
    einval, esize, f32, f16 = lib_mod.TIA_EINVAL, lib_mod.TIA_ESIZE, 0, 1
    # --- tia_vit_patchify_norm_u8_h
    img = torch.zeros((1, 28, 28, 3), device="cuda", dtype=torch.uint8)
    table = torch.zeros((256 * 3 + 8,), device="cuda", dtype=torch.float16)
    tok = torch.full((1, 4, 608), 7.0, device="cuda", dtype=torch.float16)
    ok = (img.data_ptr(), table.data_ptr(), tok.data_ptr(), 1, 28, 28, 14, 608, f16)

    def patchify(**over):
        names = ("x", "table", "tokens", "n", "h", "w", "patch", "k_pad", "dtype")
        return lib.tia_vit_patchify_norm_u8_h(*[over.get(k, v) for k, v in zip(names, ok)], stream)

    assert patchify(dtype=f32) == einval and patchify(dtype=3) == einval
    assert patchify(x=None) == einval and patchify(table=None) == einval and patchify(tokens=None) == einval
    assert patchify(table=table.data_ptr() + 2) == einval and patchify(tokens=tok.data_ptr() + 8) == einval  # misaligned
    assert patchify(n=0) == einval and patchify(h=-28) == einval and patchify(w=0) == einval
    assert patchify(patch=0) == einval and patchify(k_pad=0) == einval
    assert patchify(k_pad=600) == esize   # k_pad % 32
    assert patchify(k_pad=576) == esize   # k_pad < 3 p^2 = 588
    assert patchify(h=30) == esize and patchify(w=21) == esize  # h % patch, w % patch
    torch.cuda.synchronize()
    assert bool((tok == 7.0).all())  # noqa: PLR2004  (nothing was launched)
    assert patchify() == 0
    # --- tia_linear_softmax_rows_f32
    x, w, b = torch.zeros((2, 136), device="cuda"), torch.zeros((65, 136), device="cuda"), torch.zeros(65, device="cuda")
    p = torch.full((2, 65), 7.0, device="cuda")
    ok = (x.data_ptr(), 136, w.data_ptr(), b.data_ptr(), p.data_ptr(), 2, 128, 9)

    def head(**over):
        names = ("x", "stride", "w", "bias", "p", "rows", "f", "c")
        return lib.tia_linear_softmax_rows_f32(*[over.get(k, v) for k, v in zip(names, ok)], stream)

    assert head(c=65) == esize and head(f=130, stride=132) == esize and head(f=8196, stride=8196) == esize
    assert head(x=None) == einval and head(w=None) == einval and head(p=None) == einval
    assert head(rows=0) == einval and head(f=0) == einval and head(c=0) == einval
    assert head(stride=124) == einval and head(stride=130) == einval              # shorter than a row; rows off the 16-byte vectors
    assert head(x=x.data_ptr() + 4) == einval and head(w=w.data_ptr() + 8) == einval and head(p=p.data_ptr() + 2) == einval
    torch.cuda.synchronize()
    assert bool((p == 7.0).all())  # noqa: PLR2004
    assert head() == 0 and head(bias=None) == 0 and head(c=64) == 0 and head(c=1) == 0
    torch.cuda.synchronize()

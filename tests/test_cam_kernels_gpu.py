"""``tia_cam_nhwc_f32`` / ``tia_cam_nhwc_h`` (``csrc/cnn_cam.hip``; ``architecture/fused.py``: ``hip_cam``) against float64 on the inputs
as stored -- for the half forms: the half values, widened --, batch invariance bit for bit, and every refusal.

The bound per entry, with ``S = sum_c |w x|`` in float64: ``|got - ref| <= (c + 8) 2^-24 S + 2^-120``.  Every order of ``c`` float32
multiply-adds, fused or not, satisfies it to first order; the 8 is slack for the second-order term (below 0.3 units at c = 4096).  It is
derived, not measured."""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
GRIDS = {1: (1, 1), 15: (3, 5), 49: (7, 7), 64: (8, 8)}


def _inputs(n: int, c: int, hw: int, k: int, dtype: torch.dtype, seed: int):
    """``x = |N(0, 1)|`` ``[n, c, h, w]`` channels-last in ``dtype`` and ``w = N(0, 1)`` ``[k, c]`` float32, on the device."""
    g = torch.Generator().manual_seed(seed)
    h, w = GRIDS[hw]
    x = torch.randn((n, h, w, c), generator=g).abs().to(dtype).permute(0, 3, 1, 2)  # the NCHW view of an NHWC batch
    return x.cuda(), torch.randn((k, c), generator=g).cuda()


def check_against_float64(got: torch.Tensor, x: torch.Tensor, weight: torch.Tensor) -> float:
    """Asserts the bound for every entry; returns the largest error in units of the bound."""
    xf, wf = x.detach().double().cpu(), weight.detach().double().cpu()
    ref = torch.einsum("kc,nchw->nkhw", wf, xf)
    s = torch.einsum("kc,nchw->nkhw", wf.abs(), xf.abs())
    bound = (x.shape[1] + 8) * U * s + 2.0 ** -120
    err = (got.detach().double().cpu() - ref).abs()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    assert bool((err <= bound).all()), float((err / bound).max())
    return float((err / bound).max())


@pytest.mark.parametrize("c", [64, 512, 2048])
@pytest.mark.parametrize("name", list(DTYPES))
def test_kernel_against_float64(name, c):
    from tiatoolbox_amd.models.architecture.fused import hip_cam

    worst = 0.0
    for hw in GRIDS:
        for k in (1, 2, 9, 33):
            for n in (1, 3):
                x, w = _inputs(n, c, hw, k, DTYPES[name], seed=c + 7 * hw + 13 * k + n)
                assert x.is_contiguous(memory_format=torch.channels_last)
                worst = max(worst, check_against_float64(hip_cam(x, w), x, w))
    print(f"{name} c={c}: largest error {worst:.3f} of the bound")


@pytest.mark.parametrize("name", list(DTYPES))
def test_large_channel_counts_and_class_tiles(name):
    """c = 4096 (nine classes in one tile of LDS) and c = 8192 with more classes than a tile holds; a row count that is no multiple of
    the four rows a wave takes, over more than one workgroup."""
    from tiatoolbox_amd.models.architecture.fused import hip_cam

    for n, c, k, hw in ((2, 4096, 9, 49), (1, 8192, 9, 15), (37, 512, 5, 49), (3, 2048, 13, 49)):
        x, w = _inputs(n, c, hw, k, DTYPES[name], seed=c + k)
        check_against_float64(hip_cam(x, w), x, w)


@pytest.mark.parametrize("c", [512, 2048])
@pytest.mark.parametrize("name", list(DTYPES))
def test_batch_invariance(name, c):
    """Patch ``i`` alone, and inside batches of 3 and 7 at two positions each, gives identical bits."""
    from tiatoolbox_amd.models.architecture.fused import hip_cam

    x, w = _inputs(7, c, 49, 9, DTYPES[name], seed=c)
    alone = hip_cam(x[2:3], w)
    whole = hip_cam(x, w)
    assert torch.equal(whole[2:3], alone)
    for order in ([2, 0, 1], [5, 6, 2], [0, 1, 3, 2, 4, 5, 6], [6, 5, 4, 3, 1, 0, 2]):
        batch = x[order].contiguous(memory_format=torch.channels_last)
        assert torch.equal(hip_cam(batch, w)[order.index(2)], alone[0]), order


def test_layouts_and_out():
    """An NCHW-contiguous feature map is copied to channels-last and gives the same bits; ``out=`` is written in place."""
    from tiatoolbox_amd.models.architecture.fused import hip_cam

    x, w = _inputs(3, 512, 49, 9, torch.float32, seed=1)
    got = hip_cam(x, w)
    assert torch.equal(hip_cam(x.contiguous(), w), got)
    buf = torch.full((5, 9, 7, 7), float("nan"), device="cuda")
    assert hip_cam(x, w, out=buf[1:4]).data_ptr() == buf[1:4].data_ptr()
    assert torch.equal(buf[1:4], got) and bool(buf[0].isnan().all()) and bool(buf[4].isnan().all())
    with pytest.raises(ValueError, match="`out` must be"):
        hip_cam(x, w, out=buf)


def test_wrapper_refusals():
    from tiatoolbox_amd.models.architecture.fused import hip_cam

    x, w = _inputs(1, 64, 15, 2, torch.float32, seed=0)
    with pytest.raises(ValueError, match="CUDA tensors"):
        hip_cam(x.cpu(), w)
    with pytest.raises(ValueError, match="CUDA tensors"):
        hip_cam(x, w.cpu())
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        hip_cam(x.double(), w)
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        hip_cam(x[0], w)
    with pytest.raises(ValueError, match="64 channels and the weights 32"):
        hip_cam(x, w[:, :32].contiguous())
    with pytest.raises(ValueError, match="float32 weights"):
        hip_cam(x, w.half())
    with pytest.raises(ValueError, match="float32 weights"):
        hip_cam(x.half(), w.half())
    for c in (96, 8256):
        xc, wc = torch.zeros((1, c, 2, 2), device="cuda").contiguous(memory_format=torch.channels_last), torch.zeros((2, c), device="cuda")
        with pytest.raises(ValueError, match=f"multiples of 64 up to 8192 .*got C = {c}"):
            hip_cam(xc, wc)
        with pytest.raises(ValueError, match="multiples of 64 up to 8192"):
            hip_cam(xc.bfloat16(), wc)


def test_abi_return_codes():
    """Checked before any launch: the output stays as it was."""
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    x = torch.ones((2, 4, 128), device="cuda")
    xh = x.half()
    w = torch.ones((3, 128), device="cuda")
    out = torch.full((2, 3, 4), 7.0, device="cuda")
    ptr = (x.data_ptr(), w.data_ptr(), out.data_ptr())
    assert lib.tia_cam_nhwc_f32(*ptr, 0, 4, 128, 3, None) == _lib.TIA_EINVAL
    assert lib.tia_cam_nhwc_f32(*ptr, 2, 0, 128, 3, None) == _lib.TIA_EINVAL
    assert lib.tia_cam_nhwc_f32(*ptr, 2, 4, 128, -1, None) == _lib.TIA_EINVAL
    assert lib.tia_cam_nhwc_f32(*ptr, 2, 4, 96, 3, None) == _lib.TIA_ESIZE
    assert lib.tia_cam_nhwc_f32(*ptr, 2, 4, 8256, 3, None) == _lib.TIA_ESIZE
    for null in range(3):
        args = [None if i == null else p for i, p in enumerate(ptr)]
        assert lib.tia_cam_nhwc_f32(*args, 2, 4, 128, 3, None) == _lib.TIA_EINVAL
        args[0] = None if null == 0 else xh.data_ptr()
        assert lib.tia_cam_nhwc_h(*args, 2, 4, 128, 3, 1, None) == _lib.TIA_EINVAL
    assert lib.tia_cam_nhwc_f32(ptr[0] + 4, ptr[1], ptr[2], 2, 4, 128, 3, None) == _lib.TIA_EINVAL  # a misaligned feature map
    hptr = (xh.data_ptr(), w.data_ptr(), out.data_ptr())
    assert lib.tia_cam_nhwc_h(*hptr, 0, 4, 128, 3, 1, None) == _lib.TIA_EINVAL
    assert lib.tia_cam_nhwc_h(*hptr, 2, 4, 96, 3, 2, None) == _lib.TIA_ESIZE
    assert lib.tia_cam_nhwc_h(*hptr, 2, 4, 128, 3, 0, None) == _lib.TIA_EINVAL  # TIA_DT_F32 is the other entry point
    assert lib.tia_cam_nhwc_h(*hptr, 2, 4, 128, 3, 3, None) == _lib.TIA_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert lib.tia_cam_nhwc_f32(*ptr, 2, 4, 128, 3, torch.cuda.current_stream().cuda_stream) == 0
    assert lib.tia_cam_nhwc_h(*hptr, 2, 4, 128, 3, 1, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((out == 128.0).all()) and lib.tia_abi_version() == 6  # noqa: PLR2004

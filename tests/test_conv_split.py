"""The split-operand convolution on the bf16 matrix cores (``conv_ring_bf16x3_kernel``), on the host: an emulation of its
arithmetic against float64, the exact three-part split of the activations, the packed weight layout, and the exact cases of
``test_conv_split_gpu.py`` as the emulation predicts them."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _conv_split_cases import (DROPPED, GEOMETRIES, ORDER, case_integers, case_mid_mid, case_power_of_two_activations, case_single_tap,
                               emulate_conv, emulate_gemm, packed_index)
from tiatoolbox_amd.models.architecture.fused import split_stem_weights


def _operands(k: int, seed: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """``relu(randn)`` activations [64, K] and ``randn / sqrt(K)`` weights [K, 32] (K = 576 / 4608: 9 cin of resnet18's layers 2 / 4)."""
    g = torch.Generator().manual_seed(seed + k)
    return torch.relu(torch.randn((64, k), generator=g)), torch.randn((k, 32), generator=g) / k ** 0.5


@pytest.fixture(scope="module", params=[16, 576, 4608])
def gemm(request):
    a, w = _operands(request.param)
    return request.param, a, w, a.double() @ w.double()


def test_emulated_kernel_arithmetic_is_within_the_summation_order_gate(gemm):
    """Six products in the kernel's order, float32 accumulation per 16-k step, against float64: within 1e-5 of max |y| (the gate of
    ``test_engine.py::test_winograd_conv_matches_torch_cpu_fp32``), and of the size of torch's own float32 matmul error."""
    k, a, w, ref = gemm
    err = ((emulate_gemm(a, w).double() - ref).abs().max() / ref.abs().max()).item()
    err_f32 = (((a @ w).double() - ref).abs().max() / ref.abs().max()).item()
    print(f"K = {k}: six products, float32 accumulation {err:.2e}; torch float32 matmul {err_f32:.2e}")
    assert err <= 1e-5, err


def test_dropped_terms_are_below_one_float32_ulp_of_the_products(gemm):
    """With exact accumulation what is left is mid lo + lo mid + lo lo: at most 2^-23 sum |a| |w|, element by element."""
    k, a, w, ref = gemm
    six = emulate_gemm(a, w, fp64_accumulate=True)
    bound = 2.0 ** -23 * (a.double().abs() @ w.double().abs())
    assert bool(((six - ref).abs() <= bound).all()), ((six - ref).abs() / bound).max().item()
    # ... and they ARE the difference: the nine products are the product (float64 holds every term and these sums)
    nine = six + emulate_gemm(a, w, terms=DROPPED, fp64_accumulate=True)
    assert ((nine - ref).abs().max() / ref.abs().max()).item() < 1e-13
    assert len(ORDER) + len(DROPPED) == 9 and not set(ORDER) & set(DROPPED)  # noqa: PLR2004


def _kernel_split_np(v: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The kernel's instruction sequence on one value, on the bit patterns: v_cvt_pk_bf16_f32 (round to nearest even), the part as a
    float32 again (shift / mask), v_sub_f32, twice, and a third conversion."""
    def cvt(x: np.ndarray) -> np.ndarray:
        u = x.view(np.uint32).astype(np.uint64)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint32)

    def as_f32(h: np.ndarray) -> np.ndarray:
        return (h << np.uint32(16)).view(np.float32)

    v = v.astype(np.float32)
    hi = cvt(v)
    r1 = v - as_f32(hi)
    mid = cvt(r1)
    lo = cvt(r1 - as_f32(mid))
    return as_f32(hi), as_f32(mid), as_f32(lo)


def test_activation_split_is_exact_for_every_mantissa_and_sign_at_one_exponent():
    """All 2^24 sign x mantissa patterns at the biased exponent 127 (|a| in [1, 2): post-ReLU activations of a BN-folded trunk), in
    the kernel's instruction sequence, and against ``split_stem_weights`` (which the emulation uses)."""
    for sign in (0, 1):
        for lo_half in (0, 1):  # two halves of the mantissa range: 2^22 values at a time keep the temporaries small
            mant = np.arange(lo_half << 22, (lo_half + 1) << 22, dtype=np.uint32)
            v = (mant | np.uint32(127 << 23) | np.uint32(sign << 31)).view(np.float32)
            hi, mid, lo = _kernel_split_np(v)
            assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), v.astype(np.float64))
            for part in (hi, mid, lo):
                assert not (part.view(np.uint32) & 0xFFFF).any()
            sub = slice(0, 1 << 20)
            parts, usable = split_stem_weights(torch.from_numpy(v[sub].copy()))
            assert usable
            assert np.array_equal(parts[0].numpy(), hi[sub]) and np.array_equal(parts[1].numpy(), mid[sub]) and np.array_equal(parts[2].numpy(), lo[sub])


def test_activation_split_of_special_values():
    special = np.array([0.0, -0.0, 1.0, -2.0, 2.0 ** -20, 2.0 ** 20, 2.0 ** -100, 1.0 - 2.0 ** -24, 2.0 - 2.0 ** -23, 1.0 + 2.0 ** -10, 2047.0, -2048.0,
                        1.0 / 3.0, 3.39e38], dtype=np.float32)
    hi, mid, lo = _kernel_split_np(special)
    assert np.array_equal(hi.astype(np.float64) + mid + lo, special.astype(np.float64))
    assert hi[9] == 1.0 and mid[9] == 2.0 ** -10 and lo[9] == 0.0
    # the largest bf16 number is 2^127 (2 - 2^-7) = 3.3895e38: 3.39e38 still rounds to it (an exact, finite split); from
    # 2^127 (2 - 2^-8) = 3.3961e38 on hi is infinite, v - hi = -inf and the third part inf - inf = NaN
    assert np.isfinite(hi[13])
    with np.errstate(invalid="ignore", over="ignore"):
        for bad in (3.4e38, np.inf, -np.inf, np.nan):
            hi, mid, lo = _kernel_split_np(np.array([bad], dtype=np.float32))
            assert not np.isfinite(hi[0]) and np.isnan(lo[0])


@pytest.mark.parametrize(("cout", "cin", "k"), [(128, 16, 1), (256, 48, 3), (128, 64, 5)])
def test_packed_layout_round_trips(cout, cin, k):
    """The index formula of ``tia_conv_pack_weights_bf16x3`` restated: it is a permutation of the parts, a stage (tap, slice, column
    tile) is 12 KB contiguous, and a lane's eight k values of a column are 16 contiguous bytes."""
    idx = packed_index(cout, cin, k, k)
    assert tuple(idx.shape) == (k, k, cin // 16, cout // 128, 3, 2, 128, 8)
    flat = idx.reshape(-1)
    assert torch.equal(flat.sort().values, torch.arange(3 * cout * cin * k * k))
    assert idx[0, 0, 0, 0].numel() * 2 == 12 * 1024  # noqa: PLR2004
    parts = torch.arange(3 * cout * cin * k * k).reshape(3, cout, cin, k, k)
    packed = parts.reshape(-1)[flat].reshape(idx.shape)
    for ty, tx, cs, ct, p, q, c, e in ((0, 0, 0, 0, 0, 0, 0, 0), (k - 1, k // 2, cin // 16 - 1, cout // 128 - 1, 2, 1, 127, 7), (k // 2, 0, 0, 0, 1, 1, 33, 5)):
        assert packed[ty, tx, cs, ct, p, q, c, e] == parts[p, 128 * ct + c, 16 * cs + 8 * q + e, ty, tx]
    # round trip: scatter the packed values back
    back = torch.empty_like(parts.reshape(-1))
    back[flat] = packed.reshape(-1)
    assert torch.equal(back.reshape(parts.shape), parts)


@pytest.mark.parametrize("bad", [1e-36, float("nan"), float("inf")])
def test_weights_without_a_usable_split_are_not_packed(bad):
    from tiatoolbox_amd.models.architecture.fused import pack_conv_weights_split

    conv = torch.nn.Conv2d(16, 128, 3, stride=2, padding=1)
    with torch.no_grad():
        conv.weight[5, 1, 2, 0] = bad
    assert pack_conv_weights_split(conv) is None


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_emulation_predicts_the_exact_cases_bit_for_bit(geometry):
    """(i) - (iii) of the GPU file on every geometry: no rounded sum anywhere, so the emulated kernel arithmetic gives the float64 result."""
    k, stride, pad = geometry
    for build in (case_single_tap, case_power_of_two_activations, case_mid_mid):
        x, w, ref = build(k, stride, pad)
        got = emulate_conv(x, w, k, stride, pad)
        assert torch.equal(got, ref), (build.__name__, (got - ref).abs().max().item())


def test_emulation_predicts_the_integer_case_bit_for_bit():
    x, w, ref = case_integers()
    assert ref.abs().max() > 2 ** 20  # the sums are not small: taps, slices and padding all contribute
    assert torch.equal(emulate_conv(x, w, 3, 2, 1), ref)

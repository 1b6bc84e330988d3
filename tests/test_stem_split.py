"""The exact three-part bf16 split behind the uint8 stem on the bf16 matrix cores (``split_stem_weights``), on the host.

Premises checked here: a float32 weight is ``hi + mid + lo`` with three bf16 numbers (or is reported as not splittable), every
product ``byte * part`` is exact in float32, and the new order of operations (integer bytes, sum, ``/ 255``, ``+ bias``) stays
within the project's gate for "float32 summation order only" of the unfused torch ops.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from tiatoolbox_amd.models.architecture.fused import split_stem_weights


def _bf16_round_np(x: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even float32 -> bf16 (as float32), restated on the bit patterns (finite inputs)."""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _split_np(w: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    w = w.astype(np.float32)
    hi = _bf16_round_np(w)
    r1 = w - hi
    mid = _bf16_round_np(r1)
    lo = _bf16_round_np(r1 - mid)
    return hi, mid, lo


def _is_bf16(parts: torch.Tensor) -> bool:
    return bool(((parts.contiguous().view(torch.int32) & 0xFFFF) == 0).all())


def test_split_is_exact_for_every_mantissa_and_sign_at_one_exponent():
    """All 2^24 sign x mantissa patterns at the biased exponent 120 (|w| in [2^-7, 2^-6): the magnitude of trained stem weights)."""
    mant = torch.arange(1 << 23, dtype=torch.int32)
    for sign in (0, 1):
        bits = mant | (120 << 23) | (-(1 << 31) if sign else 0)
        w = bits.view(torch.float32)
        parts, usable = split_stem_weights(w)
        assert usable
        assert _is_bf16(parts)
        assert torch.equal(parts.double().sum(0), w.double())
        # the restatement agrees part by part (a 2^20 subset that contains every value of the low 16 bits)
        sub = slice(0, 1 << 20)
        hi, mid, lo = _split_np(w[sub].numpy())
        assert np.array_equal(parts[0, sub].numpy(), hi) and np.array_equal(parts[1, sub].numpy(), mid)
        assert np.array_equal(parts[2, sub].numpy(), lo)


def test_split_of_the_test_weights_and_special_values():
    from test_stem_gpu import _stem_parts

    for seed in (0, 3, 224224, 256256):
        w = _stem_parts(seed).weight.detach()
        parts, usable = split_stem_weights(w)
        assert usable and _is_bf16(parts) and parts.shape == (3, 64, 3, 7, 7)
        assert torch.equal(parts.double().sum(0), w.double())
        hi, mid, lo = _split_np(w.numpy())
        assert np.array_equal(parts[0].numpy(), hi) and np.array_equal(parts[1].numpy(), mid) and np.array_equal(parts[2].numpy(), lo)
    special = torch.tensor([0.0, -0.0, 1.0, -2.0, 2.0 ** -20, 2.0 ** 20, 2.0 ** -100, 1.0 - 2.0 ** -24, 2.0 - 2.0 ** -23, -(1.0 - 2.0 ** -24),
                            400.0, -399.0, 1.0 / 3.0], dtype=torch.float32)
    parts, usable = split_stem_weights(special)
    assert usable and _is_bf16(parts) and torch.equal(parts.double().sum(0), special.double())
    assert torch.equal(parts[:, 0], torch.zeros(3))  # zero splits into zeros


@pytest.mark.parametrize("bad", [3.4e38, -3.4e38, 1e-36, 1e-40, float("inf"), float("-inf"), float("nan")])
def test_values_without_a_usable_split_are_reported(bad):
    """Next to overflow ``bf16(w)`` is infinite; at 1e-36 the middle part is subnormal; 1e-40 is subnormal itself."""
    w = torch.full((64, 3, 7, 7), 0.01, dtype=torch.float32)
    assert split_stem_weights(w)[1]
    w[5, 1, 2, 3] = bad
    assert not split_stem_weights(w)[1]


def test_every_product_of_a_byte_and_a_part_is_exact_in_float32():
    from test_stem_gpu import _stem_parts

    parts, usable = split_stem_weights(_stem_parts(0).weight.detach())
    assert usable
    p = parts.reshape(-1)
    extra, _ = split_stem_weights(torch.tensor([1.0 - 2.0 ** -24, 2.0 - 2.0 ** -23, 1.0 / 3.0, -400.0], dtype=torch.float32))
    p = torch.cat([p, extra.reshape(-1)])
    bytes_ = torch.arange(256, dtype=torch.float32)
    prod32 = bytes_[:, None] * p[None, :]
    prod64 = bytes_.double()[:, None] * p.double()[None, :]
    assert torch.equal(prod32.double(), prod64)
    # ... and a bf16 number each factor: the matrix cores see exactly these operands
    assert _is_bf16(bytes_) and _is_bf16(p)


def _quotient_255(s: torch.Tensor) -> torch.Tensor:
    """The kernel's three instructions: ``q = s r; e = fma(-255, q, s); q' = fma(e, r, q)`` with ``r = fl(1 / 255)`` -- float32 fma
    emulated in float64 (each product of two float32 numbers is exact there; the sum is then rounded once to float64 and once to
    float32, which these magnitudes do not disturb: checked against the exact quotient below)."""
    r = torch.tensor(1.0, dtype=torch.float32) / 255
    q = s * r
    e = (s.double() - 255.0 * q.double()).float()
    return (e.double() * r.double() + q.double()).float()


def test_three_instruction_quotient_is_the_correctly_rounded_division():
    g = torch.Generator().manual_seed(1)
    s = torch.cat([torch.arange(256, dtype=torch.float32), torch.randn(20000, generator=g) * 300,
                   torch.randint(-(1 << 24), 1 << 24, (20000,), generator=g).float()])
    assert torch.equal(_quotient_255(s), s / 255)  # IEEE division on the CPU
    assert torch.equal(_quotient_255(torch.arange(256, dtype=torch.float32)), torch.arange(256).float().div(255))
    r = torch.tensor(1.0, dtype=torch.float32) / 255
    assert not torch.equal(s * r, s / 255)  # the bare product with the reciprocal is NOT


def _shapes():
    from test_stem_gpu import SHAPES

    return SHAPES


@pytest.mark.parametrize("shape", _shapes())
def test_float32_emulation_of_the_new_order_stays_within_the_summation_order_gate(shape):
    """Integer bytes, float32 sum, ``/ 255``, ``+ bias``, ReLU, pool against torch's unfused float32 ops on ``x / 255``: 1e-5, the
    gate of ``test_stem_gpu.py`` for "float32 summation order only" (measured: 1.0e-6)."""
    from test_stem_gpu import _reference, _stem_parts

    n, h, w = shape
    conv = _stem_parts(seed=h * 1000 + w)
    g = torch.Generator().manual_seed(n + h + w)
    x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    ref = _reference(conv, x.float().div(255))
    with torch.inference_mode():
        s = F.conv2d(x.float().permute(0, 3, 1, 2), conv.weight, None, 2, 3)
        got = F.max_pool2d(F.relu(_quotient_255(s) + conv.bias.view(1, -1, 1, 1)), 3, 2, 1)
    err = (got - ref).abs().max().item()
    print(f"shape {shape}: max |emulation - reference| = {err:.3e}")
    assert err <= 1e-5, err

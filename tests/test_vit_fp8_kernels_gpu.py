"""The kernels of ``vit_fp8.hip`` against float64 (``_vit_fp8_ref.py``): the FP8 GEMM bit for bit on exact integer data (the check of
the matrix instruction's operand lane maps) and to the half GEMM's gate on the whole e4m3 range, its refusals, the weight packing
against the recipe, and the three quantising producers."""

from __future__ import annotations

import functools

import pytest
import torch

from _vit_fp8_ref import (FINITE_CODES, HALF_EPS, check_quantised_rows, decode, e4m3_tie_rows, encode_exact, gelu64, gemm_ref64,
                          layernorm64, swiglu64)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
N_MIN = 16  # the smallest N tia_linear_fp8_rows takes (its N granularity)
KS, NS, ROWS = (128, 384, 1536), (N_MIN, 192, 1152), (1, 130, 394)
GUARD = 64  # sentinel rows behind the output


def _dt(dtype):
    from tiatoolbox_amd.models.architecture.fused import _DT

    return _DT[dtype]


def _run_gemm(a, sa, w, sw, bias, res, dtype):
    """The entry point itself on device copies; the output sits in front of ``GUARD`` sentinel rows, which must come back untouched."""
    from tiatoolbox_amd import _lib

    rows, k = a.shape
    n = w.shape[0]
    dev = [None if t is None else t.cuda().contiguous() for t in (a, sa, w, sw, bias, None if res is None else res.to(dtype))]
    buf = torch.full((rows + GUARD, n), 777.0, dtype=dtype, device="cuda")
    ptr = [0 if t is None else t.data_ptr() for t in dev]
    rc = _lib.load().tia_linear_fp8_rows(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4] or None, ptr[5] or None, buf.data_ptr(), rows, n, k,
                                         _dt(dtype), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((buf[rows:] == 777.0).all()), "a store beyond the last row"  # noqa: PLR2004
    return buf[:rows].cpu()


@functools.lru_cache(maxsize=None)
def _exact_case(k: int, n: int, rows: int):
    """Integer codes in [-8, 8] (exact in e4m3, asymmetric between the operands), power-of-two scales in {1/2, 1, 2}, integer bias and
    residual in [-8, 8]: |acc| <= 64 k < 2^17, so every partial sum, the scaled sum (2 fraction bits) and the additions are exact in
    float32 in any order, and the result is ``half_rne`` of the exact value."""
    g = torch.Generator().manual_seed(k * 7 + n * 3 + rows)
    a = encode_exact(torch.randint(-8, 9, (rows, k), generator=g).double())
    w = encode_exact(torch.randint(-8, 9, (n, k), generator=g).double())
    sa = torch.exp2(torch.randint(-1, 2, (rows,), generator=g).float())
    sw = torch.exp2(torch.randint(-1, 2, (n,), generator=g).float())
    bias = torch.randint(-8, 9, (n,), generator=g).float()
    res = torch.randint(-8, 9, (rows, n), generator=g).float()
    return a, sa, w, sw, bias, res


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "bias+residual"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_gemm_is_exact_on_integer_data(k, n, rows, extras, dtype):
    a, sa, w, sw, bias, res = _exact_case(k, n, rows)
    bias, res = (bias, res) if extras else (None, None)
    ref64 = gemm_ref64(a, sa, w, sw, bias, res)
    assert float(ref64.abs().max()) < 2.0 ** 22 and bool((ref64 * 4 == torch.round(ref64 * 4)).all())  # exact in float32
    want = ref64.float().to(dtype)  # half_rne of the exact value
    got = _run_gemm(a, sa, w, sw, bias, res, dtype)
    wrong = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"k={k} n={n} rows={rows} {dtype}: {wrong} of {got.numel()} elements differ")
    assert wrong == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize(("k", "n", "rows"), [(128, N_MIN, 1), (384, 192, 130), (1536, 1152, 394)])
def test_gemm_holds_the_half_gate_on_the_whole_code_range(k, n, rows, dtype):
    """Random codes over every finite e4m3 value (subnormals and +-448 included), random positive scales; per element
    ``HALF_EPS |ref| + 1e-4 max |ref|``, the gate ``tests/_conv_ref.py`` holds the half GEMM to."""
    g = torch.Generator().manual_seed(k + n + rows)
    a = FINITE_CODES[torch.randint(0, FINITE_CODES.numel(), (rows, k), generator=g)]
    w = FINITE_CODES[torch.randint(0, FINITE_CODES.numel(), (n, k), generator=g)]
    a[0, :4] = torch.tensor([0x7E, 0xFE, 0x01, 0x81], dtype=torch.uint8)  # +-448 and the smallest subnormals, in any draw
    w[0, :4] = torch.tensor([0x7E, 0x7E, 0x01, 0x07], dtype=torch.uint8)
    # scales that keep the fp16 output finite: |acc| <= 448^2 k
    sa = (torch.rand(rows, generator=g) + 0.5) * 2.0 ** -10
    sw = (torch.rand(n, generator=g) + 0.5) * 2.0 ** -10
    bias = torch.randn(n, generator=g)
    res = torch.randn((rows, n), generator=g).to(dtype)
    ref = gemm_ref64(a, sa, w, sw, bias, res)
    got = _run_gemm(a, sa, w, sw, bias, res, dtype).double()
    gate = HALF_EPS[dtype] * ref.abs() + 1e-4 * float(ref.abs().max())
    worst = float(((got - ref).abs() / gate).max())
    print(f"k={k} n={n} rows={rows} {dtype}: worst element {worst:.3f} of its gate, max |ref| {float(ref.abs().max()):.3e}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0


def test_gemm_refusals_launch_nothing():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    a = torch.zeros((4, 128), dtype=torch.uint8, device="cuda")
    w = torch.zeros((16, 128), dtype=torch.uint8, device="cuda")
    sa, sw = torch.ones(8, device="cuda"), torch.ones(16, device="cuda")
    y = torch.full((4, 16), 5.0, dtype=torch.bfloat16, device="cuda")
    bf, einval, esize = _dt(torch.bfloat16), -1, -3

    def call(ap=a.data_ptr(), sap=sa.data_ptr(), yp=y.data_ptr(), rows=4, n=16, k=128, dtype=bf):
        return lib.tia_linear_fp8_rows(ap, sap, w.data_ptr(), sw.data_ptr(), None, None, yp, rows, n, k, dtype, stream)

    assert call(k=96) == esize and call(n=24) == esize and call(k=0) == einval
    assert call(rows=0) == einval and call(rows=-1) == einval
    assert call(ap=a.data_ptr() + 1) == einval and call(sap=sa.data_ptr() + 4) == einval and call(yp=y.data_ptr() + 2) == einval
    assert call(ap=None) == einval and call(dtype=0) == einval
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())  # noqa: PLR2004
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())
    # the host-only query gives the same answers without a launch
    assert lib.tia_linear_fp8_serves(4, 16, 128) == 1 and lib.tia_linear_fp8_serves(4, 16, 96) == 0
    assert lib.tia_linear_fp8_serves(4, 24, 128) == 0 and lib.tia_linear_fp8_serves(0, 16, 128) == einval


@pytest.mark.parametrize(("n", "k"), [(16, 128), (200 * 16, 384), (1152, 3456)])
def test_pack_weights_is_the_recipe(n, k):
    """Codes and scales of ``tia_linear_fp8_pack_weights`` equal the torch statement of the recipe exactly (float32 in, one IEEE
    division each way, the same conversion): rows with a zero, an all-zero row, a row with a large outlier."""
    from tiatoolbox_amd.models.architecture.vit_fused import pack_linear_weights_fp8, quantize_rows_e4m3

    g = torch.Generator().manual_seed(n + k)
    w = torch.randn((n, k), generator=g) / k ** 0.5
    w[1] = 0.0
    w[2, 5] = 1e4
    w[3] = 0.37
    packed = pack_linear_weights_fp8(w.cuda())
    q, s = quantize_rows_e4m3(w)
    assert torch.equal(packed.scales.cpu(), s)
    assert torch.equal(packed.codes.cpu(), q.view(torch.uint8))


def test_pack_weights_rounds_every_tie_as_the_recipe():
    """Normal draws never land on a rounding tie.  ``e4m3_tie_rows``: the row maximum is exactly 448 (``inv = s = 1``), the other entries
    every midpoint between adjacent finite e4m3 magnitudes (the subnormal steps and the 2^-6 boundary included) with its two float32
    neighbours, in both signs -- the device's conversion must give the recipe's codes (ties to even) bit for bit."""
    from tiatoolbox_amd.models.architecture.vit_fused import pack_linear_weights_fp8, quantize_rows_e4m3

    w = e4m3_tie_rows(16)
    assert w.shape == (16, 768)
    packed = pack_linear_weights_fp8(w.cuda())
    q, s = quantize_rows_e4m3(w)
    assert bool((s == 1.0).all()) and torch.equal(packed.scales.cpu(), s)
    got, want = packed.codes.cpu(), q.view(torch.uint8)
    wrong = torch.nonzero(got != want)
    assert wrong.numel() == 0, (f"{wrong.shape[0]} codes differ from the recipe's; first (row, column) {wrong[0].tolist()}: value "
                                f"{float(w[tuple(wrong[0])])!r} -> code {int(got[tuple(wrong[0])]):#04x}, the recipe's {int(want[tuple(wrong[0])]):#04x}")


def _special_rows(x: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    """Rows 1 .. 3 (where there are that many): a constant row, a row with one outlier 1e4 x the rest, an all-negative row."""
    if x.shape[0] >= 5:  # noqa: PLR2004
        x[1] = 0.75
        x[2] = torch.randn(x.shape[1], generator=g) * 1e-2
        x[2, x.shape[1] // 3] = 100.0
        x[3] = -x[3].abs() - 0.5
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", [1, 5, 394])
@pytest.mark.parametrize("d", [128, 384, 1280, 1536])
def test_layernorm_q8(d, rows, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_layernorm_rows_q8

    g = torch.Generator().manual_seed(d + rows)
    x = _special_rows(torch.randn((rows, d), generator=g) * 2.0 + 0.5, g).to(dtype)
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.1
    out = hip_layernorm_rows_q8(x.cuda().reshape(1, rows, d), gamma.cuda(), beta.cuda(), eps=1e-6)
    torch.cuda.synchronize()
    check_quantised_rows(layernorm64(x, gamma, beta, 1e-6), out.codes, out.scales, f"layernorm d={d} rows={rows} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", [1, 5, 394])
@pytest.mark.parametrize("hidden", [512, 3072])
def test_gelu_q8(hidden, rows, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_q8

    g = torch.Generator().manual_seed(hidden + rows)
    x = _special_rows(torch.randn((rows, hidden), generator=g) * 2.0, g).to(dtype)
    before = x.clone()
    xd = x.cuda().reshape(1, rows, hidden)
    out = hip_act_rows_q8(xd, swiglu=False)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu().reshape(rows, hidden), before)  # not in place
    check_quantised_rows(gelu64(x), out.codes, out.scales, f"gelu hidden={hidden} rows={rows} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", [1, 5, 394])
@pytest.mark.parametrize(("half", "real"), [(512, 512), (3456, 3416)])
def test_swiglu_q8(half, real, rows, dtype):
    """``real < half``: the lanes a padded ``fc1`` writes exact zeros to (gate and value) must come out as zero codes."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_q8

    g = torch.Generator().manual_seed(half + rows)
    gate = _special_rows(torch.randn((rows, half), generator=g) * 3.0, g)
    value = _special_rows(torch.randn((rows, half), generator=g) * 2.0, g)
    if rows >= 5:  # noqa: PLR2004
        gate[4] = -30.0 - torch.rand(half, generator=g) * 60.0  # exp(-|t|) down to 1e-39: tiny products, no inf / inf
    gate[:, real:], value[:, real:] = 0.0, 0.0
    x = torch.cat([gate, value], dim=1).to(dtype)
    out = hip_act_rows_q8(x.cuda().reshape(1, rows, 2 * half), swiglu=True)
    torch.cuda.synchronize()
    assert tuple(out.codes.shape) == (1, rows, half)
    assert bool((out.codes.cpu().reshape(rows, half)[:, real:] == 0).all())  # pad lanes: exactly code 0
    check_quantised_rows(swiglu64(x), out.codes, out.scales, f"swiglu half={half} rows={rows} {dtype}")


def test_producers_refuse_what_they_do_not_take():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    x = torch.zeros((2, 64), dtype=torch.bfloat16, device="cuda")
    q = torch.full((2, 64), 9, dtype=torch.uint8, device="cuda")
    s, gb = torch.full((4,), 9.0, device="cuda"), torch.ones(64, device="cuda")
    bf, einval, esize = _dt(torch.bfloat16), -1, -3
    ln = lambda **kw: lib.tia_layernorm_rows_q8(kw.get("x", x.data_ptr()), kw.get("stride", 32), gb.data_ptr(), gb.data_ptr(), 1e-6,  # noqa: E731
                                                q.data_ptr(), s.data_ptr(), kw.get("rows", 2), kw.get("c", 32), kw.get("dtype", bf), stream)
    assert ln(c=24) == esize and ln(c=8208) == esize and ln(rows=0) == einval and ln(stride=16) == einval and ln(dtype=0) == einval
    assert ln(x=x.data_ptr() + 2) == einval
    for entry in (lib.tia_gelu_rows_q8, lib.tia_swiglu_rows_q8):
        assert entry(x.data_ptr(), q.data_ptr(), s.data_ptr(), 2, 24, bf, stream) == esize
        assert entry(x.data_ptr(), q.data_ptr(), s.data_ptr(), 0, 32, bf, stream) == einval
        assert entry(x.data_ptr(), q.data_ptr() + 8, s.data_ptr(), 2, 32, bf, stream) == einval
        assert entry(x.data_ptr(), q.data_ptr(), s.data_ptr(), 2, 32, 0, stream) == einval
    torch.cuda.synchronize()
    assert bool((q == 9).all()) and bool((s == 9.0).all())  # noqa: PLR2004
    assert ln() == 0 and decode(q.cpu()[:1, :32]).abs().max() == 448.0  # beta = 1 everywhere: the row is constant 1 -> code 0x7e  # noqa: PLR2004

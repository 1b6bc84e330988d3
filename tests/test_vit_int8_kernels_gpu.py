"""The kernels of ``vit_int8.hip`` against int64 / float64 (``_vit_int8_ref.py``): the INT8 GEMM bit for bit on arbitrary codes (the
accumulator is an exact int32: this is also the check of the matrix instruction's operand lane maps) and to the half GEMM's gate with
arbitrary scales, its refusals, the weight packing against the recipe, and the three quantising producers."""

from __future__ import annotations

import functools

import pytest
import torch

from _vit_int8_ref import HALF_EPS, acc64, check_quantised_rows, gelu64, gemm_ref32, gemm_ref64, layernorm64, swiglu64

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
KS, NS, ROWS = (128, 384, 1536), (16, 192, 1152), (1, 130, 394)
GUARD = 64  # sentinel rows behind the output


def _dt(dtype):
    from tiatoolbox_amd.models.architecture.fused import _DT

    return _DT[dtype]


def _run_gemm(a, sa, w, sw, bias, res, dtype):
    """The entry point itself on device copies; the output sits in front of ``GUARD`` sentinel rows, which must come back untouched."""
    from tiatoolbox_amd import _lib

    rows, k = a.shape
    n = w.shape[0]
    assert a.dtype == torch.int8 and w.dtype == torch.int8
    dev = [None if t is None else t.cuda().contiguous() for t in (a, sa, w, sw, bias, None if res is None else res.to(dtype))]
    buf = torch.full((rows + GUARD, n), 777.0, dtype=dtype, device="cuda")
    ptr = [0 if t is None else t.data_ptr() for t in dev]
    rc = _lib.load().tia_linear_int8_rows(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4] or None, ptr[5] or None, buf.data_ptr(), rows, n, k,
                                          _dt(dtype), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((buf[rows:] == 777.0).all()), "a store beyond the last row"  # noqa: PLR2004
    return buf[:rows].cpu()


def _differing(got: torch.Tensor, want: torch.Tensor) -> int:
    return int((got.view(torch.int16) != want.view(torch.int16)).sum())


@functools.lru_cache(maxsize=None)
def _exact_case(k: int, n: int, rows: int):
    """Random codes over all of -127 .. 127 (the two operands drawn apart: nothing is symmetric between them), power-of-two scales in
    {1/2, 1, 2} x 2^-6 on either side (they keep the fp16 output finite: |acc| <= 127^2 k), integer bias and residual in [-8, 8].
    The reference and its one assumption -- products with powers of two are exact -- are ``gemm_ref32``'s."""
    g = torch.Generator().manual_seed(k * 7 + n * 3 + rows)
    a = torch.randint(-127, 128, (rows, k), generator=g).to(torch.int8)
    w = torch.randint(-127, 128, (n, k), generator=g).to(torch.int8)
    sa = torch.exp2(torch.randint(-1, 2, (rows,), generator=g).float() - 6.0)
    sw = torch.exp2(torch.randint(-1, 2, (n,), generator=g).float() - 6.0)
    bias = torch.randint(-8, 9, (n,), generator=g).float()
    res = torch.randint(-8, 9, (rows, n), generator=g).float()
    return a, sa, w, sw, bias, res


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "bias+residual"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_gemm_is_exact_on_arbitrary_codes(k, n, rows, extras, dtype):
    a, sa, w, sw, bias, res = _exact_case(k, n, rows)
    bias, res = (bias, res) if extras else (None, None)
    want = gemm_ref32(a, sa, w, sw, bias, res).to(dtype)  # half_rne of the int64 accumulation through the contract's float32 steps
    assert bool(torch.isfinite(want).all()) and (a.numel() < 512 or (int(a.min()), int(a.max())) == (-127, 127))  # noqa: PLR2004
    got = _run_gemm(a, sa, w, sw, bias, res, dtype)
    wrong = _differing(got, want)
    print(f"k={k} n={n} rows={rows} {dtype}: {wrong} of {got.numel()} elements differ")
    assert wrong == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_gemm_rounds_an_odd_accumulator_above_2_to_24_to_even(dtype):
    """All-+-127 rows at K = 1536 with one code changed: |acc| = 1536 * 127^2 - 127 (2 r + 1), odd and above 2^24, where float32
    steps by 2 -- ``float(acc)`` must be the round-to-nearest-even conversion.  Both tie directions occur: accumulators
    congruent to 1 and to 3 modulo 4, of both signs.  The scales 2^-12 keep the products exact and the fp16 output finite."""
    # (cases that tell round-to-nearest-even from truncation and from round-half-up are counted below: `seen`)
    k, n, rows = 1536, 16, 8
    a = torch.full((rows, k), 127, dtype=torch.int8)
    w = torch.full((n, k), 127, dtype=torch.int8)
    a[1::2] = -127
    for r in range(rows):
        a[r, 5 + r] = a[r, 5 + r] - (2 * r + 1) * (1 if a[r, 5 + r] > 0 else -1)  # |code| 126, 124, ... : the sum moves by 127 (2 r + 1)
    w[3, 700] = 126
    w[4, 701] = -127
    acc = acc64(a, w)
    assert bool((acc.abs() > 2 ** 24).all()) and int((acc % 2 != 0).sum()) > rows * n // 2  # noqa: PLR2004
    assert {int(v) for v in (acc[acc % 2 != 0] % 4).unique()} == {1, 3}
    assert not torch.equal(acc.to(torch.float32).double(), acc.double())  # the conversion does round here
    sa, sw = torch.full((rows,), 2.0 ** -12), torch.full((n,), 2.0 ** -12)
    # the half output shows 8 or 11 bits of a float32 value: a bias that cancels the leading part, -(acc[0, 0] / 2^24), leaves the
    # conversion's last bit in reach of bf16 / fp16 in row 0
    bias = -(acc[0, 0].double() * 2.0 ** -24).float().expand(n).contiguous()
    want = gemm_ref32(a, sa, w, sw, bias, None).to(dtype)
    got = _run_gemm(a, sa, w, sw, bias, None, dtype)
    wrong = _differing(got, want)
    # a truncating or round-half-up conversion moves float(acc) by 2 on some of these: visible after the cancellation in row 0
    up = (torch.ceil(acc.double() / 2) * 2).float() * 2.0 ** -24 + bias
    down = (torch.floor(acc.double() / 2) * 2).float() * 2.0 ** -24 + bias
    seen = int(((up.to(dtype) != down.to(dtype)) & (acc % 2 != 0)).sum())
    print(f"odd accumulators above 2^24, {dtype}: {wrong} of {got.numel()} elements differ; {seen} elements tell the two roundings apart")
    assert seen > 0 and wrong == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_gemm_keeps_rows_and_columns_apart(dtype):
    """Asymmetric operands: token ``r`` holds the code ``r + 1`` at ``k = r`` only, channel ``o`` the code ``-(o + 1)`` at every
    ``k <= o`` -- acc[r, o] = -(r + 1)(o + 1) for r <= o, else 0: an upper-triangular, non-symmetric matrix on a non-square shape, with
    scales and a bias that differ per row and per column.  A row <-> column swap, a transposed store or a K map that differs between
    the operands cannot produce it."""
    rows, n, k = 100, 48, 128
    a = torch.zeros((rows, k), dtype=torch.int8)
    w = torch.zeros((n, k), dtype=torch.int8)
    for r in range(rows):
        a[r, r] = r + 1
    for o in range(n):
        w[o, :o + 1] = -(o + 1)
    acc = acc64(a, w)
    tri = torch.tensor([[-(r + 1) * (o + 1) if r <= o else 0 for o in range(n)] for r in range(rows)])
    assert torch.equal(acc, tri) and not torch.equal(acc[:n], acc[:n].T)
    sa = torch.exp2(-(torch.arange(rows) % 5).float())
    sw = torch.exp2((torch.arange(n) % 3).float() - 4.0)
    bias = torch.arange(n).float() * 0.25
    want = gemm_ref32(a, sa, w, sw, bias, None).to(dtype)
    got = _run_gemm(a, sa, w, sw, bias, None, dtype)
    assert _differing(got, want) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize(("k", "n", "rows"), [(128, 16, 1), (384, 192, 130), (1536, 1152, 394)])
def test_gemm_holds_the_half_gate_with_arbitrary_scales(k, n, rows, dtype):
    """Random codes, random positive float32 scales (products and sums now round, and may be fused); per element
    ``HALF_EPS |ref| + 1e-4 max |ref|``, the gate ``tests/_conv_ref.py`` holds the half GEMM to."""
    g = torch.Generator().manual_seed(k + n + rows)
    a = torch.randint(-127, 128, (rows, k), generator=g).to(torch.int8)
    w = torch.randint(-127, 128, (n, k), generator=g).to(torch.int8)
    sa = (torch.rand(rows, generator=g) + 0.5) * 2.0 ** -7
    sw = (torch.rand(n, generator=g) + 0.5) * 2.0 ** -7
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
    a = torch.ones((4, 128), dtype=torch.int8, device="cuda")
    w = torch.ones((16, 128), dtype=torch.int8, device="cuda")
    sa, sw = torch.ones(8, device="cuda"), torch.ones(16, device="cuda")
    y = torch.full((4, 16), 5.0, dtype=torch.bfloat16, device="cuda")
    bf, einval, esize = _dt(torch.bfloat16), -1, -3

    def call(ap=a.data_ptr(), sap=sa.data_ptr(), wp=w.data_ptr(), swp=sw.data_ptr(), yp=y.data_ptr(), rows=4, n=16, k=128, dtype=bf,
             bias=None, res=None):
        return lib.tia_linear_int8_rows(ap, sap, wp, swp, bias, res, yp, rows, n, k, dtype, stream)

    assert call(k=96) == esize and call(n=24) == esize and call(k=65536 + 128) == esize and call(k=0) == einval
    assert call(rows=0) == einval and call(rows=-1) == einval
    assert call(ap=a.data_ptr() + 1) == einval and call(sap=sa.data_ptr() + 4) == einval and call(yp=y.data_ptr() + 2) == einval
    assert call(wp=w.data_ptr() + 8) == einval and call(bias=sw.data_ptr() + 4) == einval and call(res=y.data_ptr() + 2) == einval
    assert call(ap=None) == einval and call(sap=None) == einval and call(wp=None) == einval and call(swp=None) == einval
    assert call(yp=None) == einval and call(dtype=0) == einval and call(dtype=99) == einval
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())  # noqa: PLR2004
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((y == 128.0).all())  # noqa: PLR2004
    # the host-only query gives the same answers without a launch
    assert lib.tia_linear_int8_serves(4, 16, 128) == 1 and lib.tia_linear_int8_serves(4, 16, 96) == 0
    assert lib.tia_linear_int8_serves(4, 24, 128) == 0 and lib.tia_linear_int8_serves(0, 16, 128) == einval
    assert lib.tia_linear_int8_serves(4, 16, 65536) == 1 and lib.tia_linear_int8_serves(4, 16, 65536 + 128) == 0
    # the packing entry: the GEMM's limits, and nothing written on a refusal
    q = torch.full((16, 128), 9, dtype=torch.int8, device="cuda")
    s = torch.full((16,), 9.0, device="cuda")
    w32 = torch.ones((16, 128), device="cuda")
    pack = lambda **kw: lib.tia_linear_int8_pack_weights(kw.get("w", w32.data_ptr()), kw.get("n", 16), kw.get("k", 128),  # noqa: E731
                                                         kw.get("q", q.data_ptr()), s.data_ptr(), stream)
    assert pack(k=96) == esize and pack(n=24) == esize and pack(n=0) == einval and pack(w=None) == einval and pack(q=q.data_ptr() + 4) == einval
    torch.cuda.synchronize()
    assert bool((q == 9).all()) and bool((s == 9.0).all())  # noqa: PLR2004


@pytest.mark.parametrize(("n", "k"), [(16, 128), (200 * 16, 384), (1152, 3456)])
def test_pack_weights_is_the_recipe(n, k):
    """Codes and scales of ``tia_linear_int8_pack_weights`` equal the torch statement of the recipe exactly (float32 in, one IEEE
    division each way, the same rounding): an all-zero row, a row with a large outlier, a constant row, a row of rounding ties."""
    from tiatoolbox_amd.models.architecture.vit_fused import pack_linear_weights_int8, quantize_rows_int8

    g = torch.Generator().manual_seed(n + k)
    w = torch.randn((n, k), generator=g) / k ** 0.5
    w[1] = 0.0
    w[2, 5] = 1e4
    w[3] = 0.37
    w[4] = (torch.arange(k) % 254 - 127).float() * 0.5  # halves with the maximum 63.5 -> ... and, scaled by 2, every tie k + 0.5
    w[4, 0], w[4, 1] = 127.0, -127.0  # inv = s = 1: the codes are rne of the values themselves
    w[5] = -w[5].abs() - 0.01
    packed = pack_linear_weights_int8(w.cuda())
    q, s = quantize_rows_int8(w)
    assert packed.codes.dtype == torch.int8 and float(s[4]) == 1.0
    assert torch.equal(packed.scales.cpu(), s)
    wrong = torch.nonzero(packed.codes.cpu() != q)
    assert wrong.numel() == 0, (wrong.shape[0], wrong[0].tolist())
    assert int(packed.codes.min()) == -127  # noqa: PLR2004


def _special_rows(x: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    """Rows 0 .. 2 of three or more: a constant row, a row with one outlier 1e4 x the rest, an all-negative row; random rows after."""
    if x.shape[0] >= 3:  # noqa: PLR2004
        x[0] = 0.75
        x[1] = torch.randn(x.shape[1], generator=g) * 1e-2
        x[1, x.shape[1] // 3] = 100.0
        x[2] = -x[2].abs() - 0.5
    return x


CS, PROD_ROWS = (128, 384, 1024, 1536), (1, 3, 394)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", PROD_ROWS)
@pytest.mark.parametrize("d", CS)
def test_layernorm_qi8(d, rows, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_layernorm_rows_qi8

    g = torch.Generator().manual_seed(d + rows)
    x = _special_rows(torch.randn((rows, d), generator=g) * 2.0 + 0.5, g).to(dtype)
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.1
    out = hip_layernorm_rows_qi8(x.cuda().reshape(1, rows, d), gamma.cuda(), beta.cuda(), eps=1e-6)
    torch.cuda.synchronize()
    assert out.codes.dtype == torch.int8 and tuple(out.codes.shape) == (1, rows, d)
    check_quantised_rows(layernorm64(x, gamma, beta, 1e-6), out.codes, out.scales, f"layernorm d={d} rows={rows} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", PROD_ROWS)
@pytest.mark.parametrize("hidden", CS)
def test_gelu_qi8(hidden, rows, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_qi8

    g = torch.Generator().manual_seed(hidden + rows)
    x = _special_rows(torch.randn((rows, hidden), generator=g) * 2.0, g).to(dtype)
    before = x.clone()
    xd = x.cuda().reshape(1, rows, hidden)
    out = hip_act_rows_qi8(xd, swiglu=False)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu().reshape(rows, hidden), before)  # not in place
    check_quantised_rows(gelu64(x), out.codes, out.scales, f"gelu hidden={hidden} rows={rows} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", PROD_ROWS)
@pytest.mark.parametrize(("half", "real"), [(128, 128), (384, 360), (1024, 1024), (1536, 1448)])
def test_swiglu_qi8(half, real, rows, dtype):
    """``real < half``: the lanes a padded ``fc1`` writes exact zeros to (gate and value) must come out as zero codes."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_qi8

    g = torch.Generator().manual_seed(half + rows)
    gate = _special_rows(torch.randn((rows, half), generator=g) * 3.0, g)
    value = _special_rows(torch.randn((rows, half), generator=g) * 2.0, g)
    if rows >= 5:  # noqa: PLR2004
        gate[4] = -30.0 - torch.rand(half, generator=g) * 60.0  # exp(-|t|) down to 1e-39: tiny products, no inf / inf
    gate[:, real:], value[:, real:] = 0.0, 0.0
    x = torch.cat([gate, value], dim=1).to(dtype)
    out = hip_act_rows_qi8(x.cuda().reshape(1, rows, 2 * half), swiglu=True)
    torch.cuda.synchronize()
    assert tuple(out.codes.shape) == (1, rows, half)
    assert not bool(out.codes.cpu().reshape(rows, half)[:, real:].any())  # pad lanes: exactly code 0
    check_quantised_rows(swiglu64(x), out.codes, out.scales, f"swiglu half={half} rows={rows} {dtype}")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("producer", ["layernorm", "gelu", "swiglu"])
def test_a_non_finite_row_gets_a_non_finite_scale_and_leaves_its_neighbours(producer, bad):
    """Rows 1 and 6 of 9 (two workgroups of four rows) hold one non-finite value: their scale is non-finite, their codes stay inside
    [-127, 127], and every other row's codes and scale are bit-identical to a run without them.  Through the GEMM every output of
    those tokens is non-finite and the other tokens' outputs are bit-identical as well."""
    from tiatoolbox_amd.models.architecture.vit_fused import (QuantRows, hip_act_rows_qi8, hip_layernorm_rows_qi8, hip_linear_int8_rows,
                                                              pack_linear_weights_int8)

    g = torch.Generator().manual_seed(11)
    rows, c = 9, 384
    width = 2 * c if producer == "swiglu" else c
    clean = torch.randn((1, rows, width), generator=g).to(torch.bfloat16)
    dirty = clean.clone()
    dirty[0, 1, 7], dirty[0, 6, width - 3] = bad, bad
    gamma, beta = (torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.1).cuda()

    def run(x):
        if producer == "layernorm":
            return hip_layernorm_rows_qi8(x.cuda(), gamma, beta, eps=1e-6)
        return hip_act_rows_qi8(x.cuda(), swiglu=producer == "swiglu")

    want, got = run(clean), run(dirty)
    torch.cuda.synchronize()
    keep = [0, 2, 3, 4, 5, 7, 8]
    assert not bool(torch.isfinite(got.scales[[1, 6]]).any()) and bool(torch.isfinite(got.scales[keep]).all())
    assert int(got.codes.min()) >= -127  # noqa: PLR2004
    assert torch.equal(got.codes[0, keep], want.codes[0, keep]) and torch.equal(got.scales[keep], want.scales[keep])
    w = pack_linear_weights_int8(torch.randn((32, c), generator=g).cuda())
    bias = torch.randn(32, generator=g).cuda()
    y_want = hip_linear_int8_rows(QuantRows(want.codes, want.scales), w, bias, dtype=torch.bfloat16)
    y_got = hip_linear_int8_rows(QuantRows(got.codes, got.scales), w, bias, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(y_got[0, [1, 6]]).any())  # never a finite wrong value
    assert torch.equal(y_got[0, keep], y_want[0, keep]) and bool(torch.isfinite(y_want).all())


def test_producers_refuse_what_they_do_not_take():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    x = torch.zeros((2, 64), dtype=torch.bfloat16, device="cuda")
    q = torch.full((2, 64), 9, dtype=torch.int8, device="cuda")
    s, gb = torch.full((4,), 9.0, device="cuda"), torch.ones(64, device="cuda")
    bf, einval, esize = _dt(torch.bfloat16), -1, -3
    ln = lambda **kw: lib.tia_layernorm_rows_qi8(kw.get("x", x.data_ptr()), kw.get("stride", 32), gb.data_ptr(), gb.data_ptr(), 1e-6,  # noqa: E731
                                                 q.data_ptr(), s.data_ptr(), kw.get("rows", 2), kw.get("c", 32), kw.get("dtype", bf), stream)
    assert ln(c=24) == esize and ln(c=8208) == esize and ln(rows=0) == einval and ln(stride=16) == einval and ln(dtype=0) == einval
    assert ln(x=x.data_ptr() + 2) == einval and ln(x=None) == einval
    for entry in (lib.tia_gelu_rows_qi8, lib.tia_swiglu_rows_qi8):
        assert entry(x.data_ptr(), q.data_ptr(), s.data_ptr(), 2, 24, bf, stream) == esize
        assert entry(x.data_ptr(), q.data_ptr(), s.data_ptr(), 2, 8208, bf, stream) == esize
        assert entry(x.data_ptr(), q.data_ptr(), s.data_ptr(), 0, 32, bf, stream) == einval
        assert entry(x.data_ptr(), q.data_ptr() + 8, s.data_ptr(), 2, 32, bf, stream) == einval
        assert entry(x.data_ptr(), q.data_ptr(), s.data_ptr(), 2, 32, 0, stream) == einval
        assert entry(None, q.data_ptr(), s.data_ptr(), 2, 32, bf, stream) == einval
    torch.cuda.synchronize()
    assert bool((q == 9).all()) and bool((s == 9.0).all())  # noqa: PLR2004
    assert ln() == 0  # beta = 1 everywhere: the rows are the constant 1 -> code 127, scale 1 / 127
    torch.cuda.synchronize()
    flat = q.reshape(-1)  # two rows of c = 32 codes, back to back
    assert bool((flat[:64] == 127).all()) and bool((flat[64:] == 9).all()) and bool((s[:2] == 1.0 / 127.0).all())  # noqa: PLR2004
    assert bool((s[2:] == 9.0).all())  # noqa: PLR2004

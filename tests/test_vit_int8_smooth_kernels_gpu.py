"""The kernels ``int8_smoothing`` adds to ``vit_int8.hip`` against float64 (``_vit_int8_ref.py``, ``_vit_int8_smooth_ref.py``): the smoothed
GELU / SwiGLU producers -- byte for byte the unsmoothed ones under all-ones scales, inside the quantisation bound under random powers
of two, the contract of the hard rows kept -- the calibration statistics, and what the five entries refuse.

Rows 1, 3, 5 and 130: four rows per workgroup, so partial workgroups and more than one; hidden 128 .. 8192: every vectors-per-lane form
of the row-in-registers kernels (1, 2, 4, 8, 16) and a partly filled wave (528 = 66 vectors)."""

from __future__ import annotations

import functools

import pytest
import torch

from _vit_int8_ref import SCALE_ULPS, check_quantised_rows, gelu64, layernorm64, swiglu64
from _vit_int8_smooth_ref import absmax64

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
ROWS, HIDDEN = (1, 3, 5, 130), (128, 528, 1024, 3456, 8192)
SWIGLU_REAL = {3456: 3416}  # Virchow's padded half: the lanes beyond 3416 are exact zeros of a padded fc1


def _dt(dtype):
    from tiatoolbox_amd.models.architecture.fused import _DT

    return _DT[dtype]


@functools.lru_cache(maxsize=None)
def _act_input(rows: int, hidden: int, swiglu: bool, dtype: torch.dtype) -> torch.Tensor:
    """``[1, rows, hidden]`` (GELU) or ``[1, rows, 2 hidden]`` (SwiGLU, pad lanes zero) on the CPU; of three or more rows, row 0 is
    constant, row 1 has one outlier 1e4 x the rest and row 2 gives an all-negative activation row."""
    g = torch.Generator().manual_seed(rows * 31 + hidden + swiglu)
    x = torch.randn((rows, hidden), generator=g) * 2.0
    if rows >= 3:  # noqa: PLR2004
        x[0] = 0.75
        x[1] = torch.randn(hidden, generator=g) * 1e-2
        x[1, hidden // 3] = 100.0
        x[2] = -x[2].abs() * 0.2 - 0.1  # GELU of a small negative value is negative; as a SwiGLU gate, silu is negative too
    if swiglu:
        value = torch.randn((rows, hidden), generator=g).abs() + 0.25
        real = SWIGLU_REAL.get(hidden, hidden)
        x[:, real:], value[:, real:] = 0.0, 0.0
        x = torch.cat([x, value], dim=1)
    return x.to(dtype).reshape(1, rows, -1)


def _pow2(hidden: int, seed: int) -> torch.Tensor:
    return torch.exp2(torch.randint(-6, 7, (hidden,), generator=torch.Generator().manual_seed(seed)).float())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("swiglu", [False, True], ids=["gelu", "swiglu"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("hidden", HIDDEN)
def test_smoothed_producers(hidden, rows, swiglu, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_qi8, hip_act_rows_qi8_smooth

    x = _act_input(rows, hidden, swiglu, dtype)
    xd = x.cuda()
    plain = hip_act_rows_qi8(xd, swiglu=swiglu)
    ones = hip_act_rows_qi8_smooth(xd, torch.ones(hidden, device="cuda"), swiglu=swiglu)
    inv = _pow2(hidden, hidden + rows)
    out = hip_act_rows_qi8_smooth(xd, inv.cuda(), swiglu=swiglu)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x)  # not in place
    assert ones.codes.dtype == torch.int8 and tuple(ones.codes.shape) == (1, rows, hidden)
    assert torch.equal(ones.codes, plain.codes) and torch.equal(ones.scales.view(torch.int32), plain.scales.view(torch.int32))
    act = (swiglu64 if swiglu else gelu64)(x.reshape(rows, -1))
    check_quantised_rows(act * inv.double(), out.codes, out.scales, f"{'swiglu' if swiglu else 'gelu'} smooth hidden={hidden} rows={rows} {dtype}")
    if swiglu and hidden in SWIGLU_REAL:
        assert not bool(out.codes.cpu().reshape(rows, hidden)[:, SWIGLU_REAL[hidden]:].any())  # pad lanes: exactly code 0
    if rows >= 3:  # noqa: PLR2004
        q = out.codes.cpu().reshape(rows, hidden)
        assert int(q.abs().amax(dim=1).min()) == 127 and int(q.min()) >= -127  # every row reaches +-127, never -128  # noqa: PLR2004
        if not swiglu:
            assert int(q[2].max()) <= 0  # the all-negative row


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("swiglu", [False, True], ids=["gelu", "swiglu"])
def test_a_non_finite_row_keeps_its_contract_under_smoothing(swiglu, bad):
    """Rows 1 and 6 of 9 hold one non-finite value: their scale is non-finite, their codes stay inside [-127, 127], and every other
    row is bit-identical to a run without them -- the unsmoothed producers' contract."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_qi8_smooth

    g = torch.Generator().manual_seed(11)
    rows, c = 9, 384
    width = 2 * c if swiglu else c
    clean = torch.randn((1, rows, width), generator=g).to(torch.bfloat16)
    dirty = clean.clone()
    dirty[0, 1, 7], dirty[0, 6, width - 3] = bad, bad
    inv = _pow2(c, 5).cuda()
    want, got = hip_act_rows_qi8_smooth(clean.cuda(), inv, swiglu=swiglu), hip_act_rows_qi8_smooth(dirty.cuda(), inv, swiglu=swiglu)
    torch.cuda.synchronize()
    keep = [0, 2, 3, 4, 5, 7, 8]
    assert not bool(torch.isfinite(got.scales[[1, 6]]).any()) and bool(torch.isfinite(got.scales[keep]).all())
    assert int(got.codes.min()) >= -127  # noqa: PLR2004
    assert torch.equal(got.codes[0, keep], want.codes[0, keep]) and torch.equal(got.scales[keep], want.scales[keep])


def _ulps(got: torch.Tensor, want64: torch.Tensor) -> float:
    """The largest distance of a float32 column maximum from the float64 one, in float32 ulp of the latter (zero columns: exact)."""
    live = want64 > 0
    assert bool((got.double()[~live] == 0).all())
    ulp = torch.exp2(torch.floor(torch.log2(want64[live])) - 23.0)
    return float(((got.double()[live] - want64[live]).abs() / ulp).max()) if bool(live.any()) else 0.0


# The statistics are compared with float64 to SCALE_ULPS float32 ulp OF THE COLUMN MAXIMUM, the row-scale tests' tolerance.  A row maximum
# is always attained where the producers' float32 formulas are well conditioned; a column maximum over few rows need not be: the
# kernels' GELU, 0.5 x (1 + erf(x / sqrt 2)), rounds 1 + erf to 2^-24, a relative error of 2^-24 / (1 + erf) that passes 4 ulp below
# x ~ -1.2, and a LayerNorm output gamma a + beta near zero carries the absolute error of its two terms.  No float32 evaluation of the
# stated arithmetic meets an ulp bound there, so the inputs keep every column's maximum at a well-conditioned value: row 0 of each
# batch is built for that (GELU: 1 + |N| or -0.75, GELU's own minimum, which no other negative input exceeds in magnitude;
# LayerNorm: +-(1 + U) about a zero mean, small beta), and every further row is plain Gaussian data, ill-conditioned entries
# included -- they must not win.  SwiGLU's silu(t) v has no cancellation and takes Gaussian data throughout.
def _gelu_stat_input(rows: int, hidden: int, dtype: torch.dtype, seed: int, scale: float = 1.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, hidden), generator=g) * 2.0
    coin = torch.rand(hidden, generator=g) < 0.5  # noqa: PLR2004
    x[0] = torch.where(coin, (1.0 + torch.randn(hidden, generator=g).abs()) * scale, torch.full((hidden,), -0.75))
    return x.to(dtype).reshape(1, rows, hidden)


def _layernorm_stat_input(rows: int, d: int, dtype: torch.dtype, seed: int, scale: float = 2.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, d), generator=g) * 2.0 + 0.5
    sign = torch.where(torch.arange(d) % 2 == 0, 1.0, -1.0)[torch.randperm(d, generator=g)]  # as many +1 as -1: a mean near zero
    x[0] = sign * (1.0 + torch.rand(d, generator=g)) * scale
    return x.to(dtype).reshape(1, rows, d)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("swiglu", [False, True], ids=["gelu", "swiglu"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("hidden", HIDDEN)
def test_act_absmax(hidden, rows, swiglu, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_absmax_h

    act = swiglu64 if swiglu else gelu64
    x = _act_input(rows, hidden, swiglu, dtype) if swiglu else _gelu_stat_input(rows, hidden, dtype, hidden + rows)
    amax = torch.zeros(hidden, device="cuda")
    assert hip_act_rows_absmax_h(x.cuda(), amax, swiglu=swiglu) is amax
    torch.cuda.synchronize()
    first = amax.cpu().clone()
    want = absmax64(act(x.reshape(rows, -1)))
    off = _ulps(first, want)
    print(f"{'swiglu' if swiglu else 'gelu'} absmax hidden={hidden} rows={rows} {dtype}: off by {off:.2f} float32 ulp")
    assert off <= SCALE_ULPS
    if not swiglu:  # magnitudes of negative values are in the statistic: the columns whose maximum is |GELU(-0.75)|
        assert rows > 1 or int(((first > 0.169) & (first < 0.171)).sum()) > hidden // 4  # noqa: PLR2004
    # a second call accumulates: the maximum with another batch -- larger in some columns, smaller in others -- and nothing is lost
    if swiglu:
        y = (x.float() * 0.5).to(dtype)
        y[0, :, 0:hidden:2] = x[0, :, 0:hidden:2] * 3.0  # every other gate three times as large, everything else halved
    else:
        y = _gelu_stat_input(rows, hidden, dtype, hidden + rows + 1, scale=1.5)
    hip_act_rows_absmax_h(y.cuda(), amax, swiglu=swiglu)
    torch.cuda.synchronize()
    second = absmax64(act(y.reshape(rows, -1)))
    assert bool((second > want).any()) and bool((second < want).any())
    assert _ulps(amax.cpu(), torch.maximum(want, second)) <= SCALE_ULPS and bool((amax.cpu() >= first).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", HIDDEN)
def test_layernorm_absmax(d, rows, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_layernorm_rows_absmax_h

    g = torch.Generator().manual_seed(d + rows)
    x = _layernorm_stat_input(rows, d, dtype, d + rows)
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.02
    gamma[d // 5], beta[d // 5] = gamma[d // 5] * 60.0, beta[d // 5] * 60.0
    amax = torch.zeros(d, device="cuda")
    hip_layernorm_rows_absmax_h(x.cuda(), gamma.cuda(), beta.cuda(), amax, eps=1e-6)
    torch.cuda.synchronize()
    want = absmax64(layernorm64(x.reshape(rows, d), gamma, beta, 1e-6))
    off = _ulps(amax.cpu(), want)
    print(f"layernorm absmax d={d} rows={rows} {dtype}: off by {off:.2f} float32 ulp")
    assert off <= SCALE_ULPS
    x2 = _layernorm_stat_input(rows, d, dtype, d + rows + 1, scale=3.0)
    hip_layernorm_rows_absmax_h(x2.cuda(), gamma.cuda(), beta.cuda(), amax, eps=1e-6)
    torch.cuda.synchronize()
    second = absmax64(layernorm64(x2.reshape(rows, d), gamma, beta, 1e-6))
    assert bool((second > want).any()) and bool((second < want).any())
    assert _ulps(amax.cpu(), torch.maximum(want, second)) <= SCALE_ULPS


@pytest.mark.parametrize("producer", ["layernorm", "gelu", "swiglu"])
def test_a_nan_stays_in_its_column_only(producer):
    """130 rows in more than one workgroup: a NaN activation in column 9 (GELU / SwiGLU) makes that column's statistic NaN and leaves
    every other column what it is without it, also after a further clean call.  A NaN input of the LayerNorm makes its whole row NaN,
    so every column is NaN: the same rule."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_absmax_h, hip_layernorm_rows_absmax_h

    g = torch.Generator().manual_seed(2)
    rows, c = 130, 528
    width = 2 * c if producer == "swiglu" else c
    clean = torch.randn((1, rows, width), generator=g).to(torch.bfloat16)
    dirty = clean.clone()
    dirty[0, 77, 9] = float("nan")
    gamma, beta = (torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.1).cuda()

    def run(x, amax):
        if producer == "layernorm":
            return hip_layernorm_rows_absmax_h(x.cuda(), gamma, beta, amax, eps=1e-6)
        return hip_act_rows_absmax_h(x.cuda(), amax, swiglu=producer == "swiglu")

    want, got = run(clean, torch.zeros(c, device="cuda")), torch.zeros(c, device="cuda")
    run(dirty, got)
    run(clean, got)
    torch.cuda.synchronize()
    if producer == "layernorm":
        assert bool(torch.isnan(got).all())
        return
    others = [j for j in range(c) if j != 9]  # noqa: PLR2004
    assert bool(torch.isnan(got[9])) and torch.equal(got[others], want[others]) and bool(torch.isfinite(want).all())


def test_the_new_entries_refuse_what_they_do_not_take():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    x = torch.zeros((2, 64), dtype=torch.bfloat16, device="cuda")
    q = torch.full((2, 64), 9, dtype=torch.int8, device="cuda")
    s, ones = torch.full((4,), 9.0, device="cuda"), torch.ones(64, device="cuda")
    amax = torch.full((64,), 9.0, device="cuda")
    bf, einval, esize = _dt(torch.bfloat16), -1, -3
    for entry in (lib.tia_gelu_rows_qi8_smooth, lib.tia_swiglu_rows_qi8_smooth):
        call = lambda entry=entry, **kw: entry(kw.get("x", x.data_ptr()), kw.get("inv", ones.data_ptr()), kw.get("q", q.data_ptr()), s.data_ptr(),  # noqa: E731
                                               kw.get("rows", 2), kw.get("hidden", 32), kw.get("dtype", bf), stream)
        assert call(hidden=24) == esize and call(hidden=8208) == esize and call(rows=0) == einval and call(hidden=0) == einval
        assert call(q=q.data_ptr() + 8) == einval and call(inv=ones.data_ptr() + 4) == einval and call(x=x.data_ptr() + 2) == einval
        assert call(dtype=0) == einval and call(dtype=99) == einval and call(x=None) == einval and call(inv=None) == einval and call(q=None) == einval
    for entry in (lib.tia_gelu_rows_absmax_h, lib.tia_swiglu_rows_absmax_h):
        call = lambda entry=entry, **kw: entry(kw.get("x", x.data_ptr()), kw.get("amax", amax.data_ptr()), kw.get("rows", 2), kw.get("hidden", 32),  # noqa: E731
                                               kw.get("dtype", bf), stream)
        assert call(hidden=24) == esize and call(hidden=8208) == esize and call(rows=0) == einval and call(dtype=0) == einval
        assert call(amax=amax.data_ptr() + 4) == einval and call(x=x.data_ptr() + 2) == einval and call(x=None) == einval and call(amax=None) == einval
    ln = lambda **kw: lib.tia_layernorm_rows_absmax_h(kw.get("x", x.data_ptr()), kw.get("stride", 32), ones.data_ptr(), ones.data_ptr(), 1e-6,  # noqa: E731
                                                      kw.get("amax", amax.data_ptr()), kw.get("rows", 2), kw.get("c", 32), kw.get("dtype", bf), stream)
    assert ln(c=24) == esize and ln(c=8208) == esize and ln(rows=0) == einval and ln(stride=16) == einval and ln(dtype=0) == einval
    assert ln(x=x.data_ptr() + 2) == einval and ln(x=None) == einval and ln(amax=None) == einval and ln(amax=amax.data_ptr() + 8) == einval
    torch.cuda.synchronize()
    assert bool((q == 9).all()) and bool((s == 9.0).all()) and bool((amax == 9.0).all())  # nothing was launched  # noqa: PLR2004
    # and the calls they do take: GELU(0) = 0 -> zero codes, scale 1; the LayerNorm of a zero row is beta = 1 -> |v| = 1 below the 9
    assert lib.tia_gelu_rows_qi8_smooth(x.data_ptr(), ones.data_ptr(), q.data_ptr(), s.data_ptr(), 2, 32, bf, stream) == 0
    assert ln() == 0
    torch.cuda.synchronize()
    flat = q.reshape(-1)
    assert not bool(flat[:64].any()) and bool((flat[64:] == 9).all()) and bool((s[:2] == 1.0).all()) and bool((s[2:] == 9.0).all())  # noqa: PLR2004
    assert bool((amax == 9.0).all())  # noqa: PLR2004
    amax.zero_()
    assert ln() == 0
    torch.cuda.synchronize()
    assert bool((amax[:32] == 1.0).all()) and not bool(amax[32:].any())


def test_the_wrappers_refuse_wrong_tensors():
    from tiatoolbox_amd.models.architecture.vit_fused import hip_act_rows_absmax_h, hip_act_rows_qi8_smooth, hip_layernorm_rows_absmax_h

    x = torch.zeros((1, 2, 128), dtype=torch.bfloat16, device="cuda")
    ones = torch.ones(128, device="cuda")
    for inv in (torch.ones(64, device="cuda"), torch.ones(128), torch.ones(128, device="cuda", dtype=torch.float64), torch.ones((1, 128), device="cuda")):
        with pytest.raises(ValueError, match="hip_act_rows_qi8_smooth takes inv_smooth as 128 contiguous float32"):
            hip_act_rows_qi8_smooth(x, inv, swiglu=False)
        with pytest.raises(ValueError, match="hip_act_rows_absmax_h takes amax as 128 contiguous float32"):
            hip_act_rows_absmax_h(x, inv, swiglu=False)
        with pytest.raises(ValueError, match="hip_layernorm_rows_absmax_h takes amax as 128 contiguous float32"):
            hip_layernorm_rows_absmax_h(x, ones, ones, inv, eps=1e-6)
    with pytest.raises(ValueError, match="hip_act_rows_qi8_smooth"):
        hip_act_rows_qi8_smooth(x.float(), ones, swiglu=False)
    with pytest.raises(ValueError, match=r"\[n, S, H\]"):
        hip_act_rows_qi8_smooth(x[0], ones, swiglu=False)
    with pytest.raises(ValueError, match="hip_act_rows_absmax_h"):
        hip_act_rows_absmax_h(x.cpu(), ones, swiglu=False)

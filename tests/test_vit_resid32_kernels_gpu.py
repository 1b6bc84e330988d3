"""The three kernels of ``residual_dtype="float32"`` (``csrc/vit_rows.hip``: ``tia_add_layernorm_rows_f32``,
``tia_vit_assemble_rows_f32``, ``tia_vit_cls_mean_pool_f32``) against references computed on the CPU from exactly the bits the kernels
are given: the float32 adds bit for bit, the LayerNorms in float64 under the gates of ``test_vit_kernels_gpu`` /
``test_vit_virchow_kernels_gpu``; what lies around the outputs stays untouched; the entry points' refusals."""

from __future__ import annotations

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
UNIT = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -22}  # one unit in the last place of an output
EPS = 1e-6
GUARD = 64  # elements of NaN in front of and behind every buffer a kernel writes (a multiple of 16 bytes in every type)


def _dt(dtype: torch.dtype) -> int:
    from tiatoolbox_amd.models.architecture.fused import _DT

    return _DT[dtype]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)  # noqa: PLR2004  (NaN guards compare as bits)


def _ln64(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    return (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + EPS) * gamma.double() + beta.double()


def _guarded(payload: torch.Tensor) -> torch.Tensor:
    """``payload`` (flat, CPU) between two NaN guards, on the device."""
    nan = torch.full((GUARD,), float("nan"), dtype=payload.dtype)
    return torch.cat([nan, payload.reshape(-1), nan]).cuda()


# ------------------------------------------------------------------------------------------------------------------------------------
# tia_add_layernorm_rows_f32
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_aln(x_buf, branch_buf, gamma, beta, y_dtype, *, rows, c, stride, dtype):
    """The entry point on the middle of guarded buffers.  ``x_buf`` / ``branch_buf`` ``[rows, stride]`` on the CPU (the last row is cut
    after its ``c`` values, so that the guard follows it at once); ``branch_buf`` / ``y_dtype`` ``None`` leave that part out.  Returns
    ``(x buffer after, with guards; y [rows, c] or None; whether y's guards are still NaN)``."""
    from tiatoolbox_amd import _lib

    used = (rows - 1) * stride + c
    xg = _guarded(x_buf.reshape(-1)[:used])
    bg = branch_buf.reshape(-1)[:used].cuda() if branch_buf is not None else None
    yg = torch.full((2 * GUARD + rows * c,), float("nan"), dtype=y_dtype, device="cuda") if y_dtype is not None else None
    g, b = gamma.cuda(), beta.cuda()
    rc = _lib.load().tia_add_layernorm_rows_f32(
        xg.data_ptr() + 4 * GUARD, stride, bg.data_ptr() if bg is not None else None, stride, g.data_ptr(), b.data_ptr(), EPS,
        yg.data_ptr() + GUARD * yg.element_size() if yg is not None else None, _dt(y_dtype or dtype), rows, c, _dt(dtype),
        _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    if yg is None:
        return xg.cpu(), None, True
    untouched = bool(torch.isnan(yg[:GUARD]).all()) and bool(torch.isnan(yg[GUARD + rows * c:]).all())
    return xg.cpu(), yg[GUARD:GUARD + rows * c].reshape(rows, c).cpu(), untouched


def _check_aln(x_buf, branch_buf, gamma, beta, *, rows, c, stride, dtype, what):
    """All three modes on one set of rows: the written ``x`` is the CPU's float32 ``x + branch.float()`` bit for bit and everything
    else of the buffer (guards, the values between strided rows) keeps its bits; ``y`` is within ``u |ref| + 2^-16 max |ref|`` of the
    float64 LayerNorm of the ``x`` the kernel wrote; LayerNorm alone leaves ``x`` bit-identical."""
    used = (rows - 1) * stride + c
    want = x_buf.clone()
    want[:, :c] += branch_buf[:, :c].float()  # one IEEE float32 add per element, as the kernel's
    want_g = torch.cat([torch.full((GUARD,), float("nan")), want.reshape(-1)[:used], torch.full((GUARD,), float("nan"))])
    same_g = torch.cat([torch.full((GUARD,), float("nan")), x_buf.reshape(-1)[:used], torch.full((GUARD,), float("nan"))])
    ref_sum, ref_x = _ln64(want[:, :c], gamma, beta), _ln64(x_buf[:, :c], gamma, beta)
    worst = 0.0
    for y_dtype in (dtype, torch.float32):
        for branch, x_want, ref in ((branch_buf, want_g, ref_sum), (None, same_g, ref_x)):
            x_after, y, untouched = _run_aln(x_buf, branch, gamma, beta, y_dtype, rows=rows, c=c, stride=stride, dtype=dtype)
            assert untouched and torch.equal(_bits(x_after), _bits(x_want)), (what, y_dtype, branch is None)
            assert y.dtype == y_dtype and bool(torch.isfinite(y).all())
            bound = UNIT[y_dtype] * ref.abs() + 2.0 ** -16 * float(ref.abs().max())
            worst = max(worst, float(((y.double() - ref).abs() / bound).max()))
    x_after, y, _ = _run_aln(x_buf, branch_buf, gamma, beta, None, rows=rows, c=c, stride=stride, dtype=dtype)  # the add alone
    assert y is None and torch.equal(_bits(x_after), _bits(want_g)), what
    print(f"add_layernorm {what}: {worst:.3f} of the bound")
    assert worst <= 1.0


def _aln_rows(g, rows, c, stride, dtype):
    """Rows with std in [0.5, 4] and mean within +-2 std (the rows of ``test_layernorm_rows``) in float32, a half branch of std in
    [0.01, 1] per row; the columns between strided rows hold other draws."""
    std = torch.rand((rows, 1), generator=g) * 3.5 + 0.5
    mean = (torch.rand((rows, 1), generator=g) * 4.0 - 2.0) * std
    x = torch.randn((rows, stride), generator=g)
    x[:, :c] = torch.randn((rows, c), generator=g) * std + mean
    branch = (torch.randn((rows, stride), generator=g) * (torch.rand((rows, 1), generator=g) * 0.99 + 0.01)).to(dtype)
    return x, branch


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [8, 128, 512, 520, 1280, 1536])  # one lane; the step from one to two vectors per lane at 512; 3 per lane
def test_add_layernorm_rows(c, dtype):
    g = torch.Generator().manual_seed(c)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    for rows in (1, 3, 5, 394):  # against four rows per workgroup
        for stride in (c, 5 * c):  # dense, and the class-row form
            x, branch = _aln_rows(g, rows, c, stride, dtype)
            _check_aln(x, branch, gamma, beta, rows=rows, c=c, stride=stride, dtype=dtype, what=f"c={c} rows={rows} stride={stride} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [4096, 8192])  # 8 and 16 vectors per lane
def test_add_layernorm_rows_wide(c, dtype):
    g = torch.Generator().manual_seed(c)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    for stride in (c, 5 * c):
        x, branch = _aln_rows(g, 2, c, stride, dtype)
        _check_aln(x, branch, gamma, beta, rows=2, c=c, stride=stride, dtype=dtype, what=f"c={c} rows=2 stride={stride} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [128, 1536])
def test_add_layernorm_centres_before_the_variance(c, dtype):
    """A row of mean 1e3 and unit spread.  The row is built so that the float32 arithmetic in front of the centring is exact, and the
    usual gate then holds the centring alone: ``x = 1000 + e`` and the branch ``b`` lie on a grid of 1/8 (``|b| <= 4``: exact in both
    half types), ``d = e + b`` is a unit-spread draw taken with its negative, so every partial sum of the row is a multiple of 1/8
    below ``1536 * 1004 < 2^21`` -- exact in float32 in any order -- the row sum is ``1000 c`` and the mean 1000 exactly.  A variance
    taken as ``E[x^2] - mean^2`` rounds ``x^2 ~ 1e6`` to 1/16 and misses the gate by orders of magnitude."""
    g = torch.Generator().manual_seed(c + 1)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    rows = 3
    half = (torch.randn((rows, c // 2), generator=g) * 8.0).round().clamp(-24, 24) / 8.0
    d = torch.cat([half, -half], dim=1)[:, torch.randperm(c, generator=g)]
    b = torch.randint(-32, 33, (rows, c), generator=g).float() / 8.0
    x, branch = 1000.0 + (d - b), b.to(dtype)
    assert torch.equal(branch.float(), b) and torch.equal((x + b).double(), 1000.0 + d.double())
    assert bool(((x + b).double().mean(-1) == 1000.0).all())  # noqa: PLR2004
    _check_aln(x, branch, gamma, beta, rows=rows, c=c, stride=c, dtype=dtype, what=f"mean 1e3, c={c} {dtype}")


def test_add_layernorm_wrapper_returns_the_entry_points_bits():
    from tiatoolbox_amd.models.architecture.vit_fused import hip_add_layernorm_rows_f32

    g = torch.Generator().manual_seed(5)
    n, s, c, dtype = 2, 5, 136, torch.bfloat16
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    x, branch = _aln_rows(g, n * s, c, c, dtype)
    x_after, y, _ = _run_aln(x, branch, gamma, beta, dtype, rows=n * s, c=c, stride=c, dtype=dtype)
    xd = x.reshape(n, s, c).cuda()
    got = hip_add_layernorm_rows_f32(xd, branch.reshape(n, s, c).cuda(), gamma.cuda(), beta.cuda(), eps=EPS, rows=n * s, row_stride=c, dtype=dtype)
    assert got.dtype == dtype and torch.equal(got.cpu(), y) and torch.equal(xd.cpu().reshape(-1), x_after[GUARD:-GUARD])
    # the class rows alone (both strides S * D), float32 out: the other rows of x keep their values
    xd = x.reshape(n, s, c).cuda()
    got = hip_add_layernorm_rows_f32(xd, branch.reshape(n, s, c).cuda(), gamma.cuda(), beta.cuda(), eps=EPS, rows=n, row_stride=s * c, dtype=dtype,
                                     out_dtype=torch.float32)
    want = x.reshape(n, s, c).clone()
    want[:, 0] += branch.reshape(n, s, c)[:, 0].float()
    assert got.shape == (n, c) and got.dtype == torch.float32 and torch.equal(xd.cpu(), want)


# ------------------------------------------------------------------------------------------------------------------------------------
# tia_vit_assemble_rows_f32
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["plain", "registers-no-class-entry", "host-folded-prefix"])
def test_assemble_rows_is_the_float32_add(form, dtype):
    """``(R, pos_has_cls)``: (0, 1) the plain form, (4, 0) register tokens beside a table without a class entry, (3, 0) with the
    prefix rows' position entries folded in on the host (``FusedViT._prefix_for``).  The result is the CPU's float32 adds bit for bit,
    the class and register rows the float32 inputs themselves; nothing is written around it."""
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_assemble_rows_f32

    nreg, has_cls = {"plain": (0, True), "registers-no-class-entry": (4, False), "host-folded-prefix": (3, False)}[form]
    gen = torch.Generator().manual_seed(nreg)
    for n in (1, 3):
        for g in (1, 4, 12):  # 12: a 3 x 4 grid
            for d in (8, 128, 320):
                tok = torch.randn((n, g, d), generator=gen).to(dtype)
                cls, reg = torch.randn(d, generator=gen), (torch.randn((nreg, d), generator=gen) if nreg else None)
                pos = torch.randn((g + int(has_cls), d), generator=gen)
                if form == "host-folded-prefix":  # the table has 1 + R prefix entries: folded in float32 before the call
                    table = torch.randn((1 + nreg + g, d), generator=gen)
                    cls, reg, pos = cls + table[0], reg + table[1:1 + nreg], table[1 + nreg:].contiguous()
                parts = [(cls + pos[0] if has_cls else cls).expand(n, 1, d)]
                if nreg:
                    parts.append(reg.expand(n, nreg, d))
                parts.append(tok.float() + pos[int(has_cls):])
                want = torch.cat(parts, 1)
                s = 1 + nreg + g
                buf = torch.full((2 * GUARD + n * s * d,), float("nan"), device="cuda")
                tk, cl, rg, ps = tok.cuda(), cls.cuda(), (reg.cuda() if nreg else None), pos.cuda()
                rc = _lib.load().tia_vit_assemble_rows_f32(tk.data_ptr(), cl.data_ptr(), rg.data_ptr() if nreg else None, ps.data_ptr(),
                                                           int(has_cls), buf.data_ptr() + 4 * GUARD, n, g, nreg, d, _dt(dtype),
                                                           _lib.current_stream())
                assert rc == 0
                torch.cuda.synchronize()
                assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n * s * d:]).all())
                got = buf[GUARD:GUARD + n * s * d].reshape(n, s, d).cpu()
                assert torch.equal(got, want), (form, n, g, d)
                if not has_cls:
                    assert torch.equal(got[:, 0], cls.expand(n, d)) and (not nreg or torch.equal(got[:, 1:1 + nreg], reg.expand(n, nreg, d)))
                assert torch.equal(hip_vit_assemble_rows_f32(tk, cl, rg, ps, pos_has_cls=has_cls).cpu(), want)


# ------------------------------------------------------------------------------------------------------------------------------------
# tia_vit_cls_mean_pool_f32
# ------------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 2, 1, 8), (3, 9, 4, 320), (2, 261, 5, 1280), (2, 7, 2, 4096), (2, 6, 3, 8192)]


def _pool(x, branch, gamma, beta, skip, dtype):
    """The entry point into the middle of a NaN-filled buffer: (result ``[n, 2d]``, whether both guards are still NaN)."""
    from tiatoolbox_amd import _lib

    n, s, d = x.shape
    buf = torch.full((2 * GUARD + n * 2 * d,), float("nan"), dtype=torch.float32, device="cuda")
    rc = _lib.load().tia_vit_cls_mean_pool_f32(x.data_ptr(), branch.data_ptr() if branch is not None else None, gamma.data_ptr(),
                                               beta.data_ptr(), EPS, buf.data_ptr() + 4 * GUARD, n, s, skip, d, _dt(dtype),
                                               _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n * 2 * d:]).all())
    return buf[GUARD:GUARD + n * 2 * d].reshape(n, 2 * d).clone(), untouched


@functools.lru_cache(maxsize=None)
def _pool_case(n: int, s: int, d: int, dtype: torch.dtype):
    """Float32 rows with std in [0.5, 4] and mean within +-2 std, a half branch, the affine (the rows of ``test_cls_mean_pool``)."""
    g = torch.Generator().manual_seed(n * 1000 + s * 10 + d)
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.3
    std = torch.rand((n, s, 1), generator=g) * 3.5 + 0.5
    mean = (torch.rand((n, s, 1), generator=g) * 4.0 - 2.0) * std
    x = torch.randn((n, s, d), generator=g) * std + mean
    branch = (torch.randn((n, s, d), generator=g) * 0.5).to(dtype)
    return x, branch, gamma, beta


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_branch", [False, True], ids=["no-branch", "branch"])
@pytest.mark.parametrize(("n", "s", "skip", "d"), POOL_SHAPES)
def test_cls_mean_pool_f32(n, s, skip, d, with_branch, dtype):
    """The bounds of ``test_cls_mean_pool`` for the two halves of the output, against the float64 LayerNorm of
    ``x (+ branch.float())``, the sum taken in float32 on the CPU (the kernel's one add): class half ``u |ref| + 2^-16 max |ref|`` with
    ``u = 2^-22``; mean half ``u mean_i |y_i| + 2^-16 A``.  Every image equals its own ``n = 1`` call bit for bit, nothing is written
    outside ``[n, 2d]``, ``x`` keeps its bits, and the wrapper returns the entry point's bits."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_cls_mean_pool_f32

    x, branch, gamma, beta = _pool_case(n, s, d, dtype)
    y = _ln64(x + branch.float() if with_branch else x, gamma, beta)
    xd, bd, gd, btd = x.cuda(), (branch.cuda() if with_branch else None), gamma.cuda(), beta.cuda()
    got, untouched = _pool(xd, bd, gd, btd, skip, dtype)
    assert untouched and bool(torch.isfinite(got).all()) and torch.equal(xd.cpu(), x)
    assert torch.equal(hip_vit_cls_mean_pool_f32(xd, bd, gd, btd, eps=EPS, skip=skip, dtype=dtype), got)
    for b in range(n):
        alone, untouched = _pool(xd[b:b + 1].contiguous(), bd[b:b + 1].contiguous() if with_branch else None, gd, btd, skip, dtype)
        assert untouched and torch.equal(alone[0], got[b]), b
    got = got.cpu().double()
    u32 = UNIT[torch.float32]
    ref_cls, rows = y[:, 0], y[:, skip:]
    bound = u32 * ref_cls.abs() + 2.0 ** -16 * float(ref_cls.abs().max())
    worst_cls = float(((got[:, :d] - ref_cls).abs() / bound).max())
    bound = u32 * rows.abs().mean(1) + 2.0 ** -16 * float(rows.abs().max())
    worst_mean = float(((got[:, d:] - rows.mean(1)).abs() / bound).max())
    print(f"cls_mean_pool_f32 n={n} s={s} skip={skip} d={d} branch={with_branch} {dtype}: class {worst_cls:.4f}, mean {worst_mean:.4f} of the bound")
    assert worst_cls <= 1.0 and worst_mean <= 1.0
    if with_branch:  # the branch is in the result: without it the class half is another vector
        assert float((got[:, :d] - _ln64(x, gamma, beta)[:, 0]).abs().max()) > 1e-3  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def _refusals(entry, names, ok, cases, stream):
    def call(**over):
        return entry(*[over.get(k, v) for k, v in zip(names, ok)], stream)

    for over, code in cases:
        assert call(**over) == code, over
    return call


def test_add_layernorm_refuses_before_launching():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    einval, esize, f32, f16, bf16 = _lib.TIA_EINVAL, _lib.TIA_ESIZE, 0, _dt(torch.float16), _dt(torch.bfloat16)
    rows, c = 3, 16
    x = torch.full((rows, c), 7.0, device="cuda")
    branch = torch.ones((rows, c), device="cuda", dtype=torch.float16)
    gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    y = torch.full((rows, c), 7.0, device="cuda", dtype=torch.float16)
    names = ("x", "xs", "branch", "bs", "gamma", "beta", "eps", "y", "yd", "rows", "c", "dtype")
    ok = (x.data_ptr(), c, branch.data_ptr(), c, gamma.data_ptr(), beta.data_ptr(), 1e-6, y.data_ptr(), f16, rows, c, f16)
    cases = [({"x": None}, einval), ({"branch": None, "y": None}, einval), ({"gamma": None}, einval), ({"beta": None}, einval),
             *[({k: ok[names.index(k)] + 4}, einval) for k in ("x", "gamma", "beta", "y")], ({"branch": branch.data_ptr() + 2}, einval),
             ({"dtype": f32}, einval), ({"dtype": 5}, einval), ({"yd": bf16}, einval), ({"yd": 5}, einval), ({"eps": -1.0}, einval),
             ({"rows": 0}, einval), ({"c": 0}, einval), ({"c": -8}, einval), ({"xs": 8}, einval), ({"xs": 18}, einval),
             ({"bs": 8}, einval), ({"bs": 20}, einval), ({"c": 12, "xs": 12, "bs": 16}, esize), ({"c": 8200, "xs": 8200, "bs": 8200}, esize)]
    call = _refusals(lib.tia_add_layernorm_rows_f32, names, ok, cases, stream)
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((y == 7.0).all())  # noqa: PLR2004  (nothing was launched)
    assert call() == 0 and call(yd=f32, y=torch.empty((rows, c), device="cuda").data_ptr()) == 0
    assert call(y=None) == 0 and call(branch=None) == 0  # each part alone; the add alone does not look at the affine
    assert call(y=None, gamma=None, beta=None, eps=-1.0, yd=5) == 0
    torch.cuda.synchronize()
    assert bool((x == 7.0 + 4.0).all()) and bool(torch.isfinite(y).all())  # noqa: PLR2004  (four calls added the branch of ones)


def test_assemble_rows_refuses_before_launching():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    einval, esize, f32, f16 = _lib.TIA_EINVAL, _lib.TIA_ESIZE, 0, _dt(torch.float16)
    n, g, r, d = 2, 3, 2, 16
    tok = torch.ones((n, g, d), device="cuda", dtype=torch.float16)
    cls, reg, pos = torch.ones(d, device="cuda"), torch.ones((r, d), device="cuda"), torch.ones((g, d), device="cuda")
    out = torch.full((n, 1 + r + g, d), 7.0, device="cuda")
    names = ("tok", "cls", "reg", "pos", "has_cls", "out", "n", "g", "r", "d", "dtype")
    ok = (tok.data_ptr(), cls.data_ptr(), reg.data_ptr(), pos.data_ptr(), 0, out.data_ptr(), n, g, r, d, f16)
    cases = [*[({k: None}, einval) for k in ("tok", "cls", "reg", "pos", "out")], ({"r": 0}, einval),  # (reg beside R = 0)
             *[({k: ok[names.index(k)] + 4}, einval) for k in ("cls", "reg", "pos", "out")], ({"tok": tok.data_ptr() + 2}, einval),
             ({"has_cls": 2}, einval), ({"dtype": f32}, einval), ({"dtype": 5}, einval), ({"n": 0}, einval), ({"g": 0}, einval),
             ({"d": 0}, einval), ({"r": -1}, einval), ({"d": 12}, esize), ({"d": 8200}, esize)]
    call = _refusals(lib.tia_vit_assemble_rows_f32, names, ok, cases, stream)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # noqa: PLR2004  (nothing was launched)
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())  # noqa: PLR2004


def test_cls_mean_pool_f32_refuses_before_launching():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    einval, esize, f32, f16 = _lib.TIA_EINVAL, _lib.TIA_ESIZE, 0, _dt(torch.float16)
    n, s, skip, d = 2, 6, 2, 16
    x = torch.randn((n, s, d), device="cuda")
    branch = torch.ones((n, s, d), device="cuda", dtype=torch.float16)
    gamma, beta = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
    out = torch.full((n, 2 * d), 7.0, device="cuda")
    names = ("x", "branch", "gamma", "beta", "eps", "out", "n", "s", "skip", "d", "dtype")
    ok = (x.data_ptr(), branch.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-6, out.data_ptr(), n, s, skip, d, f16)
    cases = [*[({k: None}, einval) for k in ("x", "gamma", "beta", "out")],
             *[({k: ok[names.index(k)] + 4}, einval) for k in ("x", "gamma", "beta", "out")], ({"branch": branch.data_ptr() + 2}, einval),
             ({"dtype": f32}, einval), ({"dtype": 5}, einval), ({"n": 0}, einval), ({"s": 0}, einval), ({"d": 0}, einval), ({"d": -8}, einval),
             ({"eps": -1.0}, einval), ({"skip": 0}, einval), ({"skip": -1}, einval), ({"skip": s}, einval), ({"skip": s + 3}, einval),
             ({"d": 12}, esize), ({"d": 8200}, esize)]
    call = _refusals(lib.tia_vit_cls_mean_pool_f32, names, ok, cases, stream)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # noqa: PLR2004  (nothing was launched)
    assert call() == 0 and call(branch=None) == 0 and call(skip=s - 1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())  # noqa: PLR2004

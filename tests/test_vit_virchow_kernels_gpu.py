"""The kernels ``Virchow`` / ``Virchow2`` add (attention at 80 dimensions per head in ``csrc/vit_attention.hip``, the class + mean-patch
pooling in ``csrc/vit_rows.hip``) against float64 references computed on the CPU from exactly the half values the kernels are given,
in fp16 and bf16; LayerNorm and the half GEMM at the new widths; the entry points' refusals."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from _conv_ref import Case, check_tolerance, conv_ref64, epilogue64, make_data

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
HD = 80
SCALE = HD ** -0.5
SEQ = [1, 2, 15, 16, 17, 63, 64, 65, 129, 257, 261]
U32 = 2.0 ** -22  # one unit in the last place of a float32 output (the figure of `test_vit_kernels_gpu.UNIT`)


def _dt(dtype: torch.dtype) -> int:
    from tiatoolbox_amd.models.architecture.fused import _DT

    return _DT[dtype]


# ------------------------------------------------------------------------------------------------------------------------------------
# attention at head_dim 80
# ------------------------------------------------------------------------------------------------------------------------------------
def _attention_data(kind: str, n: int, heads: int, s: int, dtype: torch.dtype, hd: int = HD) -> torch.Tensor:
    """``[n, s, 3, heads, hd]`` of ``dtype``, the kinds of ``test_vit_kernels_gpu``.  ``late``: every key of the LAST 64-key tile scores
    about 40 above every earlier key for every query -- a shared component on dimension 72 (the padded third k-step carries it): 6 in
    the queries, 60 in those keys, times the 80^-1/2 scale -- so the running maximum jumps in the last tile."""
    g = torch.Generator().manual_seed(s * 131 + heads * 7 + n + len(kind))
    qkv = torch.randn((n, s, 3, heads, hd), generator=g)
    if kind == "late":
        t0 = 64 * ((s - 1) // 64)
        qkv[:, :, 0, :, hd - 8] = 6.0
        qkv[:, :, 1, :, hd - 8] = 0.0
        qkv[:, t0:, 1, :, hd - 8] = 60.0
    elif kind == "equal":
        qkv[:, :, 1] = qkv[:, :1, 1]
    return qkv.to(dtype)


@functools.lru_cache(maxsize=None)
def _attention_case(kind: str, n: int, heads: int, s: int, dtype: torch.dtype, hd: int = HD):
    """(input, float64 reference ``[n, s, heads * hd]``, error of the CPU's half ``scaled_dot_product_attention`` against it)."""
    qkv = _attention_data(kind, n, heads, s, dtype, hd)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))  # [n, heads, s, hd]
    sc = (q.double() @ k.double().transpose(-2, -1)) * hd ** -0.5
    ref = (torch.softmax(sc, -1) @ v.double()).permute(0, 2, 1, 3).reshape(n, s, heads * hd)
    yard = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n, s, heads * hd)
    e_yard = float((yard.double() - ref).abs().max()) / float(ref.abs().max())
    return qkv, ref, e_yard


def _attention_error(qkv, ref, n, heads, s, dtype, hd: int = HD) -> float:
    from tiatoolbox_amd.models.architecture.vit_fused import hip_mha_fwd_h

    out = hip_mha_fwd_h(qkv.cuda().reshape(n, s, 3 * heads * hd), heads, hd ** -0.5)
    assert out.shape == (n, s, heads * hd) and out.dtype == dtype
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all())
    return float((got - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["gauss", "late", "equal"])
@pytest.mark.parametrize(("n", "heads", "s"), [*[(2, 3, s) for s in SEQ], (1, 16, 257)])
def test_attention_80_matches_float64(n, heads, s, kind, dtype):
    """``e = max |out - ref| / max |ref|`` at most twice what the CPU's own half attention leaves (the project's usual margin)."""
    qkv, ref, e_yard = _attention_case(kind, n, heads, s, dtype)
    e_new = _attention_error(qkv, ref, n, heads, s, dtype)
    print(f"attention80 {kind} n={n} heads={heads} s={s} {dtype}: e_new {e_new:.3e}  e_yard {e_yard:.3e}")
    assert e_new <= 2.0 * e_yard


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("s", [17, 64, 261])
def test_attention_80_selects_rows_bit_for_bit(s, dtype):
    """Key ``j`` carries the +-1 code of ``j`` in dimensions 70..79 (real lanes of the padded third k-step), query ``i`` 512 x the code of
    a seeded target: the target leads every other key by >= 2 * 512 * 80^-1/2 = 114 after the scale, ``exp2`` of the rest is exactly 0
    in float32 and ``l == 1`` -- the output must BE the target's ``v`` row (integers in [-8, 8] over all 80 dimensions, so every one of
    the five output blocks is checked)."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_mha_fwd_h

    n, heads = 2, 3
    rng = np.random.default_rng(s)
    code = (((np.arange(s)[:, None] >> np.arange(10)[None, :]) & 1) * 2 - 1).astype(np.float32)  # [s, 10]
    target = rng.integers(0, s, (n, heads, s))
    qkv = np.zeros((n, s, 3, heads, HD), np.float32)
    qkv[:, :, 1, :, 70:] = code[None, :, None, :]
    for b in range(n):
        for h in range(heads):
            qkv[b, :, 0, h, 70:] = 512.0 * code[target[b, h]]
    v = rng.integers(-8, 9, (n, s, heads, HD)).astype(np.float32)
    qkv[:, :, 2] = v
    t = torch.from_numpy(qkv).to(dtype)
    assert torch.equal(t.float(), torch.from_numpy(qkv))  # every value is representable
    out = hip_mha_fwd_h(t.cuda().reshape(n, s, 3 * heads * HD), heads, SCALE).cpu().float().reshape(n, s, heads, HD).numpy()
    exp = np.stack([np.stack([v[b, target[b, h], h] for h in range(heads)], axis=1) for b in range(n)])  # [n, s, heads, 80]
    assert np.isfinite(out).all()
    wrong = np.argwhere((out != exp).any(-1))
    assert wrong.size == 0, f"{len(wrong)} (image, query, head) rows differ; first {wrong[:4].tolist()}"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_80_pad_lanes_never_see_stale_memory(dtype):
    """One launch on a ``qkv`` of NaN (its output is NaN: expected, no fault), then ``gauss`` data on the same device: finite and within
    the bound.  A pad lane of the third k-step that read LDS left by the first launch would give 0 x NaN = NaN."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_mha_fwd_h

    n, heads, s = 2, 3, 129
    poison = torch.full((n, s, 3 * heads * HD), float("nan"), dtype=dtype, device="cuda")
    assert bool(torch.isnan(hip_mha_fwd_h(poison, heads, SCALE)).all())
    qkv, ref, e_yard = _attention_case("gauss", n, heads, s, dtype)
    e_new = _attention_error(qkv, ref, n, heads, s, dtype)
    print(f"attention80 after a NaN launch s={s} {dtype}: e_new {e_new:.3e}  e_yard {e_yard:.3e}")
    assert e_new <= 2.0 * e_yard


def test_attention_entry_takes_64_and_80_only():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    esize, f16 = _lib.TIA_ESIZE, 1
    n, heads, s = 1, 2, 4
    for hd, code in ((80, 0), (64, 0), (32, esize), (96, esize), (72, esize), (88, esize), (160, esize)):
        qkv = torch.randn((n, s, 3 * heads * hd), device="cuda").half()
        out = torch.full((n, s, heads * hd), 7.0, device="cuda", dtype=torch.float16)
        assert lib.tia_mha_fwd_h(qkv.data_ptr(), out.data_ptr(), n, s, heads, hd, hd ** -0.5, f16, stream) == code, hd
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool((out == 7.0).all()) == (code != 0)  # noqa: PLR2004  (nothing launched on a refusal)
    # the other refusals keep their order: a null pointer beside an unsupported head_dim is TIA_EINVAL, as before
    assert lib.tia_mha_fwd_h(None, out.data_ptr(), n, s, heads, 96, 0.1, f16, stream) == _lib.TIA_EINVAL
    assert lib.tia_mha_fwd_h(qkv.data_ptr(), out.data_ptr(), n, s, heads, 80, 0.0, f16, stream) == _lib.TIA_EINVAL  # scale
    assert lib.tia_mha_fwd_h(qkv.data_ptr() + 2, out.data_ptr(), n, s, heads, 80, 0.1, f16, stream) == _lib.TIA_EINVAL  # misaligned
    assert lib.tia_mha_fwd_h(qkv.data_ptr(), out.data_ptr(), n, s, 0x7fffffff // 240 + 1, 80, 0.1, f16, stream) == esize  # 3 * 80 * heads
    # the 64 form beside it, on a fixed input: the accuracy it had
    for dtype in DTYPES:
        qkv, ref, e_yard = _attention_case("gauss", 2, 3, 129, dtype, 64)
        e_new = _attention_error(qkv, ref, 2, 3, 129, dtype, 64)
        print(f"attention64 gauss s=129 {dtype}: e_new {e_new:.3e}  e_yard {e_yard:.3e}")
        assert e_new <= 2.0 * e_yard


# ------------------------------------------------------------------------------------------------------------------------------------
# class + mean-patch pooling
# ------------------------------------------------------------------------------------------------------------------------------------
# (the last two: the widest rows the entry takes, 8 and 16 vectors per lane -- kernel forms no registered model reaches)
POOL_SHAPES = [(1, 2, 1, 8), (3, 9, 4, 320), (2, 261, 5, 1280), (1, 257, 1, 1536), (2, 7, 2, 4096), (2, 6, 3, 8192)]


def _pool(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, skip: int, guard: int = 64):
    """The entry point into the middle of a NaN-filled buffer: (result ``[n, 2d]``, whether both guards are still NaN)."""
    from tiatoolbox_amd import _lib

    n, s, d = x.shape
    buf = torch.full((guard + n * 2 * d + guard,), float("nan"), dtype=torch.float32, device="cuda")
    rc = _lib.load().tia_vit_cls_mean_pool_h(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-6, buf.data_ptr() + 4 * guard, n, s, skip, d,
                                             _dt(x.dtype), _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    untouched = bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n * 2 * d:]).all())
    return buf[guard:guard + n * 2 * d].reshape(n, 2 * d).clone(), untouched


@functools.lru_cache(maxsize=None)
def _pool_case(n: int, s: int, d: int, dtype: torch.dtype):
    """Rows with std in [0.5, 4] and mean within +-2 std (the rows of ``test_layernorm_rows``), the affine, the float64 LayerNorm."""
    g = torch.Generator().manual_seed(n * 1000 + s * 10 + d)
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.3
    std = torch.rand((n, s, 1), generator=g) * 3.5 + 0.5
    mean = (torch.rand((n, s, 1), generator=g) * 4.0 - 2.0) * std
    x = (torch.randn((n, s, d), generator=g) * std + mean).to(dtype)
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    y = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-6) * gamma.double() + beta.double()
    return x, gamma, beta, y


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize(("n", "s", "skip", "d"), POOL_SHAPES)
def test_cls_mean_pool(n, s, skip, d, dtype):
    """Class half: ``|delta| <= u |ref| + 2^-16 max |ref|`` with ``u = 2^-22``, ``test_layernorm_rows``'s criterion for a float32 output.
    Mean half: the same criterion carried through the mean of its addends, ``u mean_i |y_i| + 2^-16 A`` with ``y_i`` the reference's
    normalised rows ``skip .. s - 1`` and ``A`` their largest magnitude.  Every image equals its own ``n = 1`` call bit for bit, nothing
    is written outside ``[n, 2d]``, and the wrapper returns the entry point's bits."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_cls_mean_pool_h

    x, gamma, beta, y = _pool_case(n, s, d, dtype)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    got, untouched = _pool(xd, gd, bd, skip)
    assert untouched and bool(torch.isfinite(got).all())
    assert torch.equal(hip_vit_cls_mean_pool_h(xd, gd, bd, eps=1e-6, skip=skip), got)
    for b in range(n):
        alone, untouched = _pool(xd[b:b + 1].contiguous(), gd, bd, skip)
        assert untouched and torch.equal(alone[0], got[b]), b
    got = got.cpu().double()
    ref_cls, rows = y[:, 0], y[:, skip:]
    bound = U32 * ref_cls.abs() + 2.0 ** -16 * float(ref_cls.abs().max())
    worst_cls = float(((got[:, :d] - ref_cls).abs() / bound).max())
    bound = U32 * rows.abs().mean(1) + 2.0 ** -16 * float(rows.abs().max())
    worst_mean = float(((got[:, d:] - rows.mean(1)).abs() / bound).max())
    print(f"cls_mean_pool n={n} s={s} skip={skip} d={d} {dtype}: class {worst_cls:.4f}, mean {worst_mean:.4f} of the bound")
    assert worst_cls <= 1.0 and worst_mean <= 1.0
    if skip > 1:  # the register rows are left out: with them the mean is another vector
        assert float((got[:, d:] - y[:, 1:].mean(1)).abs().max()) > 1e-3  # noqa: PLR2004


def test_cls_mean_pool_refuses_before_launching():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    einval, esize, f32, f16 = _lib.TIA_EINVAL, _lib.TIA_ESIZE, 0, 1
    n, s, skip, d = 2, 6, 2, 16
    x = torch.randn((n, s, d), device="cuda").half()
    gamma, beta = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
    out = torch.full((n, 2 * d), 7.0, device="cuda")
    ok = (x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-6, out.data_ptr(), n, s, skip, d, f16)
    names = ("x", "gamma", "beta", "eps", "out", "n", "s", "skip", "d", "dtype")

    def pool(**over):
        return lib.tia_vit_cls_mean_pool_h(*[over.get(k, v) for k, v in zip(names, ok)], stream)

    for name in ("x", "gamma", "beta", "out"):
        assert pool(**{name: None}) == einval, name                           # null
        assert pool(**{name: ok[names.index(name)] + 4}) == einval, name      # misaligned
    assert pool(dtype=f32) == einval and pool(dtype=5) == einval
    assert pool(n=0) == einval and pool(s=0) == einval and pool(d=0) == einval and pool(d=-8) == einval and pool(eps=-1.0) == einval
    assert pool(skip=0) == einval and pool(skip=-1) == einval and pool(skip=s) == einval and pool(skip=s + 3) == einval
    assert pool(d=12) == esize and pool(d=8200) == esize                      # d % 8, d > 8192
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # noqa: PLR2004  (nothing was launched)
    assert pool() == 0 and pool(skip=s - 1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm and the half GEMM at the new widths
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [320, 1280])
def test_layernorm_rows_at_the_new_widths(c, dtype):
    """``test_vit_kernels_gpu.test_layernorm_rows``'s rows and bound, ``|delta| <= u |ref| + 2^-16 max |ref|``, at 320 and 1280 channels."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_layernorm_rows_h

    unit = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: U32}
    g = torch.Generator().manual_seed(c)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    for rows in (1, 3, 261):
        for stride in (c, 5 * c):
            std = torch.rand((rows, 1), generator=g) * 3.5 + 0.5
            mean = (torch.rand((rows, 1), generator=g) * 4.0 - 2.0) * std
            buf = torch.randn((rows, stride), generator=g).to(dtype)
            buf[:, :c] = (torch.randn((rows, c), generator=g) * std + mean).to(dtype)
            x = buf[:, :c].double()
            mu = x.mean(-1, keepdim=True)
            ref = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-6) * gamma.double() + beta.double()
            for out_dtype in (dtype, torch.float32):
                got = hip_layernorm_rows_h(buf.cuda(), gamma.cuda(), beta.cuda(), eps=1e-6, rows=rows, row_stride=stride, out_dtype=out_dtype)
                assert got.shape == (rows, c) and got.dtype == out_dtype
                bound = unit[out_dtype] * ref.abs() + 2.0 ** -16 * float(ref.abs().max())
                worst = float(((got.cpu().double() - ref).abs() / bound).max())
                print(f"layernorm c={c} rows={rows} stride={stride} {dtype} -> {out_dtype}: {worst:.3f} of the bound")
                assert worst <= 1.0


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize(("n", "s", "cin", "cout"), [(2, 9, 320, 960), (1, 5, 544, 320)])
def test_linear_at_the_new_widths(n, s, cin, cout, dtype):
    """The qkv GEMM of a 320-wide model and ``fc2`` on a padded SwiGLU half (544), bias and residual fused: the criterion and the
    float64 reference of the convolution sweep (``_conv_ref``)."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_linear_h, pack_linear_weights_h

    case = Case("half", n, cin, cout, s, 1, k=1, stride=1, pad_lo=0, pad_hi=0, dtype=dtype)
    dt = getattr(torch, dtype)
    x, weight, bias, res = make_data(case, seed=cin + s)
    ref = epilogue64(conv_ref64(case, x, weight), bias, res.double(), relu=False)
    tokens = x.permute(0, 2, 3, 1).reshape(n, s, cin).contiguous().to(dt).cuda()
    residual = res.permute(0, 2, 3, 1).reshape(n, s, cout).contiguous().to(dt).cuda()
    packed = pack_linear_weights_h(weight.reshape(cout, cin).cuda(), dt)
    got = hip_linear_h(tokens, packed, bias.cuda(), residual, cout=cout)
    assert got.shape == (n, s, cout) and got.dtype == dt
    ratio = check_tolerance(case, (True, True, False), got.cpu().reshape(n, s, 1, cout).permute(0, 3, 1, 2), ref)
    print(f"linear {n}x{s}x{cin} -> {cout} {dtype}: {ratio:.3f} of the gate")

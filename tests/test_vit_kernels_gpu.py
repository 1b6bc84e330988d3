"""The Vision Transformer kernels (``csrc/vit_attention.hip``, ``csrc/vit_rows.hip``) against float64 references computed on the CPU
from exactly the half values the kernels are given, in fp16 and bf16; the half GEMM at token shapes; the entry points' refusals."""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from _conv_ref import Case, check_tolerance, conv_ref64, epilogue64, make_data

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
UNIT = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -22}  # one unit in the last place of the output
SEQ = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 197, 257, 577]


# ------------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------------
def _attention_data(kind: str, n: int, heads: int, s: int, dtype: torch.dtype) -> torch.Tensor:
    """``[n, s, 3, heads, 64]`` of ``dtype``.  ``gauss``: normal q, k, v.  ``late``: every key of the LAST 64-key tile scores about
    45 above every earlier key for every query (a shared component on dimension 0: 6 in the queries, 60 in those keys, times the
    0.125 scale), so the running maximum jumps there and everything accumulated before is rescaled by ~exp(-45).  ``equal``: all
    keys identical, so every score of a query is the same."""
    g = torch.Generator().manual_seed(s * 131 + heads * 7 + n + len(kind))
    qkv = torch.randn((n, s, 3, heads, 64), generator=g)
    if kind == "late":
        t0 = 64 * ((s - 1) // 64)
        qkv[:, :, 0, :, 0] = 6.0
        qkv[:, :, 1, :, 0] = 0.0
        qkv[:, t0:, 1, :, 0] = 60.0
    elif kind == "equal":
        qkv[:, :, 1] = qkv[:, :1, 1]
    return qkv.to(dtype)


@functools.lru_cache(maxsize=None)
def _attention_case(kind: str, n: int, heads: int, s: int, dtype: torch.dtype):
    """(input, float64 reference ``[n, s, heads * 64]``, error of the CPU's half ``scaled_dot_product_attention`` against it)."""
    qkv = _attention_data(kind, n, heads, s, dtype)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))  # [n, heads, s, 64]
    sc = (q.double() @ k.double().transpose(-2, -1)) * 0.125
    ref = (torch.softmax(sc, -1) @ v.double()).permute(0, 2, 1, 3).reshape(n, s, heads * 64)
    yard = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n, s, heads * 64)
    e_yard = float((yard.double() - ref).abs().max()) / float(ref.abs().max())
    return qkv, ref, e_yard


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["gauss", "late", "equal"])
@pytest.mark.parametrize(("n", "heads", "s"), [*[(2, 3, s) for s in SEQ], (1, 16, 197)])
def test_attention_matches_float64(n, heads, s, kind, dtype):
    """``e = max |out - ref| / max |ref|`` at most twice what the CPU's own half attention leaves (the project's usual margin)."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_mha_fwd_h

    qkv, ref, e_yard = _attention_case(kind, n, heads, s, dtype)
    out = hip_mha_fwd_h(qkv.cuda().reshape(n, s, 3 * heads * 64), heads, 0.125)
    assert out.shape == (n, s, heads * 64) and out.dtype == dtype
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all())
    e_new = float((got - ref).abs().max()) / float(ref.abs().max())
    print(f"attention {kind} n={n} heads={heads} s={s} {dtype}: e_new {e_new:.3e}  e_yard {e_yard:.3e}")
    assert e_new <= 2.0 * e_yard


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("s", [17, 64, 197, 577])
def test_attention_selects_rows_bit_for_bit(s, dtype):
    """Key ``j`` carries the +-1 code of ``j`` in its first 10 dimensions, query ``i`` 512 x the code of a seeded target: the target leads
    every other key by >= 128 after the scale, ``exp`` of the rest is exactly 0 in float32 and ``l == 1`` -- the output must BE the
    target's ``v`` row (integers in [-8, 8]).  A wrong key order between P and V, a slip in the masked tail or an ``inf - inf`` gives
    a wrong row or a NaN."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_mha_fwd_h

    n, heads = 2, 3
    rng = np.random.default_rng(s)
    code = (((np.arange(s)[:, None] >> np.arange(10)[None, :]) & 1) * 2 - 1).astype(np.float32)  # [s, 10]
    target = rng.integers(0, s, (n, heads, s))
    qkv = np.zeros((n, s, 3, heads, 64), np.float32)
    qkv[:, :, 1, :, :10] = code[None, :, None, :]
    for b in range(n):
        for h in range(heads):
            qkv[b, :, 0, h, :10] = 512.0 * code[target[b, h]]
    v = rng.integers(-8, 9, (n, s, heads, 64)).astype(np.float32)
    qkv[:, :, 2] = v
    t = torch.from_numpy(qkv).to(dtype)
    assert torch.equal(t.float(), torch.from_numpy(qkv))  # every value is representable
    out = hip_mha_fwd_h(t.cuda().reshape(n, s, 3 * heads * 64), heads, 0.125).cpu().float().reshape(n, s, heads, 64).numpy()
    exp = np.stack([np.stack([v[b, target[b, h], h] for h in range(heads)], axis=1) for b in range(n)])  # [n, s, heads, 64]
    assert np.isfinite(out).all()
    wrong = np.argwhere((out != exp).any(-1))
    assert wrong.size == 0, f"{len(wrong)} (image, query, head) rows differ; first {wrong[:4].tolist()}"


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm, GELU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("c", [128, 384, 768, 1024, 1536])
def test_layernorm_rows(c, dtype):
    """Rows with std in [0.5, 4] and mean within +-2 std; dense and strided (5 c) calls, half and float32 outputs: per element
    ``|delta| <= u |ref| + 2^-16 max |ref|`` with ``u`` one unit in the last place of the output type."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_layernorm_rows_h

    g = torch.Generator().manual_seed(c)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    for rows in (1, 3, 394):
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
                err = (got.cpu().double() - ref).abs()
                bound = UNIT[out_dtype] * ref.abs() + 2.0 ** -16 * float(ref.abs().max())
                worst = float((err / bound).max())
                print(f"layernorm c={c} rows={rows} stride={stride} {dtype} -> {out_dtype}: {worst:.3f} of the bound")
                assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_gelu_rows(dtype):
    """A grid over [-12, 12] and normal draws: ``|delta| <= u |ref| + 2^-22 |x|`` (+ 2^-24 in fp16: its subnormal spacing)."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_gelu_rows_h_

    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.linspace(-12.0, 12.0, 24 * 512 + 8), torch.randn(197 * 1536, generator=g)]).to(dtype)
    assert x.numel() % 8 == 0
    xd = x.double()
    ref = 0.5 * xd * (1.0 + torch.erf(xd / math.sqrt(2.0)))
    got = hip_gelu_rows_h_(x.cuda().clone()).cpu().double()
    bound = UNIT[dtype] * ref.abs() + 2.0 ** -22 * xd.abs() + (2.0 ** -24 if dtype == torch.float16 else 0.0)
    err = (got - ref).abs()
    exact = bound == 0  # x == 0
    assert bool((err[exact] == 0).all())
    worst = float((err[~exact] / bound[~exact]).max())
    print(f"gelu {dtype}: {worst:.3f} of the bound")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------
# patchify, token assembly
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize(("h", "w", "p"), [(32, 48, 16), (224, 224, 16), (16, 8, 8)])
def test_patchify_and_assemble_are_exact(h, w, p, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_assemble_tokens_h, hip_vit_patchify_h

    rng = np.random.default_rng(h + w)
    n, gh, gw = 3, h // p, w // p
    img = rng.integers(0, 256, (n, h, w, 3)).astype(np.float32)
    exp = img.reshape(n, gh, p, gw, p, 3).transpose(0, 1, 3, 2, 4, 5).reshape(n, gh * gw, p * p * 3)  # [b, (gy, gx), (ky, kx, c)]
    for src in (torch.from_numpy(img), torch.from_numpy(img).to(dtype)):  # the float32 batch, and the batch already in the run's type
        tok = hip_vit_patchify_h(src.cuda(), p, dtype)
        assert tok.shape == exp.shape and tok.dtype == dtype
        assert np.array_equal(tok.cpu().float().numpy(), exp)
    d, g = 136, gh * gw  # 17 vectors of 8: no multiple of the wave
    tokens = rng.integers(-64, 65, (n, g, d)).astype(np.float32)
    cls = rng.integers(-64, 65, d).astype(np.float32)
    pos = rng.integers(-64, 65, (1 + g, d)).astype(np.float32)
    want = np.concatenate([np.broadcast_to(cls, (n, 1, d)), tokens], axis=1) + pos[None]
    got = hip_vit_assemble_tokens_h(torch.from_numpy(tokens).to(dtype).cuda(), torch.from_numpy(cls).cuda(), torch.from_numpy(pos).cuda())
    assert got.shape == (n, 1 + g, d) and got.dtype == dtype
    assert np.array_equal(got.cpu().float().numpy(), want)  # |sum| <= 128: exact in both half types


# ------------------------------------------------------------------------------------------------------------------------------------
# the half GEMM at token shapes
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize(("n", "s", "cin", "cout"), [(2, 5, 128, 384), (2, 197, 384, 1536)])
def test_linear_on_the_half_convolution_kernel(n, s, cin, cout, dtype):
    """``tia_conv2d_nhwc_h`` with a 1x1 window on ``[n, S, 1, cin]`` tokens, bias and residual fused: the criterion and the float64
    reference of the convolution sweep (``_conv_ref``)."""
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
    got_nchw = got.cpu().reshape(n, s, 1, cout).permute(0, 3, 1, 2)
    ratio = check_tolerance(case, (True, True, False), got_nchw, ref)
    print(f"linear {n}x{s}x{cin} -> {cout} {dtype}: {ratio:.3f} of the gate")


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_launching():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    einval, esize, f32, f16 = _lib.TIA_EINVAL, _lib.TIA_ESIZE, 0, 1
    qkv = torch.randn((1, 4, 3 * 2 * 64), device="cuda").half()
    out = torch.empty((1, 4, 128), device="cuda", dtype=torch.float16)
    stream = _lib.current_stream()

    def valid_attention():
        assert lib.tia_mha_fwd_h(qkv.data_ptr(), out.data_ptr(), 1, 4, 2, 64, 0.125, f16, stream) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())

    valid_attention()
    for args, code in (((qkv.data_ptr(), out.data_ptr(), 1, 4, 4, 32, 0.125, f16), esize),    # head_dim 32
                       ((qkv.data_ptr(), out.data_ptr(), 1, 0, 2, 64, 0.125, f16), einval),   # s = 0
                       ((None, out.data_ptr(), 1, 4, 2, 64, 0.125, f16), einval),             # null pointer
                       ((qkv.data_ptr(), None, 1, 4, 2, 64, 0.125, f16), einval),
                       ((qkv.data_ptr(), out.data_ptr(), 1, 4, 2, 64, 0.125, f32), einval),   # a float32 dtype code
                       ((qkv.data_ptr() + 2, out.data_ptr(), 1, 4, 2, 64, 0.125, f16), einval)):  # misaligned
        assert lib.tia_mha_fwd_h(*args, stream) == code, args
        valid_attention()
    x = torch.randn((2, 104), device="cuda").half()
    gamma, beta = torch.ones(104, device="cuda"), torch.zeros(104, device="cuda")
    y = torch.empty((2, 104), device="cuda", dtype=torch.float16)
    assert lib.tia_layernorm_rows_h(x.data_ptr(), 100, gamma.data_ptr(), beta.data_ptr(), 1e-6, y.data_ptr(), 2, 100, f16, 0, stream) == esize
    assert lib.tia_layernorm_rows_h(x.data_ptr(), 16384, gamma.data_ptr(), beta.data_ptr(), 1e-6, y.data_ptr(), 1, 8200, f16, 0, stream) == esize
    assert lib.tia_layernorm_rows_h(x.data_ptr(), 104, gamma.data_ptr(), beta.data_ptr(), 1e-6, y.data_ptr(), 2, 104, f32, 0, stream) == einval
    assert lib.tia_layernorm_rows_h(x.data_ptr(), 96, gamma.data_ptr(), beta.data_ptr(), 1e-6, y.data_ptr(), 2, 104, f16, 0, stream) == einval
    assert lib.tia_layernorm_rows_h(x.data_ptr(), 104, gamma.data_ptr(), beta.data_ptr(), 1e-6, y.data_ptr(), 2, 104, f16, 0, stream) == 0
    assert lib.tia_gelu_rows_h(x.data_ptr(), 100, f16, stream) == esize and lib.tia_gelu_rows_h(None, 104, f16, stream) == einval
    assert lib.tia_gelu_rows_h(x.data_ptr(), 208, f16, stream) == 0
    img = torch.zeros((1, 16, 16, 3), device="cuda")
    tok = torch.empty((1, 1, 768), device="cuda", dtype=torch.float16)
    assert lib.tia_vit_patchify_h(img.data_ptr(), f32, tok.data_ptr(), 1, 16, 16, 12, f16, stream) == esize  # patch % 8
    assert lib.tia_vit_patchify_h(img.data_ptr(), f32, tok.data_ptr(), 1, 16, 24, 16, f16, stream) == esize  # w % patch
    assert lib.tia_vit_patchify_h(img.data_ptr(), 2, tok.data_ptr(), 1, 16, 16, 16, f16, stream) == einval   # bf16 input beside fp16 tokens
    assert lib.tia_vit_patchify_h(img.data_ptr(), f32, tok.data_ptr(), 1, 16, 16, 16, f16, stream) == 0
    assert lib.tia_vit_assemble_tokens_h(tok.data_ptr(), gamma.data_ptr(), gamma.data_ptr(), y.data_ptr(), 1, 1, 100, f16, stream) == esize
    assert lib.tia_vit_assemble_tokens_h(tok.data_ptr(), None, gamma.data_ptr(), y.data_ptr(), 1, 1, 104, f16, stream) == einval
    torch.cuda.synchronize()

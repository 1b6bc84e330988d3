"""The kernels of the float32 Vision Transformer route (``csrc/vit_f32.hip``; the Linear on the split-bf16 GEMM at token shapes)
against float64 references computed on the CPU from exactly the float32 values the kernels are given.  Every measured ratio is
printed (collected in ``profiles/vit_f32_tests.txt``)."""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24  # "one float32 unit" of the gates below (the unit round-off, relative)
SEQ = [1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 197, 257]
HEAD_DIMS = [64, 80]
# gates at which exp(-t) overflows in float32 (t < -88.72), their mirror images, and signed zeros (test_vit_foundation_kernels_gpu.py)
SPECIAL_GATES = [-100.0, -89.0, -0.0, 0.0, 30.0, -30.0, 100.0, 89.0, -96.0, -88.0, -90.0, 88.0]


# ------------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------------
def _attention_data(kind: str, n: int, heads: int, s: int, hd: int) -> torch.Tensor:
    """``[n, s, 3, heads, hd]`` float32: the three data sets of ``test_vit_kernels_gpu.py``.  ``gauss``: normal q, k, v.  ``late``: every
    key of the LAST 64-key tile scores about 45 above every earlier key for every query (6 in the queries, 60 in those keys on
    dimension 0, times the scale), so the running maximum jumps there and everything before is rescaled by ~exp(-45).  ``equal``:
    all keys identical, so every score of a query is the same."""
    g = torch.Generator().manual_seed(s * 131 + heads * 7 + n + len(kind) + hd)
    qkv = torch.randn((n, s, 3, heads, hd), generator=g)
    if kind == "late":
        t0 = 64 * ((s - 1) // 64)
        qkv[:, :, 0, :, 0] = 6.0
        qkv[:, :, 1, :, 0] = 0.0
        qkv[:, t0:, 1, :, 0] = 60.0
    elif kind == "equal":
        qkv[:, :, 1] = qkv[:, :1, 1]
    return qkv


@functools.lru_cache(maxsize=None)
def _attention_case(kind: str, n: int, heads: int, s: int, hd: int):
    """(input, float64 reference ``[n, s, heads * hd]``, error of the CPU's float32 ``scaled_dot_product_attention`` against it)."""
    qkv = _attention_data(kind, n, heads, s, hd)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))  # [n, heads, s, hd]
    sc = (q.double() @ k.double().transpose(-2, -1)) / math.sqrt(hd)
    ref = (torch.softmax(sc, -1) @ v.double()).permute(0, 2, 1, 3).reshape(n, s, heads * hd)
    yard = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n, s, heads * hd)
    e_yard = float((yard.double() - ref).abs().max()) / float(ref.abs().max())
    return qkv, ref, e_yard


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("kind", ["gauss", "late", "equal"])
@pytest.mark.parametrize("s", SEQ)
def test_attention_matches_float64(s, kind, hd):
    """``e = max |out - ref| / max |ref| <= 2 e_yard + 8 * 2^-24``: twice what the CPU's own float32 attention leaves (the project's
    rule for a yardstick comparison) plus a floor of eight float32 units -- the rms size of a 64-term float32 dot product's rounding
    -- so that a yardstick that happens to land nearly exact does not fail a correct kernel."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_mha_fwd_f32

    n, heads = 2, 3
    qkv, ref, e_yard = _attention_case(kind, n, heads, s, hd)
    out = hip_mha_fwd_f32(qkv.cuda().reshape(n, s, 3 * heads * hd), heads, hd ** -0.5)
    assert out.shape == (n, s, heads * hd) and out.dtype == torch.float32
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all())
    e_new = float((got - ref).abs().max()) / float(ref.abs().max())
    gate = 2.0 * e_yard + 8.0 * U32
    print(f"attention f32 {kind} hd={hd} s={s}: e_new {e_new:.3e}  e_yard {e_yard:.3e}  {e_new / gate:.3f} of the gate")
    assert e_new <= gate


@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("s", [17, 64, 197, 257])
def test_attention_selects_rows_bit_for_bit(s, hd):
    """The half test's construction: key ``j`` carries the +-1 code of ``j`` in its first 10 dimensions, query ``i`` 512 x the code of a
    seeded target: the target leads every other key by >= 1024 / sqrt(hd) > 114 after the scale, ``exp`` of the rest is exactly 0 in
    float32 and ``l == 1`` -- the output must BE the target's ``v`` row (integers in [-8, 8]).  A wrong key order between P and V, a
    wrong dim order of the output blocks, a slip in the masked tail or an ``inf - inf`` gives a wrong row or a NaN."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_mha_fwd_f32

    n, heads = 2, 3
    rng = np.random.default_rng(s + hd)
    code = (((np.arange(s)[:, None] >> np.arange(10)[None, :]) & 1) * 2 - 1).astype(np.float32)  # [s, 10]
    target = rng.integers(0, s, (n, heads, s))
    qkv = np.zeros((n, s, 3, heads, hd), np.float32)
    qkv[:, :, 1, :, :10] = code[None, :, None, :]
    for b in range(n):
        for h in range(heads):
            qkv[b, :, 0, h, :10] = 512.0 * code[target[b, h]]
    v = rng.integers(-8, 9, (n, s, heads, hd)).astype(np.float32)
    qkv[:, :, 2] = v
    out = hip_mha_fwd_f32(torch.from_numpy(qkv).cuda().reshape(n, s, 3 * heads * hd), heads, hd ** -0.5)
    out = out.cpu().reshape(n, s, heads, hd).numpy()
    exp = np.stack([np.stack([v[b, target[b, h], h] for h in range(heads)], axis=1) for b in range(n)])  # [n, s, heads, hd]
    assert np.isfinite(out).all()
    wrong = np.argwhere((out != exp).any(-1))
    assert wrong.size == 0, f"{len(wrong)} (image, query, head) rows differ; first {wrong[:4].tolist()}"


def test_attention_refuses_before_launching():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    einval, esize, f32, f16, bf16 = _lib.TIA_EINVAL, _lib.TIA_ESIZE, 0, 1, 2
    qkv = torch.randn((1, 4, 3 * 2 * 64), device="cuda")
    out = torch.full((1, 4, 128), 7.0, device="cuda")
    stream = _lib.current_stream()
    for args, code in (((qkv.data_ptr(), out.data_ptr(), 1, 4, 4, 32, 0.125, f32), esize),       # head_dim 32
                       ((qkv.data_ptr(), out.data_ptr(), 1, 4, 2, 64, 0.125, f16), einval),      # a half dtype code
                       ((qkv.data_ptr(), out.data_ptr(), 1, 4, 2, 64, 0.125, bf16), einval),
                       ((qkv.data_ptr(), out.data_ptr(), 1, 0, 2, 64, 0.125, f32), einval),      # s = 0
                       ((None, out.data_ptr(), 1, 4, 2, 64, 0.125, f32), einval),                # null pointers
                       ((qkv.data_ptr(), None, 1, 4, 2, 64, 0.125, f32), einval),
                       ((qkv.data_ptr() + 4, out.data_ptr(), 1, 4, 2, 64, 0.125, f32), einval),  # misaligned
                       ((qkv.data_ptr(), out.data_ptr() + 8, 1, 4, 2, 64, 0.125, f32), einval)):
        assert lib.tia_mha_fwd_f32(*args, stream) == code, args
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    assert lib.tia_mha_fwd_f32(qkv.data_ptr(), out.data_ptr(), 1, 4, 2, 64, 0.125, f32, stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# GELU, SwiGLU
# ------------------------------------------------------------------------------------------------------------------------------------
# What a result below float32's normal range may be off by, absolutely (stated as test_vit_foundation_kernels_gpu.py states it for
# its types): half of float32's subnormal step, 2^-150, for the rounding of the result itself, and in the SwiGLU as much again for
# the subnormal step of exp(-|t|) carried through t * e * x2 (2^-150 |t x2|).
TINY32 = 2.0 ** -150


def test_gelu_rows():
    """The half test's data (a grid over [-12, 12] and normal draws).  Allowance per element: twice the largest error of torch's
    float32 CPU GELU over the same values, plus one float32 unit of ``|ref|`` (+ the subnormal floor); finite everywhere; signed zeros
    kept."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_gelu_rows_f32_

    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.linspace(-12.0, 12.0, 24 * 512 + 8), torch.randn(197 * 1536, generator=g), torch.tensor([0.0, -0.0, 1e-40, -1e-40])])
    assert x.numel() % 4 == 0
    xd = x.double()
    ref = 0.5 * xd * torch.special.erfc(-xd / math.sqrt(2.0))  # = 0.5 x (1 + erf(x / sqrt 2)), without float64's own cancellation
    e_torch = float((F.gelu(x).double() - ref).abs().max())
    got32 = hip_gelu_rows_f32_(x.cuda().clone()).cpu()
    got = got32.double()
    assert bool(torch.isfinite(got).all())
    zeros = x == 0
    assert torch.equal(torch.signbit(got32[zeros]), torch.signbit(x[zeros])) and bool((got32[zeros] == 0).all())
    err = (got - ref).abs()
    bound = 2.0 * e_torch + U32 * ref.abs() + TINY32
    tail = xd < -3.0  # where 1 + erf cancels: the relative figure is recorded, not gated
    rel_tail = float((err[tail] / ref[tail].abs()).max())
    print(f"gelu f32: worst {float((err / bound).max()):.3f} of the bound; max |err| {float(err.max()):.3e} against torch's {e_torch:.3e}; "
          f"relative error for x < -3: {rel_tail:.3e}")
    assert bool((err <= bound).all())


def _swiglu_input(rows: int, hidden: int) -> torch.Tensor:
    """``[rows, 2 hidden]`` float32: normal gates (std 3) and values (std 2); the first gates (row-major) are the special ones and a
    grid over [-30, 30] (the half test's input)."""
    g = torch.Generator().manual_seed(rows * 7 + hidden)
    gate = torch.randn((rows, hidden), generator=g) * 3.0
    val = torch.randn((rows, hidden), generator=g) * 2.0
    count = rows * hidden
    special = torch.tensor(SPECIAL_GATES)[:count]
    grid = torch.linspace(-30.0, 30.0, max(min(count - special.numel(), 4801), 0))
    head = torch.cat([special, grid])
    gate.view(-1)[:head.numel()] = head
    return torch.cat([gate, val], dim=1)


@pytest.mark.parametrize(("rows", "hidden"), [(1, 12), (3, 256), (197, 1540)])
def test_swiglu_rows(rows, hidden):
    """Allowance per element: twice the largest error of torch's float32 CPU ``silu(gate) * value`` over the same values, plus one
    float32 unit of ``|ref|`` (+ the subnormal floor ``2^-150 (1 + |t x2|)``); finite everywhere, the overflowing gates included;
    nothing written outside ``rows * hidden`` elements."""
    from tiatoolbox_amd import _lib

    x = _swiglu_input(rows, hidden)
    gate, val = x[:, :hidden].double(), x[:, hidden:].double()
    ref = gate / (1.0 + torch.exp(-gate)) * val
    e_torch = float(((F.silu(x[:, :hidden]) * x[:, hidden:]).double() - ref).abs().max())
    guard = 64
    buf = torch.full((rows * hidden + 2 * guard,), float("nan"), device="cuda")
    y = buf[guard:guard + rows * hidden]
    rc = _lib.load().tia_swiglu_rows_f32(x.cuda().data_ptr(), y.data_ptr(), rows, hidden, _lib.current_stream())
    assert rc == 0
    got = y.cpu().reshape(rows, hidden).double()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + rows * hidden:]).all())
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    bound = 2.0 * e_torch + U32 * ref.abs() + TINY32 * (1.0 + (gate * val).abs())
    print(f"swiglu f32 {rows}x{hidden}: worst {float((err / bound).max()):.3f} of the bound; max |err| {float(err.max()):.3e} against "
          f"torch's {e_torch:.3e}")
    assert bool((err <= bound).all())


def test_swiglu_zero_lanes_and_refusals():
    """A zero gate and value (a pad lane of the graph) is an exact zero; sizes off the vector and null pointers are refused."""
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.vit_fused import hip_swiglu_rows_f32

    x = torch.randn((5, 48), generator=torch.Generator().manual_seed(1))
    x[:, 20:24] = 0.0
    x[:, 44:48] = 0.0
    got = hip_swiglu_rows_f32(x.cuda()).cpu()
    assert got.shape == (5, 24) and bool((got[:, 20:24] == 0).all())
    lib, stream = _lib.load(), _lib.current_stream()
    buf = torch.zeros(64, device="cuda")
    assert lib.tia_swiglu_rows_f32(buf.data_ptr(), buf.data_ptr(), 1, 6, stream) == _lib.TIA_ESIZE
    assert lib.tia_swiglu_rows_f32(None, buf.data_ptr(), 1, 8, stream) == _lib.TIA_EINVAL
    assert lib.tia_gelu_rows_f32(buf.data_ptr(), 6, stream) == _lib.TIA_ESIZE
    assert lib.tia_gelu_rows_f32(buf.data_ptr() + 4, 8, stream) == _lib.TIA_EINVAL
    assert lib.tia_gelu_rows_f32(None, 8, stream) == _lib.TIA_EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------------
# patchify, token assembly: bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("h", "w", "p", "k_pad"), [(32, 48, 16, 768), (28, 42, 14, 608), (224, 224, 14, 608), (16, 8, 8, 192), (16, 8, 8, 208)])
def test_patchify_is_a_pure_gather(h, w, p, k_pad):
    """Non-square grids, patch 16 / 14 / 8, ``k_pad`` equal to and above ``3 p^2``; NaN guard bands around the output.  The batch is a
    slice that starts one float into its buffer: the image needs 4-byte alignment only."""
    from tiatoolbox_amd import _lib

    rng = np.random.default_rng(h + w + k_pad)
    n, gh, gw = 3, h // p, w // p
    img = rng.standard_normal((n, h, w, 3)).astype(np.float32)
    cols = img.reshape(n, gh, p, gw, p, 3).transpose(0, 1, 3, 2, 4, 5).reshape(n, gh * gw, p * p * 3)  # [b, (gy, gx), (ky, kx, c)]
    exp = np.zeros((n, gh * gw, k_pad), np.float32)
    exp[:, :, :3 * p * p] = cols
    guard, count = 64, n * gh * gw * k_pad
    buf = torch.full((count + 2 * guard,), float("nan"), device="cuda")
    out = buf[guard:guard + count]
    src = torch.zeros(img.size + 1, device="cuda")
    src[1:] = torch.from_numpy(img).cuda().reshape(-1)
    assert src[1:].data_ptr() % 16 == 4  # noqa: PLR2004
    rc = _lib.load().tia_vit_patchify_f32(src[1:].data_ptr(), out.data_ptr(), n, h, w, p, k_pad, _lib.current_stream())
    assert rc == 0
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + count:]).all())
    assert np.array_equal(out.cpu().numpy().reshape(exp.shape).view(np.uint32), exp.view(np.uint32))


def test_patchify_refusals():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    img, tok = torch.zeros((1, 28, 28, 3), device="cuda"), torch.zeros((4, 608), device="cuda")
    assert lib.tia_vit_patchify_f32(img.data_ptr(), tok.data_ptr(), 1, 28, 28, 14, 588, stream) == _lib.TIA_ESIZE   # k_pad % 16
    assert lib.tia_vit_patchify_f32(img.data_ptr(), tok.data_ptr(), 1, 28, 28, 14, 576, stream) == _lib.TIA_ESIZE   # k_pad < 3 p^2
    assert lib.tia_vit_patchify_f32(img.data_ptr(), tok.data_ptr(), 1, 28, 30, 14, 608, stream) == _lib.TIA_ESIZE   # w % patch
    assert lib.tia_vit_patchify_f32(None, tok.data_ptr(), 1, 28, 28, 14, 608, stream) == _lib.TIA_EINVAL
    assert lib.tia_vit_patchify_f32(img.data_ptr(), tok.data_ptr() + 4, 1, 28, 28, 14, 608, stream) == _lib.TIA_EINVAL  # rows: 16 bytes
    assert lib.tia_vit_patchify_f32(img.data_ptr() + 2, tok.data_ptr(), 1, 28, 28, 14, 608, stream) == _lib.TIA_EINVAL  # image: 4 bytes
    assert lib.tia_vit_patchify_f32(img.data_ptr(), tok.data_ptr(), 1, 28, 28, 14, 608, stream) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["plain", "registers-no-class-entry", "host-folded-prefix"])
def test_assembly_is_one_float32_add(form):
    """The three prefix forms against the CPU's gather and single float32 add, bit for bit (random float32 values: a second add or
    another order would show)."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_assemble_f32

    rng = np.random.default_rng(len(form))
    n, g, d = 3, 7, 68  # 17 vectors of 4: no multiple of the wave
    nreg, has_cls = {"plain": (0, True), "registers-no-class-entry": (4, False), "host-folded-prefix": (3, False)}[form]
    tok = rng.standard_normal((n, g, d)).astype(np.float32)
    cls = rng.standard_normal(d).astype(np.float32)
    reg = rng.standard_normal((nreg, d)).astype(np.float32) if nreg else None
    pos = rng.standard_normal((g + int(has_cls), d)).astype(np.float32)
    rows = [np.broadcast_to(cls + pos[0] if has_cls else cls, (n, 1, d))]
    if nreg:
        rows.append(np.broadcast_to(reg, (n, nreg, d)))
    rows.append(tok + pos[int(has_cls):][None])
    want = np.concatenate(rows, axis=1).astype(np.float32)
    got = hip_vit_assemble_f32(torch.from_numpy(tok).cuda(), torch.from_numpy(cls).cuda(), None if reg is None else torch.from_numpy(reg).cuda(),
                               torch.from_numpy(pos).cuda(), pos_has_cls=has_cls)
    assert got.shape == (n, 1 + nreg + g, d) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------------
# the Linear on the split kernel at token shapes
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("n", "s", "cin", "cout"), [(2, 5, 128, 384), (2, 197, 384, 1536)])
def test_linear_on_the_split_kernel(n, s, cin, cout):
    """``tia_conv2d_bf16x3_nhwc_f32`` with a 1x1 window on ``[n, S, 1, cin]`` tokens, bias + residual fused:
    ``max |y - float64| <= 1e-5 max |y|`` (the gate of ``test_conv_split_gpu.py``); the float32 kernel's error on the same tensors
    is printed beside it."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_linear_f32, pack_linear_weights_f32, pack_linear_weights_split

    g = torch.Generator().manual_seed(cin + s)
    x = torch.randn((n, s, cin), generator=g)
    w = torch.randn((cout, cin), generator=g) / cin ** 0.5
    b, res = torch.randn(cout, generator=g), torch.randn((n, s, cout), generator=g)
    ref = x.double() @ w.double().T + b.double() + res.double()
    w3 = pack_linear_weights_split(w.cuda())
    assert w3 is not None and w3.dtype == torch.bfloat16
    got = hip_linear_f32(x.cuda(), w3, b.cuda(), res.cuda(), cout=cout)
    assert got.shape == (n, s, cout) and got.dtype == torch.float32
    e_split = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
    got32 = hip_linear_f32(x.cuda(), pack_linear_weights_f32(w.cuda()), b.cuda(), res.cuda(), cout=cout)
    e_f32 = float((got32.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"linear f32 {n}x{s}x{cin} -> {cout}: split kernel {e_split:.2e}; float32 kernel {e_f32:.2e}")
    assert e_split <= 1e-5 and e_f32 <= 1e-5
    plain = hip_linear_f32(x.cuda(), w3, None, None, cout=cout)  # the epilogue's parts are optional
    assert float((plain.cpu().double() - x.double() @ w.double().T).abs().max() / ref.abs().max()) <= 1e-5


def test_linear_integer_case_is_exact():
    """Integer tokens, weights, bias and residual with ``sum |a| |w| < 2^24``: every product and partial sum is an integer float32
    holds, so both kernels must return the integer result bit for bit, in any summation order."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_linear_f32, pack_linear_weights_f32, pack_linear_weights_split

    n, s, cin, cout = 2, 67, 256, 256
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-60, 61, (n, s, cin), generator=g).float()
    w = torch.randint(-100, 101, (cout, cin), generator=g).float()
    b, res = torch.randint(-1000, 1001, (cout,), generator=g).float(), torch.randint(-1000, 1001, (n, s, cout), generator=g).float()
    assert float((x.abs().double() @ w.abs().double().T).max()) + 2000 < 2 ** 24
    ref = (x.double() @ w.double().T + b.double() + res.double()).float()
    for pack in (pack_linear_weights_split, pack_linear_weights_f32):
        got = hip_linear_f32(x.cuda(), pack(w.cuda()), b.cuda(), res.cuda(), cout=cout).cpu()
        assert torch.equal(got, ref), pack.__name__

"""The three streaming kernels the foundation models add (``csrc/vit_rows.hip``: packed SwiGLU, the padded patch im2col, token assembly
with register tokens) against float64 / exact references computed on the CPU from exactly the half values the kernels are given, in
fp16 and bf16; and the entry points' refusals."""

from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
ROUND = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}  # the one rounding to half: half a unit in the last place, relative
# What a result below the normal range may be off by, absolutely.  fp16: half its subnormal step, 2^-25.  bf16 shares float32's
# exponent range, so the same effect sits at the bottom of float32: half of bf16's subnormal step (2^-134) for the rounding, and as
# much again for float32's own subnormal step in exp(-|t|) (2^-150 |t x2| <= 2^-134 for every |t x2| <= 2^16 used here): 2^-133.
# Without it NO float32 kernel meets a relative bound for a gate of -100, where silu(t) x2 = 3.7e-42 x2 is below bf16's smallest
# subnormal (9.2e-41) and the correctly rounded result is 0.
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -133}
# gates at which exp(-t) overflows in float32 (t < -88.72), their mirror images, and signed zeros; every one is a bf16 and fp16 value
SPECIAL_GATES = [-100.0, -89.0, -0.0, 0.0, 30.0, -30.0, 100.0, 89.0, -96.0, -88.0, -90.0, 88.0]


def _lib():
    from tiatoolbox_amd import _lib as lib

    return lib


def _dt(dtype: torch.dtype) -> int:
    from tiatoolbox_amd.models.architecture.fused import _DT

    return _DT[dtype]


# ------------------------------------------------------------------------------------------------------------------------------------
# packed SwiGLU
# ------------------------------------------------------------------------------------------------------------------------------------
def _swiglu_input(rows: int, hidden: int, dtype: torch.dtype) -> torch.Tensor:
    """``[rows, 2 hidden]`` of ``dtype``: normal gates (std 3) and values (std 2); the first gates (row-major) are the special ones and
    a grid over [-30, 30]."""
    g = torch.Generator().manual_seed(rows * 7 + hidden)
    gate = torch.randn((rows, hidden), generator=g) * 3.0
    val = torch.randn((rows, hidden), generator=g) * 2.0
    count = rows * hidden
    special = torch.tensor(SPECIAL_GATES)[:count]
    grid = torch.linspace(-30.0, 30.0, max(min(count - special.numel(), 4801), 0))
    head = torch.cat([special, grid])
    gate.view(-1)[:head.numel()] = head
    return torch.cat([gate, val], dim=1).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize(("rows", "hidden"), [(1, 8), (3, 256), (394, 4096)])
def test_swiglu_rows(rows, hidden, dtype):
    """``|got - ref| <= u |ref| + 2^-20 |ref|`` (+ the absolute term of ``TINY`` below the normal range): ``u |ref|`` is the one rounding
    to half, ``2^-20 |ref|`` under 16 float32 units for exp, add, divide and multiply; finite everywhere, the overflowing gates
    included; nothing written outside ``rows * hidden`` elements."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_swiglu_rows_h

    x = _swiglu_input(rows, hidden, dtype)
    assert x.shape == (rows, 2 * hidden)
    gate, val = x[:, :hidden].double(), x[:, hidden:].double()
    assert float(gate.min()) == -100.0 and bool((gate == 0).any())  # noqa: PLR2004
    ref = gate / (1.0 + torch.exp(-gate)) * val
    assert bool(torch.isfinite(ref).all())
    # through the wrapper ...
    got = hip_swiglu_rows_h(x.cuda().reshape(1, rows, 2 * hidden))
    assert got.shape == (1, rows, hidden) and got.dtype == dtype
    # ... and through the entry point itself into the middle of a guarded buffer
    lib, guard = _lib(), 64
    buf = torch.full((guard + rows * hidden + guard,), 1234.0, dtype=dtype, device="cuda")
    xd = x.cuda()
    rc = lib.load().tia_swiglu_rows_h(xd.data_ptr(), buf.data_ptr() + 2 * guard, rows, hidden, _dt(dtype), lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 1234.0).all()) and bool((buf[guard + rows * hidden:] == 1234.0).all())  # noqa: PLR2004
    assert torch.equal(buf[guard:guard + rows * hidden].view(torch.int16), got.reshape(-1).view(torch.int16))
    got = got.cpu().double().reshape(rows, hidden)
    assert bool(torch.isfinite(got).all())
    bound = ROUND[dtype] * ref.abs() + 2.0 ** -20 * ref.abs() + TINY[dtype]
    worst = float(((got - ref).abs() / bound).max())
    print(f"swiglu rows={rows} H={hidden} {dtype}: {worst:.3f} of the bound")
    assert worst <= 1.0
    # a gate that overflows exp(-t) gives a zero or the tiny product, never a NaN or an inf; a huge positive gate is the identity
    sel = gate <= -88.0  # noqa: PLR2004
    assert bool((got[sel].abs() <= 1e-30).all())
    sel = gate >= 88.0  # noqa: PLR2004
    assert torch.equal(got[sel], (gate[sel] * val[sel]).to(dtype).double())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_swiglu_zero_gates_give_exact_zeros(dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_swiglu_rows_h

    rows, hidden = 5, 24
    rng = np.random.default_rng(5)
    gate = np.where(rng.integers(0, 2, (rows, hidden)) == 1, 0.0, -0.0).astype(np.float32)
    val = rng.integers(-200, 201, (rows, hidden)).astype(np.float32)
    x = torch.from_numpy(np.concatenate([gate, val], axis=1)).to(dtype)
    got = hip_swiglu_rows_h(x.cuda())
    assert got.shape == (rows, hidden) and bool((got == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# padded patch im2col
# ------------------------------------------------------------------------------------------------------------------------------------
def _patchify_pad(src: torch.Tensor, patch: int, k_pad: int, dtype: torch.dtype) -> torch.Tensor:
    """The entry point into a buffer pre-filled with NaN: every element of it has to be written."""
    lib = _lib()
    n, h, w, _ = src.shape
    out = torch.full((n, (h // patch) * (w // patch), k_pad), float("nan"), dtype=dtype, device="cuda")
    rc = lib.load().tia_vit_patchify_pad_h(src.data_ptr(), _dt(src.dtype), out.data_ptr(), n, h, w, patch, k_pad, _dt(dtype), lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize(("h", "w", "p", "k_pad"), [(28, 42, 14, 608), (14, 14, 14, 608), (32, 48, 16, 768), (32, 48, 16, 800)])
@pytest.mark.parametrize("n", [1, 3])
def test_padded_patchify_is_exact(n, h, w, p, k_pad, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_patchify_h, hip_vit_patchify_pad_h

    img = torch.from_numpy(np.random.default_rng(h + w + n).integers(0, 256, (n, h, w, 3)).astype(np.float32))  # exact in both half types
    g, k = (h // p) * (w // p), 3 * p * p
    cols = F.unfold(img.permute(0, 3, 1, 2), kernel_size=p, stride=p)  # [n, (c, ky, kx), g]
    exp = cols.reshape(n, 3, p, p, g).permute(0, 4, 2, 3, 1).reshape(n, g, k)  # [n, g, (ky, kx, c)]
    exp = torch.cat([exp, torch.zeros(n, g, k_pad - k)], dim=2)
    for src in (img, img.to(dtype)):  # the float32 batch, and the batch already in the run's type
        tok = _patchify_pad(src.cuda(), p, k_pad, dtype)
        assert tok.dtype == dtype and torch.equal(tok.cpu().float(), exp)  # (no NaN left: equal to finite values)
        assert bool((tok[:, :, k:].view(torch.int16) == 0).all())  # +0, bit for bit
        assert torch.equal(hip_vit_patchify_pad_h(src.cuda(), p, k_pad, dtype).view(torch.int16), tok.view(torch.int16))
        if p % 8 == 0 and k_pad == k:
            assert torch.equal(tok.view(torch.int16), hip_vit_patchify_h(src.cuda(), p, dtype).view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------------------
# token assembly with register tokens
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_prefix_assembly_is_exact(dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_assemble_prefix_h, hip_vit_assemble_tokens_h

    rng = np.random.default_rng(17)
    for nreg, has_cls, g, d, n in itertools.product((0, 4, 8), (0, 1), (1, 6), (8, 128), (1, 3)):
        draw = lambda *shape: torch.from_numpy(rng.integers(-64, 65, shape).astype(np.float32))  # noqa: E731
        tokens, cls, reg, pos = draw(n, g, d), draw(d), draw(nreg, d), draw(g + has_cls, d)
        rows = [(cls + pos[0] if has_cls else cls).expand(n, 1, d), reg.expand(n, nreg, d), tokens + pos[has_cls:]]
        want = torch.cat(rows, dim=1)  # |sum| <= 128: exact in both half types
        got = hip_vit_assemble_prefix_h(tokens.to(dtype).cuda(), cls.cuda(), reg.cuda() if nreg else None, pos.cuda(), pos_has_cls=bool(has_cls))
        assert got.shape == (n, 1 + nreg + g, d) and got.dtype == dtype, (nreg, has_cls, g, d, n)
        assert torch.equal(got.cpu().float(), want), (nreg, has_cls, g, d, n)
        if nreg == 0 and has_cls:
            old = hip_vit_assemble_tokens_h(tokens.to(dtype).cuda(), cls.cuda(), pos.cuda())
            assert torch.equal(old.view(torch.int16), got.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_prefix_assembly_rounds_once_like_the_plain_kernel(dtype):
    """Non-integer values: ``R = 0, pos_has_cls = 1`` is ``tia_vit_assemble_tokens_h`` bit for bit, and with registers every row is the
    float32 sum rounded once."""
    from tiatoolbox_amd.models.architecture.vit_fused import hip_vit_assemble_prefix_h, hip_vit_assemble_tokens_h

    g = torch.Generator().manual_seed(3)
    n, grid, d, nreg = 2, 7, 136, 4
    tokens = torch.randn((n, grid, d), generator=g).to(dtype)
    cls, reg = torch.randn(d, generator=g), torch.randn((nreg, d), generator=g)
    pos = torch.randn((1 + grid, d), generator=g)
    new = hip_vit_assemble_prefix_h(tokens.cuda(), cls.cuda(), None, pos.cuda(), pos_has_cls=True)
    old = hip_vit_assemble_tokens_h(tokens.cuda(), cls.cuda(), pos.cuda())
    assert torch.equal(new.view(torch.int16), old.view(torch.int16))
    got = hip_vit_assemble_prefix_h(tokens.cuda(), cls.cuda(), reg.cuda(), pos[1:].contiguous().cuda(), pos_has_cls=False).cpu()
    want = torch.cat([cls.expand(n, 1, d), reg.expand(n, nreg, d), tokens.float() + pos[1:]], dim=1).to(dtype)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_launching():
    lib_mod = _lib()
    lib, stream = lib_mod.load(), lib_mod.current_stream()
    einval, esize, f32, f16, bf16 = lib_mod.TIA_EINVAL, lib_mod.TIA_ESIZE, 0, 1, 2
    # --- tia_swiglu_rows_h
    x = torch.randn((2, 32), device="cuda").half()
    y = torch.full((2, 16), 7.0, device="cuda", dtype=torch.float16)
    for args, code in (((x.data_ptr(), y.data_ptr(), 2, 16, f32), einval),           # a float32 dtype code
                       ((None, y.data_ptr(), 2, 16, f16), einval),                    # null pointers
                       ((x.data_ptr(), None, 2, 16, f16), einval),
                       ((x.data_ptr() + 2, y.data_ptr(), 2, 16, f16), einval),        # misaligned
                       ((x.data_ptr(), y.data_ptr() + 8, 2, 16, f16), einval),
                       ((x.data_ptr(), y.data_ptr(), 0, 16, f16), einval),            # no rows
                       ((x.data_ptr(), y.data_ptr(), 2, -8, f16), einval),
                       ((x.data_ptr(), y.data_ptr(), 2, 12, f16), esize)):            # H % 8
        assert lib.tia_swiglu_rows_h(*args, stream) == code, args
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())  # noqa: PLR2004  (nothing was launched)
    assert lib.tia_swiglu_rows_h(x.data_ptr(), y.data_ptr(), 2, 16, f16, stream) == 0
    # --- tia_vit_patchify_pad_h
    img = torch.zeros((1, 28, 28, 3), device="cuda")
    tok = torch.full((1, 4, 608), 7.0, device="cuda", dtype=torch.float16)
    ok = (img.data_ptr(), f32, tok.data_ptr(), 1, 28, 28, 14, 608, f16)

    def patchify(**over):
        names = ("x", "x_dtype", "tokens", "n", "h", "w", "patch", "k_pad", "dtype")
        return lib.tia_vit_patchify_pad_h(*[over.get(k, v) for k, v in zip(names, ok)], stream)

    assert patchify(dtype=f32) == einval and patchify(x_dtype=bf16) == einval  # a float32 output; bf16 input beside fp16 tokens
    assert patchify(x=None) == einval and patchify(tokens=None) == einval
    assert patchify(x=img.data_ptr() + 4) == einval and patchify(tokens=tok.data_ptr() + 2) == einval
    assert patchify(n=0) == einval and patchify(patch=0) == einval and patchify(k_pad=0) == einval
    assert patchify(k_pad=600) == esize   # k_pad % 32
    assert patchify(k_pad=576) == esize   # k_pad < 3 p^2 = 588
    assert patchify(h=30) == esize and patchify(w=21) == esize  # h % patch, w % patch
    torch.cuda.synchronize()
    assert bool((tok == 7.0).all())  # noqa: PLR2004
    assert patchify() == 0
    # --- tia_vit_assemble_prefix_h
    d, g, nreg = 16, 2, 4
    tokens = torch.zeros((1, g, d), device="cuda", dtype=torch.float16)
    cls, reg, pos = torch.zeros(d, device="cuda"), torch.zeros((nreg, d), device="cuda"), torch.zeros((g + 1, d), device="cuda")
    out = torch.full((1, 1 + nreg + g, d), 7.0, device="cuda", dtype=torch.float16)
    ok = (tokens.data_ptr(), cls.data_ptr(), reg.data_ptr(), pos.data_ptr(), 1, out.data_ptr(), 1, g, nreg, d, f16)

    def assemble(**over):
        names = ("tokens", "cls", "reg", "pos", "has_cls", "out", "n", "g", "nreg", "d", "dtype")
        return lib.tia_vit_assemble_prefix_h(*[over.get(k, v) for k, v in zip(names, ok)], stream)

    assert assemble(dtype=f32) == einval
    for name in ("tokens", "cls", "reg", "pos", "out"):
        assert assemble(**{name: None}) == einval, name            # null (reg: null beside R > 0)
        assert assemble(**{name: ok[("tokens", "cls", "reg", "pos", "has_cls", "out").index(name)] + 4}) == einval, name  # misaligned
    assert assemble(nreg=0) == einval                              # a register pointer beside R = 0
    assert assemble(has_cls=2) == einval and assemble(n=0) == einval and assemble(g=0) == einval and assemble(nreg=-1) == einval
    assert assemble(d=12) == esize                                 # d % 8
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # noqa: PLR2004
    assert assemble() == 0 and assemble(reg=None, nreg=0) == 0
    torch.cuda.synchronize()

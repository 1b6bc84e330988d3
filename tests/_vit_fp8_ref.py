"""Host-side references of the FP8 Vision Transformer tests, in float64: the e4m3fn value table, the scaled GEMM, the three
quantising producers' float32 values, the bound on a quantised element, and the yardstick of the graph tests -- the torch module in
bfloat16 with the inputs and weights of ``qkv`` / ``fc1`` / ``fc2`` fake-quantised by the recipe."""

from __future__ import annotations

import math

import torch

HALF_EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}  # tests/_conv_ref.py's gate of the half GEMM: eps |ref| + 1e-4 max |ref|
E4M3_MAX = 448.0
# code -> value: torch's own decoding of the 256 bytes (0x7f / 0xff are NaN)
E4M3_VALUES = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float64)
FINITE_CODES = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)  # noqa: PLR2004


def decode(codes: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3fn codes -> float64 values."""
    return E4M3_VALUES[codes.cpu().long()]


def encode_exact(values: torch.Tensor) -> torch.Tensor:
    """Values that ARE e4m3 numbers -> their codes (checked: the round trip is the identity)."""
    codes = values.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(decode(codes), values.double()), "not representable in e4m3"
    return codes


def e4m3_tie_rows(rows: int = 16) -> torch.Tensor:
    """Float32 ``[rows, 768]`` whose maximum is exactly 448 in every row (the recipe's ``inv = s = 1``: the codes are the conversion of
    the values themselves) and whose other entries are EVERY midpoint between adjacent finite e4m3 magnitudes -- the 7 subnormal
    steps from 0 on, the step across 2^-6, up to the one between 416 and 448 -- each with its two float32 neighbours, in both signs:
    126 x 3 x 2 = 756 values, the 448 in front, zeros up to K = 6 x 128.  Row ``r`` is row 0 rotated by ``37 r`` places (behind the
    448), so that every tie meets many lanes of a packing kernel."""
    mags = decode(FINITE_CODES[:127]).to(torch.float32)  # 0, 2^-9, ..., 448 in rising order
    assert float(mags[0]) == 0.0 and float(mags[-1]) == E4M3_MAX and bool((mags[1:] > mags[:-1]).all())
    mid = (mags[:-1] + mags[1:]) / 2  # exact in float32: one more significant bit
    assert torch.equal(mid.double(), (mags[:-1].double() + mags[1:].double()) / 2)
    inf = torch.full_like(mid, float("inf"))
    body = torch.stack([torch.nextafter(mid, -inf), mid, torch.nextafter(mid, inf)], dim=1).reshape(-1)
    body = torch.cat([body, -body, torch.zeros(767 - 2 * body.numel())])
    return torch.stack([torch.cat([torch.tensor([E4M3_MAX]), torch.roll(body, 37 * r)]) for r in range(rows)])


def gemm_ref64(a: torch.Tensor, sa: torch.Tensor, w: torch.Tensor, sw: torch.Tensor, bias: torch.Tensor | None,
               residual: torch.Tensor | None) -> torch.Tensor:
    """``(sum_k qa qw) sa sw + bias (+ residual)`` in float64 from codes ``a [rows, K]`` / ``w [N, K]`` and float32 scales."""
    y = (decode(a) @ decode(w).T) * sa.double().cpu()[:, None] * sw.double().cpu()[None, :]
    if bias is not None:
        y = y + bias.double().cpu()
    if residual is not None:
        y = y + residual.cpu().double()
    return y


def ulp_e4m3(mag: torch.Tensor) -> torch.Tensor:
    """The spacing of e4m3 codes at magnitude ``mag`` (float64, <= 448 (1 + eps)): 2^-9 below the smallest normal 2^-6, else
    ``2^(floor(log2 mag) - 3)``."""
    e = torch.floor(torch.log2(mag.clamp_min(2.0 ** -6))).clamp_max(8.0)
    return torch.where(mag < 2.0 ** -6, torch.full_like(mag, 2.0 ** -9), torch.exp2(e - 3.0))


SCALE_ULPS = 4.0  # how many float32 ulp a producer's scale may be off ``amax64 / 448``


def quantised_rows_ratios(y64: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The figures of :func:`check_quantised_rows` for rows whose float64 values are ``y64 [rows, K]``: per row, how many float32 ulp
    the scale is off ``amax64 / 448`` (1 for an all-zero row); the dequantised values ``s q`` (a NaN code stays a NaN); and per
    element ``|s q - y64|`` over its bound ``(ulp_e4m3(|y64| / s) / 2 * s) (1 + 2^-10) + 2^-10 s``."""
    s = scales.cpu().double().reshape(-1)
    amax = y64.abs().amax(dim=1)
    want = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    ulp32 = torch.exp2(torch.floor(torch.log2(want)) - 23.0)
    deq = decode(codes).reshape(y64.shape) * s[:, None]
    bound = (0.5 * ulp_e4m3(y64.abs() / s[:, None]) * s[:, None]) * (1.0 + 2.0 ** -10) + 2.0 ** -10 * s[:, None]
    return (s - want).abs() / ulp32, deq, (deq - y64).abs() / bound


def check_quantised_rows(y64: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, what: str) -> None:
    """The producers' pass condition for rows whose float64 values are ``y64 [rows, K]``: the scale within 4 float32 ulp of
    ``amax64 / 448`` (1 for an all-zero row), and EVERY element ``|s q - y64| <= (ulp_e4m3(|y64| / s) / 2 * s) (1 + 2^-10) + 2^-10 s`` --
    half a code step (half the subnormal step at the bottom) plus room for the float32 evaluation of ``y``."""
    ds, deq, ratio = quantised_rows_ratios(y64, codes, scales)
    ds, worst = ds.max(), ratio.max()
    assert bool(torch.isfinite(deq).all()), f"{what}: a NaN code"
    print(f"{what}: scale off by {float(ds):.2f} float32 ulp, worst element {float(worst):.3f} of its bound")
    assert float(ds) <= SCALE_ULPS, (what, float(ds))
    assert float(worst) <= 1.0, (what, float(worst))


def layernorm64(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    x = x.cpu().double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.cpu().double() + beta.cpu().double()


def gelu64(x: torch.Tensor) -> torch.Tensor:
    x = x.cpu().double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def swiglu64(x: torch.Tensor) -> torch.Tensor:
    gate, value = x.cpu().double().chunk(2, -1)
    return gate / (1.0 + torch.exp(-gate)) * value


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def fake_quantise(v: torch.Tensor) -> torch.Tensor:
    """Quantise the rows of ``v`` by the recipe and dequantise: float32 in, float32 out (the conversion is torch's CPU one)."""
    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_e4m3

    q, s = quantize_rows_e4m3(v.detach().float().cpu())
    return (q.float() * s[..., None]).to(v.device)


def fake_quantised_module(module: torch.nn.Module, dtype: torch.dtype = torch.bfloat16) -> torch.nn.Module:
    """``module`` (float32, on its device; changed in place) as the FP8 graph's yardstick: the weights of every block's ``attn.qkv`` /
    ``mlp.fc1`` / ``mlp.fc2`` fake-quantised per output channel in float32, the module cast to ``dtype``, and a forward pre-hook on
    those three layers that fake-quantises their input per token."""
    targets = [m for name, m in module.named_modules()
               if isinstance(m, torch.nn.Linear) and name.rsplit(".", 2)[-2:] in (["attn", "qkv"], ["mlp", "fc1"], ["mlp", "fc2"])]
    assert targets, "no qkv / fc1 / fc2 layers found"
    with torch.no_grad():
        for lin in targets:
            lin.weight.copy_(fake_quantise(lin.weight))
    module = module.to(dtype)

    def hook(_mod, args):
        return (fake_quantise(args[0]).to(args[0].dtype), *args[1:])

    for lin in targets:
        lin.register_forward_pre_hook(hook)
    return module


def rel_error(got: torch.Tensor, ref: torch.Tensor) -> float:
    """``e = max |got - ref| / max(max |ref|, 1)`` (``tests/test_vit_gpu.py::_parity``)."""
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1.0)

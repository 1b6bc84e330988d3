"""Host-side references of the INT8 Vision Transformer tests: the GEMM from an int64 accumulation, the bound on a quantised element,
torch stand-ins of the INT8 wrappers (any device), and the yardstick of the graph tests -- the torch module in bfloat16 with the inputs
and weights of ``qkv`` / ``fc1`` / ``fc2`` fake-quantised by ``quantize_rows_int8``, built like ``_vit_fp8_ref.fake_quantised_module``."""

from __future__ import annotations

import torch

from _vit_fp8_ref import HALF_EPS, SCALE_ULPS, gelu64, layernorm64, rel_error, swiglu64  # noqa: F401  (shared with the test files)

I8_MAX = 127.0


def acc64(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``sum_k qa[r,k] qw[o,k]`` of int8 codes ``a [rows, K]`` / ``w [N, K]`` as int64, exactly: every partial sum of the float64
    product is an integer below ``K 127^2 < 2^53``."""
    assert a.dtype == torch.int8 and w.dtype == torch.int8
    return (a.cpu().double() @ w.cpu().double().T).long()


def gemm_ref32(a, sa, w, sw, bias, residual) -> torch.Tensor:
    """The contract's float32 statement step by step: ``float(acc)`` (the int64 sum converted with round to nearest even), times
    ``sa``, times ``sw``, plus ``bias``, plus ``float32(residual)`` -- each a float32 operation.  With power-of-two scales the two
    products are exact, so whether the device fuses them into the following addition does not show; the caller rounds to half."""
    acc = acc64(a, w)
    assert int(acc.abs().max()) < 2 ** 31
    y = acc.to(torch.float32) * sa.float().cpu()[:, None] * sw.float().cpu()[None, :]
    if bias is not None:
        y = y + bias.float().cpu()
    if residual is not None:
        y = y + residual.float().cpu()
    return y


def gemm_ref64(a, sa, w, sw, bias, residual) -> torch.Tensor:
    """``acc sa sw + bias (+ residual)`` in float64 from the int64 accumulation and the float32 scales."""
    y = acc64(a, w).double() * sa.double().cpu()[:, None] * sw.double().cpu()[None, :]
    if bias is not None:
        y = y + bias.double().cpu()
    if residual is not None:
        y = y + residual.cpu().double()
    return y


def quantised_rows_figures(y64: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> tuple[float, float]:
    """Per row, how many float32 ulp the scale is off ``amax64 / 127`` (1 for an all-zero row); per element ``|s q - y64|`` over its
    bound ``(s / 2) (1 + 2^-10) + 2^-10 s`` -- half a code step plus room for the float32 evaluation of ``y``.  The two maxima."""
    s = scales.cpu().double().reshape(-1)
    q = codes.cpu().reshape(y64.shape)
    assert q.dtype == torch.int8 and int(q.min()) >= -127, "a code outside [-127, 127]"  # noqa: PLR2004
    amax = y64.abs().amax(dim=1)
    want = torch.where(amax > 0, amax / I8_MAX, torch.ones_like(amax))
    ulp32 = torch.exp2(torch.floor(torch.log2(want)) - 23.0)
    bound = (0.5 * s[:, None]) * (1.0 + 2.0 ** -10) + 2.0 ** -10 * s[:, None]
    return float(((s - want).abs() / ulp32).max()), float(((q.double() * s[:, None] - y64).abs() / bound).max())


def check_quantised_rows(y64: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, what: str) -> None:
    ds, worst = quantised_rows_figures(y64, codes, scales)
    print(f"{what}: scale off by {ds:.2f} float32 ulp, worst element {worst:.3f} of its bound")
    assert ds <= SCALE_ULPS, (what, ds)
    assert worst <= 1.0, (what, worst)


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def fake_quantise(v: torch.Tensor) -> torch.Tensor:
    """Quantise the rows of ``v`` by the recipe and dequantise: float32 in, float32 out."""
    from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_int8

    q, s = quantize_rows_int8(v.detach().float().cpu())
    return (q.float() * s[..., None]).to(v.device)


def fake_quantised_module(module: torch.nn.Module, dtype: torch.dtype = torch.bfloat16, layers=("qkv", "fc1", "fc2")) -> torch.nn.Module:
    """``module`` (float32, on its device; changed in place) as the INT8 graph's yardstick: the weights of every block's ``attn.qkv`` /
    ``mlp.fc1`` / ``mlp.fc2`` (those named in ``layers``) fake-quantised per output channel in float32, the module cast to ``dtype``,
    and a forward pre-hook on those layers that fake-quantises their input per token."""
    pairs = [[{"qkv": "attn", "fc1": "mlp", "fc2": "mlp"}[name], name] for name in layers]
    targets = [m for name, m in module.named_modules() if isinstance(m, torch.nn.Linear) and name.rsplit(".", 2)[-2:] in pairs]
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


# ------------------------------------------------------------------------------------------------- torch stand-ins of the wrappers
def torch_int8_wrappers() -> dict:
    """Torch restatements of the INT8 wrappers ``FusedViT`` calls, for any device: name -> function.  The contract, not the kernels'
    code: producers make the float32 value from the half input and quantise it by ``quantize_rows_int8``; the GEMM accumulates the
    int8 codes exactly and refuses any other code dtype, as ``hip_linear_int8_rows`` does."""
    import torch.nn.functional as F  # noqa: N812

    from tiatoolbox_amd.models.architecture.vit_fused import QuantRows, quantize_rows_int8

    def rows(v):
        q, s = quantize_rows_int8(v)
        return QuantRows(q, s.reshape(-1))

    def serves(cout, cin):
        return cin % 128 == 0 and cout % 16 == 0 and cin <= 65536  # noqa: PLR2004

    def pack(weight):
        return rows(weight.detach().float())

    def layernorm(x, gamma, beta, *, eps):
        return rows(F.layer_norm(x.float(), (x.shape[-1],), gamma, beta, eps))

    def act(x, *, swiglu):
        if swiglu:
            gate, value = x.float().chunk(2, -1)
            return rows(F.silu(gate) * value)
        return rows(F.gelu(x.float()))

    def linear(a, w, bias, residual=None, *, dtype):
        if a.codes.dtype != torch.int8 or w.codes.dtype != torch.int8:
            msg = f"the INT8 GEMM takes torch.int8 codes; got {a.codes.dtype} beside {w.codes.dtype}."
            raise ValueError(msg)
        n, s, _ = a.codes.shape
        acc = (a.codes.reshape(n * s, -1).long() @ w.codes.long().T).float()
        y = acc * a.scales[:, None] * w.scales[None, :] + (bias if bias is not None else 0.0)
        y = y.reshape(n, s, -1)
        return (y + residual.float() if residual is not None else y).to(dtype)

    return {"linear_int8_serves": serves, "pack_linear_weights_int8": pack, "hip_layernorm_rows_qi8": layernorm, "hip_act_rows_qi8": act,
            "hip_linear_int8_rows": linear}

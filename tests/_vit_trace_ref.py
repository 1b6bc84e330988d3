"""Host-only helpers of the ``FusedViT`` stage-trace tests: a recorder of every wrapper call the graph makes, the sequence of calls a
model's configuration implies, and a checker that holds EVERY stage, at every element of every token, to a float64 reference built
from the bits that entered that stage and the torch module's own float32 ``state_dict()`` -- never from ``FusedViT``'s folded, padded
or packed attributes.  The gates are the ones each kernel's own test holds it to (imported, not restated); torch stand-ins of the FP8
wrappers complete ``_vit_classifier_ref.torch_vit_wrappers`` for runs without a GPU."""

from __future__ import annotations

import math
from typing import NamedTuple

import torch
import torch.nn.functional as F  # noqa: N812

from _vit_fp8_ref import HALF_EPS, SCALE_ULPS, gelu64, gemm_ref64, layernorm64, quantised_rows_ratios
from test_vit_foundation_kernels_gpu import ROUND as SWIGLU_ROUND
from test_vit_foundation_kernels_gpu import TINY as SWIGLU_TINY
from test_vit_kernels_gpu import UNIT

LN_EPS = 1e-6
TRACED = ("hip_vit_patchify_h", "hip_vit_patchify_pad_h", "hip_vit_patchify_norm_u8_h", "hip_linear_h", "hip_linear_fp8_rows",
          "hip_vit_assemble_tokens_h", "hip_vit_assemble_prefix_h", "hip_layernorm_rows_h", "hip_layernorm_rows_q8", "hip_mha_fwd_h",
          "hip_gelu_rows_h_", "hip_swiglu_rows_h", "hip_act_rows_q8", "hip_vit_cls_mean_pool_h")


# ------------------------------------------------------------------------------------------------------------------- the recorder
class Call(NamedTuple):
    """One wrapper call: ``args`` / ``kwargs`` / ``out`` with every tensor copied to the CPU (the arguments BEFORE the call, the result
    after it); ``live_args`` / ``live_out`` the objects themselves, for the checks of identity."""

    name: str
    args: tuple
    kwargs: dict
    out: object
    live_args: tuple
    live_out: object


def _to_cpu(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu() if v.is_cuda else v.detach().clone()
    if isinstance(v, tuple) and hasattr(v, "_fields"):  # QuantRows
        return type(v)(*[_to_cpu(t) for t in v])
    return v


def record(monkeypatch, module) -> list[Call]:
    """Wrap whatever function ``module`` (``vit_fused``) has under each name of ``TRACED`` -- the real wrappers, or stand-ins installed
    before -- and return the list the calls are appended to.  The wrapped function's result is returned untouched."""
    trace: list[Call] = []

    def recording(name, fn):
        def wrapper(*args, **kwargs):
            cpu_args, cpu_kwargs = tuple(_to_cpu(a) for a in args), {k: _to_cpu(v) for k, v in kwargs.items()}
            out = fn(*args, **kwargs)
            trace.append(Call(name, cpu_args, cpu_kwargs, _to_cpu(out), args, out))
            return out
        return wrapper

    for name in TRACED:
        monkeypatch.setattr(module, name, recording(name, getattr(module, name)))
    return trace


# ------------------------------------------------------------------------------------------- the FP8 wrappers in torch operations
def fp8_rule(cout: int, cin: int) -> bool:
    """``tia_linear_fp8_serves`` as documented: ``cin % 128 == 0 and cout % 16 == 0``."""
    return cin % 128 == 0 and cout % 16 == 0


def torch_fp8_wrappers(serves=fp8_rule) -> dict:
    """Torch restatements of the FP8 wrappers, for any device, in the manner of ``torch_vit_wrappers``: the recipe
    (``quantize_rows_e4m3``) for every quantisation, the exact sum of the code products, float32 scales / bias / residual, one
    rounding.  ``serves`` stands for ``linear_fp8_serves`` (the library does not load without a GPU build)."""
    from tiatoolbox_amd.models.architecture.vit_fused import QuantRows, quantize_rows_e4m3

    def quantise(y32):
        q, s = quantize_rows_e4m3(y32)
        return QuantRows(q.view(torch.uint8), s.reshape(-1).contiguous())

    def pack(weight):
        return quantise(weight.detach().to(torch.float32))

    def linear(a, w, bias, residual=None, *, dtype):
        acc = a.codes.view(torch.float8_e4m3fn).double() @ w.codes.view(torch.float8_e4m3fn).double().T  # exact
        y = acc.float() * a.scales.reshape(*a.codes.shape[:-1], 1) * w.scales
        if bias is not None:
            y = y + bias
        return (y + residual.float() if residual is not None else y).to(dtype)

    def layernorm(x, gamma, beta, *, eps):
        return quantise(F.layer_norm(x.float(), (x.shape[-1],), gamma, beta, eps))

    def act(x, *, swiglu):
        if swiglu:
            gate, value = x.float().chunk(2, -1)
            return quantise(F.silu(gate) * value)
        return quantise(F.gelu(x.float()))

    return {"pack_linear_weights_fp8": pack, "hip_linear_fp8_rows": linear, "hip_layernorm_rows_q8": layernorm, "hip_act_rows_q8": act,
            "linear_fp8_serves": serves}


# --------------------------------------------------------------------------------------------------------- the expected sequence
class Plan(NamedTuple):
    stages: list  # (place in the graph, wrapper name), in the order of the calls
    hidden: int   # the MLP's real width: fc2's inputs
    h_pad: int    # the width the graph carries per SwiGLU half (== hidden without padding, and for the GELU)
    fp8: dict     # "qkv" / "fc1" / "fc2" -> on the FP8 GEMM


def _up(v: int, m: int) -> int:
    return -(-v // m) * m


def plan_of(vit, *, uint8: bool = False, fp8: bool = False) -> Plan:
    """The calls ``FusedViT`` makes for ``vit``, from its configuration and the shapes of its state dict alone.  A packed SwiGLU half at
    or above 512 that is off the half GEMM's multiple of 32 is carried at the next one, and on the FP8 route at the next multiple of
    128 (the module docstring of ``vit_fused``); a Linear goes to the FP8 GEMM where ``fp8_rule`` takes the graph's shape."""
    sd = vit.state_dict()
    d, p = vit.embed_dim, vit.patch_size
    swiglu = vit.mlp_layer == "swiglu_packed"
    hidden = sd["blocks.0.mlp.fc2.weight"].shape[1]
    assert sd["blocks.0.mlp.fc1.weight"].shape[0] == (2 * hidden if swiglu else hidden)
    h_pad = hidden
    if swiglu and hidden >= 512 and hidden % 32 != 0:  # noqa: PLR2004
        h_pad = _up(hidden, 32)
    if swiglu and fp8 and h_pad >= 512 and h_pad % 128 != 0:  # noqa: PLR2004
        h_pad = _up(h_pad, 128)
    routes = {"qkv": fp8 and fp8_rule(3 * d, d), "fc1": fp8 and fp8_rule(2 * h_pad if swiglu else h_pad, d), "fc2": fp8 and fp8_rule(d, h_pad)}
    linear = lambda name: "hip_linear_fp8_rows" if routes[name] else "hip_linear_h"  # noqa: E731
    norm = lambda name: "hip_layernorm_rows_q8" if routes[name] else "hip_layernorm_rows_h"  # noqa: E731
    if uint8:
        first = "hip_vit_patchify_norm_u8_h"
    else:
        first = "hip_vit_patchify_h" if p % 8 == 0 else "hip_vit_patchify_pad_h"
    prefix = bool(vit.reg_tokens or vit.no_embed_class)
    stages = [("patchify", first), ("patch_embed.proj", "hip_linear_h"),
              ("tokens", "hip_vit_assemble_prefix_h" if prefix else "hip_vit_assemble_tokens_h")]
    act = "hip_act_rows_q8" if routes["fc2"] else ("hip_swiglu_rows_h" if swiglu else "hip_gelu_rows_h_")
    for i in range(len(vit.blocks)):
        b = f"blocks.{i}."
        stages += [(b + "norm1", norm("qkv")), (b + "qkv", linear("qkv")), (b + "attn", "hip_mha_fwd_h"), (b + "proj", "hip_linear_h"),
                   (b + "norm2", norm("fc1")), (b + "fc1", linear("fc1")), (b + "act", act), (b + "fc2", linear("fc2"))]
    stages.append(("norm_pool", "hip_vit_cls_mean_pool_h") if vit.global_pool == "token_mean" else ("norm", "hip_layernorm_rows_h"))
    return Plan(stages, hidden, h_pad, routes)


# ---------------------------------------------------------------------------------------------------------------------- the checker
class StageFailure(AssertionError):
    """A stage off its reference or its wiring; ``place`` is where it sits in the graph (``blocks.1.fc2``)."""

    def __init__(self, place: str, text: str) -> None:
        super().__init__(f"{place}: {text}")
        self.place = place


def _same(a, b) -> bool:
    return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def _folded(sd: dict, linear: str, gamma: str | None) -> tuple[torch.Tensor, torch.Tensor]:
    """Float32 ``(W, b)`` of ``linear`` with the LayerScale ``gamma`` folded as ``fold_layer_scale`` documents: ``gamma[:, None] * W`` and
    ``gamma * b``, one float32 rounding each."""
    w, b = sd[linear + ".weight"].float(), sd[linear + ".bias"].float()
    if gamma is not None and gamma in sd:
        g = sd[gamma].float()
        w, b = g[:, None] * w, g * b
    return w, b


class TraceChecker:
    """``check()`` walks a recorded ``trace`` of ``vit`` run in ``dtype`` on ``x`` (the batch as the graph's first kernel gets it:
    NHWC, float32 / ``dtype`` or uint8 with ``table32``, the hook's float32 ``[256, 3]`` table).  It fills ``rows`` with
    ``(place, wrapper, worst error as a multiple of the stage's gate)`` for every stage, ``failures`` with what broke a gate or the
    wiring, in the order of the graph, and raises the first of them."""

    def __init__(self, vit, trace: list[Call], x: torch.Tensor, dtype: torch.dtype, *, fp8: bool = False,
                 table32: torch.Tensor | None = None) -> None:
        self.vit, self.trace, self.x, self.dtype, self.table32 = vit, trace, x.cpu(), dtype, table32
        self.sd = {k: v.detach().cpu().float() for k, v in vit.state_dict().items()}
        self.plan = plan_of(vit, uint8=x.dtype == torch.uint8, fp8=fp8)
        self.d, self.heads, self.p, self.r = vit.embed_dim, vit.num_heads, vit.patch_size, vit.reg_tokens
        self.swiglu = vit.mlp_layer == "swiglu_packed"
        self.n, h, w = x.shape[0], x.shape[1], x.shape[2]
        self.grid = (h // self.p, w // self.p)
        self.s = 1 + self.r + self.grid[0] * self.grid[1]
        self.rows: list[tuple[str, str, float]] = []
        self.failures: list[StageFailure] = []

    # -- bookkeeping
    def fail(self, place: str, text: str) -> None:
        self.failures.append(StageFailure(place, text))

    def wired(self, place: str, ok: bool, text: str) -> None:
        if not ok:
            self.fail(place, "wiring: " + text)

    def gate(self, place: str, name: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> None:
        """Every element of ``got`` ``[image, token, channel]`` within ``bound`` of ``ref`` (a zero bound asks for equality, a NaN is the
        worst element)."""
        got, ref = got.double(), ref.double()
        err = (got - ref).abs()
        unequal = torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf))
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), unequal).nan_to_num(nan=math.inf)
        top = float(ratio.max())
        self.rows.append((place, name, top))
        if top > 1.0:
            idx = tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0])
            self.fail(place, f"{name}: worst element (image, token, channel) {idx}: got {float(got[idx])!r}, reference {float(ref[idx])!r}, "
                             f"{top:.3g} x its gate")

    def exact(self, place: str, name: str, got: torch.Tensor, want: torch.Tensor) -> None:
        """Bit for bit (half types), ``[image, token, channel]``."""
        wrong = _bits(got) != _bits(want)
        self.rows.append((place, name, math.inf if bool(wrong.any()) else 0.0))
        if bool(wrong.any()):
            idx = tuple(int(i) for i in torch.nonzero(wrong)[0])
            self.fail(place, f"{name}: {int(wrong.sum())} elements differ in their bits; first (image, token, channel) {idx}: got "
                             f"{float(got[idx])!r}, reference {float(want[idx])!r}")

    def zeros(self, place: str, what: str, lanes: torch.Tensor) -> None:
        if lanes.numel() and bool((lanes != 0).any()):
            idx = tuple(int(i) for i in torch.nonzero(lanes != 0)[0])
            self.fail(place, f"{what}: {int((lanes != 0).sum())} pad lanes are not exact zeros; first (image, token, pad lane) {idx}: "
                             f"{float(lanes[idx])!r}")

    # -- the walk
    def check(self) -> list[tuple[str, str, float]]:
        names = [c.name for c in self.trace]
        for i, (place, name) in enumerate(self.plan.stages):
            if i >= len(names) or names[i] != name:
                raise StageFailure(place, f"sequence: the configuration implies {name}, the graph called {names[i] if i < len(names) else 'nothing'}")
        if len(names) != len(self.plan.stages):
            raise StageFailure("end", f"sequence: {len(names) - len(self.plan.stages)} calls beyond the graph: {names[len(self.plan.stages):]}")
        calls = iter(self.trace)
        cols = self.patchify(next(calls))
        tok = self.linear("patch_embed.proj", next(calls), cols, "patch_embed.proj", None, None)
        x = self.assemble(next(calls), tok)
        for i in range(len(self.vit.blocks)):
            b = f"blocks.{i}."
            a = self.layernorm(b + "norm1", next(calls), x, b + "norm1")
            qkv = self.linear(b + "qkv", next(calls), a, b + "attn.qkv", None, None)
            a = self.attention(b + "attn", next(calls), qkv)
            y = self.linear(b + "proj", next(calls), a, b + "attn.proj", b + "ls1.gamma", x)
            a = self.layernorm(b + "norm2", next(calls), y, b + "norm2")
            a = self.linear(b + "fc1", next(calls), a, b + "mlp.fc1", None, None)
            a = self.activation(b + "act", next(calls), a)
            x = self.linear(b + "fc2", next(calls), a, b + "mlp.fc2", b + "ls2.gamma", y)
        self.final(next(calls), x)
        if self.failures:
            raise self.failures[0]
        return self.rows

    # -- the stages
    def patchify(self, call: Call):
        place, p, dtype = "patchify", self.p, self.dtype
        k = 3 * p * p
        k_want = k if p % 8 == 0 else _up(k, 32)
        if call.name == "hip_vit_patchify_h":
            x, patch, out_dtype = call.args
            k_pad = k
        elif call.name == "hip_vit_patchify_pad_h":
            x, patch, k_pad, out_dtype = call.args
        else:
            x, table, patch, k_pad, out_dtype = call.args
            self.wired(place, _same(table, self.table32.to(dtype)), "the table is not the hook's, rounded once to the run's type")
        self.wired(place, _same(x, self.x), "the batch is not the one the graph was given")
        self.wired(place, (patch, k_pad, out_dtype) == (p, k_want, dtype), f"patch, k_pad, dtype {(patch, k_pad, out_dtype)}, not {(p, k_want, dtype)}")
        src = self.table32.to(dtype)[x.long(), torch.arange(3)] if x.dtype == torch.uint8 else x.to(dtype)  # rounded ONCE to the run's type
        n, (gh, gw) = self.n, self.grid
        unf = F.unfold(src.float().permute(0, 3, 1, 2), kernel_size=p, stride=p)  # [n, (c, ky, kx), g]
        want = unf.reshape(n, 3, p, p, gh * gw).permute(0, 4, 2, 3, 1).reshape(n, gh * gw, k).to(dtype)  # (ky, kx, c); exact
        out = call.out
        if tuple(out.shape) != (n, gh * gw, k_want) or out.dtype != dtype:
            self.fail(place, f"{call.name}: result {tuple(out.shape)}, {out.dtype}")
            return out
        self.exact(place, call.name, out[..., :k], want)
        self.zeros(place, call.name, _bits(out[..., k:]))  # +0, bit for bit
        return out

    def linear(self, place: str, call: Call, x_in, layer: str, gamma: str | None, residual):
        """``x_in``: what the stage in front produced (a tensor, or that stage's ``Call`` for a quantising producer)."""
        sd, dtype, hidden, h_pad = self.sd, self.dtype, self.plan.hidden, self.plan.h_pad
        w32, b32 = _folded(sd, layer, gamma)
        what = layer.rsplit(".", 1)[-1]
        if layer == "patch_embed.proj":  # [D, 3, p, p] -> (ky, kx, c) columns; the tokens' pad columns are zeros
            w32 = w32.permute(0, 2, 3, 1).reshape(w32.shape[0], -1)
        cout_real, cin_real = w32.shape
        out = call.out
        if what == "fc1" and self.swiglu:  # gate lanes [0, H), value lanes [h_pad, h_pad + H); the reference has no padding
            lanes = torch.cat([torch.arange(hidden), h_pad + torch.arange(hidden)])
            cout = 2 * h_pad
        else:
            lanes, cout = torch.arange(cout_real), cout_real
        is_fp8 = call.name == "hip_linear_fp8_rows"
        res = call.args[3] if len(call.args) > 3 else call.kwargs.get("residual")  # noqa: PLR2004
        if residual is None:
            self.wired(place, res is None, "a residual where the graph has none")
        else:
            self.wired(place, _same(res, residual), "the residual is not " + ("the block's input" if what == "proj" else "proj's output"))
        if is_fp8:
            producer = x_in
            self.wired(place, isinstance(producer, Call) and call.live_args[0] is producer.live_out,
                       "the QuantRows are not the producer's output object")
            a = call.args[0]
            self.wired(place, _same(a.codes, producer.out.codes) and _same(a.scales, producer.out.scales), "codes / scales changed on the way")
            self.wired(place, call.kwargs.get("dtype") == dtype, f"dtype {call.kwargs.get('dtype')}")
            rows = a.codes.reshape(-1, a.codes.shape[-1])
            shape_in = tuple(a.codes.shape)
        else:
            x = call.args[0]
            self.wired(place, _same(x, x_in), "the input is not the previous stage's output")
            self.wired(place, call.kwargs.get("cout") == cout, f"cout {call.kwargs.get('cout')}, not {cout}")
            shape_in = tuple(x.shape)
        if tuple(out.shape) != (*shape_in[:2], cout) or out.dtype != dtype or shape_in[-1] < cin_real:
            self.fail(place, f"{call.name}: {shape_in} -> {tuple(out.shape)}, {out.dtype}; the graph carries {cout} channels")
            return out
        res64 = res.double().reshape(-1, cout) if res is not None else None
        if is_fp8:
            from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_e4m3

            wq, ws = quantize_rows_e4m3(w32)
            ref = gemm_ref64(rows[:, :cin_real], a.scales, wq.view(torch.uint8), ws, b32, res64[:, lanes] if res64 is not None else None)
        else:
            ref = x.double().reshape(-1, shape_in[-1])[:, :cin_real] @ w32.to(dtype).double().T + b32.double()
            if res64 is not None:
                ref = ref + res64[:, lanes]
        ref = ref.reshape(*shape_in[:2], -1)
        bound = HALF_EPS[dtype] * ref.abs() + 1e-4 * float(ref.abs().max())
        self.gate(place, call.name, out[..., lanes], ref, bound)
        pads = torch.ones(cout, dtype=torch.bool)
        pads[lanes] = False
        self.zeros(place, call.name, out[..., pads])
        return out

    def assemble(self, call: Call, tok: torch.Tensor):
        place, sd, d, r, vit = "tokens", self.sd, self.d, self.r, self.vit
        self.wired(place, _same(call.args[0], tok), "the tokens are not the patch GEMM's output")
        pos = sd["pos_embed"]
        npre = 0 if vit.no_embed_class else 1 + (r if vit.prefix_pos_embed else 0)
        g0 = tuple(vit.native_grid)
        assert pos.shape[1] == npre + g0[0] * g0[1]
        if self.grid != g0:
            tab = pos[:, npre:].reshape(1, g0[0], g0[1], d).permute(0, 3, 1, 2)
            tab = F.interpolate(tab, size=self.grid, mode="bicubic", antialias=True, align_corners=False)
            pos = torch.cat([pos[:, :npre], tab.permute(0, 2, 3, 1).reshape(1, -1, d)], dim=1)
        pos = pos.double()
        prefix = [sd["cls_token"].double()] + ([sd["reg_token"].double()] if r else [])
        seq = torch.cat([*[t.expand(self.n, -1, -1) for t in prefix], call.args[0].double()], dim=1)
        if vit.no_embed_class:
            seq[:, 1 + r:] += pos
        else:
            seq = seq + pos
        out = call.out
        if tuple(out.shape) != tuple(seq.shape) or out.dtype != self.dtype:
            self.fail(place, f"{call.name}: result {tuple(out.shape)}, {out.dtype}")
            return out
        # one unit in the last place of the half type: u |ref|, and below fp16's normal range (2^-14) the spacing of its subnormals,
        # 2^-24 -- the figure test_gelu_rows adds for the same reason; u |ref| alone refuses the correctly rounded sum there
        bound = UNIT[self.dtype] * seq.abs()
        self.gate(place, call.name, out, seq, bound.clamp_min(2.0 ** -24) if self.dtype == torch.float16 else bound)
        return out

    def layernorm(self, place: str, call: Call, x: torch.Tensor, norm: str):
        """The per-block form, half or quantising: every row of ``x``.  Returns what the next GEMM is checked against."""
        n, s, d, dtype = self.n, self.s, self.d, self.dtype
        self.wired(place, _same(call.args[0], x), "the input is not " + ("the block's input" if norm.endswith("1") else "proj's output"))
        self.wired(place, call.kwargs.get("eps") == LN_EPS, f"eps {call.kwargs.get('eps')}")
        ref = layernorm64(call.args[0].reshape(-1, d), self.sd[norm + ".weight"], self.sd[norm + ".bias"], LN_EPS)
        if call.name == "hip_layernorm_rows_q8":
            self.quantised(place, call, ref, (n, s, d))
            return call
        kw = call.kwargs
        self.wired(place, (kw.get("rows"), kw.get("row_stride")) == (n * s, d) and kw.get("out_dtype") in (None, dtype),
                   f"rows {kw.get('rows')} at stride {kw.get('row_stride')} to {kw.get('out_dtype')}, not {n * s} at {d}")
        out = call.out
        if tuple(out.shape) != (n * s, d) or out.dtype != dtype:
            self.fail(place, f"{call.name}: result {tuple(out.shape)}, {out.dtype}")
            return out
        bound = UNIT[dtype] * ref.abs() + 2.0 ** -16 * float(ref.abs().max())
        self.gate(place, call.name, out.reshape(n, s, d), ref.reshape(n, s, d), bound.reshape(n, s, d))
        return out.reshape(n, s, d)

    def quantised(self, place: str, call: Call, y64: torch.Tensor, shape: tuple) -> None:
        """``_vit_fp8_ref.check_quantised_rows``'s two conditions on a producer's codes and scales, per element."""
        q = call.out
        if tuple(q.codes.shape) != shape or q.codes.dtype != torch.uint8 or q.scales.numel() != shape[0] * shape[1]:
            self.fail(place, f"{call.name}: codes {tuple(q.codes.shape)}, {q.codes.dtype}, {q.scales.numel()} scales")
            return
        ds, deq, ratio = quantised_rows_ratios(y64.reshape(-1, shape[-1]), q.codes, q.scales)
        ds = ds.nan_to_num(nan=math.inf)
        if float(ds.max()) > SCALE_ULPS:
            row = int(torch.nonzero(ds == ds.max())[0])
            self.fail(place, f"{call.name}: the scale of (image, token) {divmod(row, shape[1])} is {float(ds[row]):.3g} float32 ulp off amax / 448")
        ratio = ratio.nan_to_num(nan=math.inf).reshape(shape)
        top = float(ratio.max())
        self.rows.append((place, call.name, max(top, float(ds.max()) / SCALE_ULPS)))
        if top > 1.0:
            idx = tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0])
            self.fail(place, f"{call.name}: worst element (image, token, channel) {idx}: got {float(deq.reshape(shape)[idx])!r}, reference "
                             f"{float(y64.reshape(shape)[idx])!r}, {top:.3g} x its gate")

    def attention(self, place: str, call: Call, qkv_in: torch.Tensor):
        n, s, d, heads, dtype = self.n, self.s, self.d, self.heads, self.dtype
        hd = d // heads
        qkv = call.args[0]
        self.wired(place, _same(qkv, qkv_in), "the input is not qkv's output")
        got_heads, got_scale = call.args[1], call.args[2]
        self.wired(place, got_heads == heads and got_scale == hd ** -0.5,
                   f"heads {got_heads}, scale {got_scale!r}; the module has {heads} heads and head_dim ** -0.5 = {hd ** -0.5!r}")
        out = call.out
        if tuple(out.shape) != (n, s, d) or out.dtype != dtype:
            self.fail(place, f"{call.name}: result {tuple(out.shape)}, {out.dtype}")
            return out
        q, k, v = (qkv.reshape(n, s, 3, heads, hd)[:, :, i].permute(0, 2, 1, 3) for i in range(3))  # [n, heads, s, hd]
        sc = (q.double() @ k.double().transpose(-2, -1)) * hd ** -0.5
        ref = (torch.softmax(sc, -1) @ v.double()).permute(0, 2, 1, 3).reshape(n, s, d)
        yard = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n, s, d)
        top = float(ref.abs().max())
        e_yard = float((yard.double() - ref).abs().max()) / top
        err = (out.double() - ref).abs().nan_to_num(nan=math.inf)
        e_new = float(err.max()) / top
        ratio = e_new / (2.0 * e_yard)  # over the whole tensor, as test_attention_matches_float64
        self.rows.append((place, call.name, ratio))
        if not ratio <= 1.0:
            idx = tuple(int(i) for i in torch.nonzero(err == err.max())[0])
            self.fail(place, f"{call.name}: e {e_new:.3e} is {ratio:.3g} x its gate 2 e_yard = {2 * e_yard:.3e}; worst element (image, token, "
                             f"channel) {idx}: got {float(out[idx])!r}, reference {float(ref[idx])!r}")
        return out

    def activation(self, place: str, call: Call, fc1_out: torch.Tensor):
        dtype, hidden, h_pad = self.dtype, self.plan.hidden, self.plan.h_pad
        x = call.args[0]
        self.wired(place, _same(x, fc1_out), "the input is not fc1's output")
        if tuple(x.shape) != (self.n, self.s, 2 * h_pad if self.swiglu else h_pad):
            self.fail(place, f"{call.name}: input {tuple(x.shape)}")
            return call.out
        xd = x.double()
        if self.swiglu:
            gate, value = xd[..., :hidden], xd[..., h_pad:h_pad + hidden]
            ref = gate / (1.0 + torch.exp(-gate)) * value
        else:
            ref = gelu64(x)
        shape = (self.n, self.s, h_pad)
        if call.name == "hip_act_rows_q8":
            self.wired(place, call.kwargs.get("swiglu") == self.swiglu, f"swiglu={call.kwargs.get('swiglu')}")
            self.quantised(place, call, F.pad(ref, (0, h_pad - ref.shape[-1])), shape)
            if tuple(call.out.codes.shape) == shape:
                self.zeros(place, call.name + " codes", call.out.codes[..., ref.shape[-1]:])
            return call
        out = call.out
        if tuple(out.shape) != shape or out.dtype != dtype:
            self.fail(place, f"{call.name}: result {tuple(out.shape)}, {out.dtype}")
            return out
        if self.swiglu:
            bound = SWIGLU_ROUND[dtype] * ref.abs() + 2.0 ** -20 * ref.abs() + SWIGLU_TINY[dtype]
        else:
            bound = UNIT[dtype] * ref.abs() + 2.0 ** -22 * xd.abs() + (2.0 ** -24 if dtype == torch.float16 else 0.0)
        self.gate(place, call.name, out[..., :ref.shape[-1]], ref, bound)
        self.zeros(place, call.name, out[..., ref.shape[-1]:])
        return out

    def final(self, call: Call, x: torch.Tensor) -> None:
        n, s, d, sd = self.n, self.s, self.d, self.sd
        place = self.plan.stages[-1][0]
        self.wired(place, _same(call.args[0], x), "the input is not the last fc2's output")
        self.wired(place, call.kwargs.get("eps") == LN_EPS, f"eps {call.kwargs.get('eps')}")
        out = call.out
        y = layernorm64(call.args[0], sd["norm.weight"], sd["norm.bias"], LN_EPS)  # [n, s, d]
        u32 = UNIT[torch.float32]
        if call.name == "hip_vit_cls_mean_pool_h":
            skip = 1 + self.r
            self.wired(place, call.kwargs.get("skip") == skip, f"skip {call.kwargs.get('skip')}, not 1 + reg_tokens = {skip}")
            if tuple(out.shape) != (n, 2 * d) or out.dtype != torch.float32:
                self.fail(place, f"{call.name}: result {tuple(out.shape)}, {out.dtype}")
                return
            ref_cls, rows = y[:, 0], y[:, skip:]  # test_cls_mean_pool's two bounds
            b_cls = u32 * ref_cls.abs() + 2.0 ** -16 * float(ref_cls.abs().max())
            b_mean = u32 * rows.abs().mean(1) + 2.0 ** -16 * float(rows.abs().max())
            self.gate(place, call.name, out[:, None], torch.cat([ref_cls, rows.mean(1)], -1)[:, None], torch.cat([b_cls, b_mean], -1)[:, None])
            return
        kw = call.kwargs
        self.wired(place, (kw.get("rows"), kw.get("row_stride"), kw.get("out_dtype")) == (n, s * d, torch.float32),
                   f"rows {kw.get('rows')} at stride {kw.get('row_stride')} to {kw.get('out_dtype')}, not {n} at {s * d} to float32")
        if tuple(out.shape) != (n, d) or out.dtype != torch.float32:
            self.fail(place, f"{call.name}: result {tuple(out.shape)}, {out.dtype}")
            return
        ref = y[:, 0]
        self.gate(place, call.name, out[:, None], ref[:, None], (u32 * ref.abs() + 2.0 ** -16 * float(ref.abs().max()))[:, None])


def table_lines(what: str, rows: list) -> list[str]:
    """One line per stage: the worst error as a multiple of the stage's gate."""
    return [f"trace {what} | {place:<18} {name:<28} {ratio:8.4f}" for place, name, ratio in rows]


# ------------------------------------------------------------------------------------------------------------- the model forms
class Form(NamedTuple):
    ident: str
    build: object          # () -> the float32 module
    n: int
    size: tuple            # (h, w)
    dtypes: tuple
    fp8: bool = False
    hook: str | None = None  # a `timm_preproc_func` name: the uint8 entrance


def _forms() -> list[Form]:
    from _vit_foundation_ref import TINY_GIGA, TINY_REG, tiny_foundation
    from _vit_ref import tiny_vit
    from _vit_virchow_ref import TINY_V1, TINY_V2, tiny_virchow

    both, bf16 = (torch.float16, torch.bfloat16), (torch.bfloat16,)
    forms = []
    for ls in (True, False):  # s = 17 (51 rows, partial tiles everywhere); resampled positions; s = 197 (three key tiles and a tail of 5)
        for n, size in ((3, (64, 64)), (3, (48, 64)), (2, (224, 224))):
            forms.append(Form(f"tiny-{'ls' if ls else 'plain'}-n{n}-{size[0]}x{size[1]}", lambda ls=ls: tiny_vit(layer_scale=ls), n, size, both))
    forms += [Form("reg-n3-42x56", lambda: tiny_foundation(TINY_REG), 3, (42, 56), both),
              Form("giga-n2-48x32", lambda: tiny_foundation(TINY_GIGA), 2, (48, 32), both)]
    for name, cfg in (("v1", TINY_V1), ("v2", TINY_V2)):
        forms += [Form(f"{name}-n2-28x28", lambda cfg=cfg: tiny_virchow(cfg), 2, (28, 28), both),
                  Form(f"{name}-n3-42x56", lambda cfg=cfg: tiny_virchow(cfg), 3, (42, 56), both)]
    forms += [Form("u8-tiny-n2-64x64", tiny_vit, 2, (64, 64), both, hook="vit_small_patch16_224"),
              Form("u8-reg-n2-42x56", lambda: tiny_foundation(TINY_REG), 2, (42, 56), both, hook="UNI2")]
    small = lambda **over: tiny_vit(embed_dim=128, num_heads=2, mlp_dim=512, **over)  # noqa: E731
    forms += [Form("fp8-tiny-n3-64x64", small, 3, (64, 64), bf16, fp8=True),
              Form("fp8-tiny-n2-224x224", small, 2, (224, 224), bf16, fp8=True),
              Form("fp8-reg4-n3-42x56", lambda: tiny_foundation({**TINY_REG, "reg_tokens": 4}), 3, (42, 56), bf16, fp8=True),
              Form("fp8-v2-n2-28x28", lambda: tiny_virchow(TINY_V2), 2, (28, 28), bf16, fp8=True),  # qkv stays half, H goes to 640
              Form("fp8-mlp576-n2-64x64", lambda: tiny_vit(mlp_dim=576), 2, (64, 64), bf16, fp8=True)]  # fc2 stays half
    return forms


FORMS = _forms()
CASES = [(form, dtype) for form in FORMS for dtype in form.dtypes]
CASE_IDS = [f"{form.ident}-{'fp16' if dtype == torch.float16 else 'bf16'}" for form, dtype in CASES]


def form_input(form: Form) -> tuple[torch.Tensor, torch.Tensor | None]:
    """``(the NHWC batch, the hook's float32 table or None)``: normal draws, or -- for the uint8 entrance -- noise with every byte value
    in every channel."""
    n, (h, w) = form.n, form.size
    if form.hook is None:
        return torch.randn((n, h, w, 3), generator=torch.Generator().manual_seed(h + w + n)), None
    from _vit_classifier_ref import all_bytes_batch

    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    return torch.from_numpy(all_bytes_batch(n, h, w, seed=h + w)), timm_preproc_func(form.hook).table


def fused_graph(vit, dtype: torch.dtype, *, fp8: bool, device: str):
    import copy

    from tiatoolbox_amd.models.architecture.vit_fused import FP8_LINEAR, FusedViT

    fused = FusedViT(copy.deepcopy(vit).to(device))
    fused.prepare(dtype, linear_dtype=FP8_LINEAR if fp8 else None)
    return fused.to(dtype)


def run_graph(fused, x: torch.Tensor, table32: torch.Tensor | None, dtype: torch.dtype, device: str) -> torch.Tensor:
    with torch.no_grad():
        if table32 is not None:
            return fused.forward_uint8(x.to(device), table32.to(dtype).to(device))
        return fused(x.to(device).permute(0, 3, 1, 2))

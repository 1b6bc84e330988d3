"""Host-only helpers of the ``FusedViT`` stage-trace tests: a recorder of every wrapper call the graph makes, the sequence of calls a
model's configuration implies, and a checker that holds EVERY stage, at every element of every token, to a float64 reference built
from the bits that entered that stage and the torch module's own float32 ``state_dict()`` -- never from ``FusedViT``'s folded, padded
or packed attributes.  The gates are the ones each kernel's own test holds it to (imported, not restated); torch stand-ins of the FP8
wrappers complete ``_vit_classifier_ref.torch_vit_wrappers`` for runs without a GPU.  Four routes beside the half graph: ``"fp8"`` and
``"int8"`` (quantised ``qkv`` / ``fc1`` / ``fc2``), ``"resid32"`` (``residual_dtype="float32"``: the float32 stream that one wrapper
updates in place) and ``"split"`` (the float32 route of ``linear_dtype="bfloat16x3"``)."""

from __future__ import annotations

import math
from typing import NamedTuple

import torch
import torch.nn.functional as F  # noqa: N812

from _vit_fp8_ref import HALF_EPS, SCALE_ULPS, gelu64, gemm_ref64, layernorm64, quantised_rows_ratios
from _vit_int8_ref import gemm_ref64 as gemm_ref64_int8
from _vit_int8_ref import quantised_rows_figures
from test_vit_f32_gpu import FLOOR as F32_FLOOR
from test_vit_f32_kernels_gpu import TINY32, U32
from test_vit_foundation_kernels_gpu import ROUND as SWIGLU_ROUND
from test_vit_foundation_kernels_gpu import TINY as SWIGLU_TINY
from test_vit_kernels_gpu import UNIT
from test_vit_resid32_kernels_gpu import UNIT as STREAM_UNIT

LN_EPS = 1e-6
TRACED = ("hip_vit_patchify_h", "hip_vit_patchify_pad_h", "hip_vit_patchify_norm_u8_h", "hip_linear_h", "hip_linear_fp8_rows",
          "hip_vit_assemble_tokens_h", "hip_vit_assemble_prefix_h", "hip_layernorm_rows_h", "hip_layernorm_rows_q8", "hip_mha_fwd_h",
          "hip_gelu_rows_h_", "hip_swiglu_rows_h", "hip_act_rows_q8", "hip_vit_cls_mean_pool_h",
          "hip_add_layernorm_rows_f32", "hip_vit_assemble_rows_f32", "hip_vit_cls_mean_pool_f32", "hip_linear_f32", "hip_mha_fwd_f32",
          "hip_gelu_rows_f32_", "hip_swiglu_rows_f32", "hip_vit_patchify_f32", "hip_vit_assemble_f32", "hip_linear_int8_rows",
          "hip_layernorm_rows_qi8", "hip_act_rows_qi8")
# wrapper -> the positional tensor arguments copied AFTER the call as well: ``tia_add_layernorm_rows_f32`` is documented to write its
# ``x`` in place (``include/tiatoolbox_amd.h``), ``tia_vit_cls_mean_pool_f32`` to add the branch on load and write nothing back
AFTER = {"hip_add_layernorm_rows_f32": (0,), "hip_vit_cls_mean_pool_f32": (0,)}
HALVES = (torch.float16, torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------- the recorder
class Call(NamedTuple):
    """One wrapper call: ``args`` / ``kwargs`` / ``out`` with every tensor copied to the CPU (the arguments BEFORE the call, the result
    after it); ``live_args`` / ``live_out`` the objects themselves, for the checks of identity; ``after`` the CPU copies of the
    arguments ``AFTER`` lists for this wrapper, taken after the call (argument index -> tensor)."""

    name: str
    args: tuple
    kwargs: dict
    out: object
    live_args: tuple
    live_out: object
    after: dict = {}  # noqa: RUF012  (a NamedTuple default: never written to)


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
            after = {i: _to_cpu(args[i]) for i in AFTER.get(name, ()) if i < len(args)}
            trace.append(Call(name, cpu_args, cpu_kwargs, _to_cpu(out), args, out, after))
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
ROUTES = (None, "fp8", "int8", "resid32", "split")
QUANT = {"fp8": ("hip_linear_fp8_rows", "hip_layernorm_rows_q8", "hip_act_rows_q8"),
         "int8": ("hip_linear_int8_rows", "hip_layernorm_rows_qi8", "hip_act_rows_qi8")}


class Plan(NamedTuple):
    stages: list  # (place in the graph, wrapper name), in the order of the calls
    hidden: int   # the MLP's real width: fc2's inputs
    h_pad: int    # the width the graph carries per SwiGLU half (== hidden without padding, and for the GELU)
    fp8: dict     # "qkv" / "fc1" / "fc2" -> on the quantised GEMM of the route (FP8 or INT8)
    route: str | None = None
    split: dict = {}  # noqa: RUF012  (route "split": "patch" / "qkv" / "proj" / "fc1" / "fc2" -> on the split kernel; else the float32 GEMM)


def _up(v: int, m: int) -> int:
    return -(-v // m) * m


def int8_rule(cout: int, cin: int) -> bool:
    """``FusedViT._route_int8``'s rule as documented: ``cin % 128 == 0 and cout % 16 == 0``."""
    return cin % 128 == 0 and cout % 16 == 0


def split_rule(cout: int, cin: int) -> bool:
    """Whether the split kernel serves a layer (``pack_linear_weights_split``): ``cin % 16 == 0 and cout % 128 == 0``."""
    return cin % 16 == 0 and cout % 128 == 0


def plan_of(vit, *, uint8: bool = False, fp8: bool = False, route: str | None = None) -> Plan:
    """The calls ``FusedViT`` makes for ``vit`` on ``route`` (``fp8=True`` is ``route="fp8"``), from its configuration and the shapes of
    its state dict alone.  A packed SwiGLU half at or above 512 that is off the half GEMM's multiple of 32 is carried at the next one,
    on the FP8 and INT8 routes at the next multiple of 128, and on the split route at the next multiple of 64 when ``fc1``'s width is
    off 128 (the module docstring of ``vit_fused``); a Linear goes to the quantised GEMM where ``fp8_rule`` / ``int8_rule`` takes the
    graph's shape, and on the split route to the split kernel where ``split_rule`` does."""
    route = route or ("fp8" if fp8 else None)
    assert route in ROUTES, route
    sd = vit.state_dict()
    d, p = vit.embed_dim, vit.patch_size
    swiglu = vit.mlp_layer == "swiglu_packed"
    hidden = sd["blocks.0.mlp.fc2.weight"].shape[1]
    assert sd["blocks.0.mlp.fc1.weight"].shape[0] == (2 * hidden if swiglu else hidden)
    h_pad = hidden
    if swiglu and hidden >= 512 and hidden % 32 != 0:  # noqa: PLR2004
        h_pad = _up(hidden, 32)
    if swiglu and route in QUANT and h_pad >= 512 and h_pad % 128 != 0:  # noqa: PLR2004
        h_pad = _up(h_pad, 128)
    if swiglu and route == "split" and h_pad >= 512 and (2 * h_pad) % 128 != 0:  # noqa: PLR2004
        h_pad = _up(h_pad, 64)
    fc1_out = 2 * h_pad if swiglu else h_pad
    prefix = bool(vit.reg_tokens or vit.no_embed_class)
    pooled = vit.global_pool == "token_mean"
    blocks = [f"blocks.{i}." for i in range(len(vit.blocks))]
    if route == "split":
        k = 3 * p * p
        split = {"patch": split_rule(d, k if p % 8 == 0 else _up(k, 32)), "qkv": split_rule(3 * d, d), "proj": split_rule(d, d),
                 "fc1": split_rule(fc1_out, d), "fc2": split_rule(d, h_pad)}
        stages = [("patchify", "hip_vit_patchify_f32"), ("patch_embed.proj", "hip_linear_f32"), ("tokens", "hip_vit_assemble_f32")]
        act = "hip_swiglu_rows_f32" if swiglu else "hip_gelu_rows_f32_"
        for b in blocks:
            stages += [(b + "norm1", "hip_add_layernorm_rows_f32"), (b + "qkv", "hip_linear_f32"), (b + "attn", "hip_mha_fwd_f32"),
                       (b + "proj", "hip_linear_f32"), (b + "norm2", "hip_add_layernorm_rows_f32"), (b + "fc1", "hip_linear_f32"),
                       (b + "act", act), (b + "fc2", "hip_linear_f32")]
        stages.append(("norm_pool", "hip_vit_cls_mean_pool_f32") if pooled else ("norm", "hip_add_layernorm_rows_f32"))
        return Plan(stages, hidden, h_pad, dict.fromkeys(("qkv", "fc1", "fc2"), False), route, split)
    rule = {"fp8": fp8_rule, "int8": int8_rule}.get(route, lambda cout, cin: False)  # noqa: ARG005
    routes = {"qkv": rule(3 * d, d), "fc1": rule(fc1_out, d), "fc2": rule(d, h_pad)}
    q_linear, q_norm, q_act = QUANT.get(route, (None, None, None))
    linear = lambda name: q_linear if routes[name] else "hip_linear_h"  # noqa: E731
    stream_norm = "hip_add_layernorm_rows_f32" if route == "resid32" else "hip_layernorm_rows_h"
    norm = lambda name: q_norm if routes[name] else stream_norm  # noqa: E731
    if uint8:
        first = "hip_vit_patchify_norm_u8_h"
    else:
        first = "hip_vit_patchify_h" if p % 8 == 0 else "hip_vit_patchify_pad_h"
    if route == "resid32":
        tokens = "hip_vit_assemble_rows_f32"
    else:
        tokens = "hip_vit_assemble_prefix_h" if prefix else "hip_vit_assemble_tokens_h"
    stages = [("patchify", first), ("patch_embed.proj", "hip_linear_h"), ("tokens", tokens)]
    act = q_act if routes["fc2"] else ("hip_swiglu_rows_h" if swiglu else "hip_gelu_rows_h_")
    for b in blocks:
        stages += [(b + "norm1", norm("qkv")), (b + "qkv", linear("qkv")), (b + "attn", "hip_mha_fwd_h"), (b + "proj", "hip_linear_h"),
                   (b + "norm2", norm("fc1")), (b + "fc1", linear("fc1")), (b + "act", act), (b + "fc2", linear("fc2"))]
    if route == "resid32":
        stages.append(("norm_pool", "hip_vit_cls_mean_pool_f32") if pooled else ("norm", "hip_add_layernorm_rows_f32"))
    else:
        stages.append(("norm_pool", "hip_vit_cls_mean_pool_h") if pooled else ("norm", "hip_layernorm_rows_h"))
    return Plan(stages, hidden, h_pad, routes, route)


# ---------------------------------------------------------------------------------------------------------------------- the checker
class StageFailure(AssertionError):
    """A stage off its reference or its wiring; ``place`` is where it sits in the graph (``blocks.1.fc2``)."""

    def __init__(self, place: str, text: str) -> None:
        super().__init__(f"{place}: {text}")
        self.place = place


def _same(a, b) -> bool:
    return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)  # noqa: PLR2004


def _same_bits(a, b) -> bool:
    return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(_bits(a), _bits(b))


def _strided_rows(t: torch.Tensor, rows: int, c: int, stride: int) -> torch.Tensor:
    return torch.as_strided(t.reshape(-1), (rows, c), (stride, 1))  # (a view of the contiguous tensor: writes land in `t`)


class Stream:
    """The float32 residual stream between two passes: the tensor object the graph holds and its recorded values."""

    def __init__(self, call: Call) -> None:
        self.live, self.state = call.live_out, call.out


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

    def __init__(self, vit, trace: list[Call], x: torch.Tensor, dtype: torch.dtype, *, fp8: bool = False, route: str | None = None,
                 table32: torch.Tensor | None = None) -> None:
        self.vit, self.trace, self.x, self.dtype, self.table32 = vit, trace, x.cpu(), dtype, table32
        self.sd = {k: v.detach().cpu().float() for k, v in vit.state_dict().items()}
        self.plan = plan_of(vit, uint8=x.dtype == torch.uint8, fp8=fp8, route=route)
        self.route = self.plan.route
        assert (dtype == torch.float32) == (self.route == "split"), (dtype, self.route)
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

    def measure(self, place: str, name: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
        """The worst ``|got - ref| / bound`` over ``[image, token, channel]`` (a zero bound asks for equality, a NaN is the worst
        element); above 1 it is a failure of ``place``."""
        got, ref = got.double(), ref.double()
        err = (got - ref).abs()
        unequal = torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf))
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), unequal).nan_to_num(nan=math.inf)
        top = float(ratio.max())
        if top > 1.0:
            idx = tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0])
            self.fail(place, f"{name}: worst element (image, token, channel) {idx}: got {float(got[idx])!r}, reference {float(ref[idx])!r}, "
                             f"{top:.3g} x its gate")
        return top

    def gate(self, place: str, name: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> None:
        """Every element of ``got`` ``[image, token, channel]`` within ``bound`` of ``ref``: the stage's one line."""
        self.rows.append((place, name, self.measure(place, name, got, ref, bound)))

    def differ(self, place: str, name: str, got: torch.Tensor, want: torch.Tensor, what: str = "") -> float:
        """0 when ``got`` is ``want`` bit for bit (half types and float32), ``[image, token, channel]``; else a failure and ``inf``."""
        wrong = _bits(got) != _bits(want)
        if not bool(wrong.any()):
            return 0.0
        idx = tuple(int(i) for i in torch.nonzero(wrong)[0])
        self.fail(place, f"{name}: {what}{int(wrong.sum())} elements differ in their bits; first (image, token, channel) {idx}: got "
                         f"{float(got[idx])!r}, reference {float(want[idx])!r}")
        return math.inf

    def exact(self, place: str, name: str, got: torch.Tensor, want: torch.Tensor) -> None:
        """Bit for bit: the stage's one line."""
        self.rows.append((place, name, self.differ(place, name, got, want)))

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
        {"resid32": self.walk_stream, "split": self.walk_f32}.get(self.route, self.walk_half)(calls)
        if self.failures:
            raise self.failures[0]
        return self.rows

    def walk_half(self, calls) -> None:
        """The half graph and its FP8 / INT8 forms: the residual adds are the GEMMs'."""
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

    def walk_stream(self, calls) -> None:
        """``residual_dtype="float32"``: ``proj`` and ``fc2`` write half branches without a residual; the pass in front of the next GEMM
        adds the branch to the float32 stream in place and normalises the sum."""
        cols = self.patchify(next(calls))
        tok = self.linear("patch_embed.proj", next(calls), cols, "patch_embed.proj", None, None)
        call = next(calls)
        self.assemble32(call, tok)
        x, branch = Stream(call), None  # the branch not yet added to x: the Call that made it
        for i in range(len(self.vit.blocks)):
            b = f"blocks.{i}."
            a = self.add_layernorm(b + "norm1", next(calls), x, branch, b + "norm1")
            qkv = self.linear(b + "qkv", next(calls), a, b + "attn.qkv", None, None)
            a = self.attention(b + "attn", next(calls), qkv)
            branch = next(calls)
            self.linear(b + "proj", branch, a, b + "attn.proj", b + "ls1.gamma", None)
            a = self.add_layernorm(b + "norm2", next(calls), x, branch, b + "norm2")
            a = self.linear(b + "fc1", next(calls), a, b + "mlp.fc1", None, None)
            a = self.activation(b + "act", next(calls), a)
            branch = next(calls)
            self.linear(b + "fc2", branch, a, b + "mlp.fc2", b + "ls2.gamma", None)
        if self.plan.stages[-1][0] == "norm_pool":
            self.pool32(next(calls), x, branch)
        else:
            self.add_layernorm("norm", next(calls), x, branch, "norm", final=True)

    def walk_f32(self, calls) -> None:
        """The float32 route: the residual adds are the GEMMs' again, on float32 tensors; the LayerNorm is the stream pass without a
        branch, which must leave its ``x`` as it found it."""
        cols = self.patchify(next(calls))
        tok = self.linear_f32("patch_embed.proj", next(calls), cols, "patch_embed.proj", None, None)
        call = next(calls)
        self.assemble32(call, tok)
        x = Stream(call)
        for i in range(len(self.vit.blocks)):
            b = f"blocks.{i}."
            a = self.add_layernorm(b + "norm1", next(calls), x, None, b + "norm1")
            qkv = self.linear_f32(b + "qkv", next(calls), a, b + "attn.qkv", None, None)
            a = self.attention(b + "attn", next(calls), qkv)
            call = next(calls)
            self.linear_f32(b + "proj", call, a, b + "attn.proj", b + "ls1.gamma", x.state)
            x = Stream(call)
            a = self.add_layernorm(b + "norm2", next(calls), x, None, b + "norm2")
            a = self.linear_f32(b + "fc1", next(calls), a, b + "mlp.fc1", None, None)
            a = self.activation_f32(b + "act", next(calls), a)
            call = next(calls)
            self.linear_f32(b + "fc2", call, a, b + "mlp.fc2", b + "ls2.gamma", x.state)
            x = Stream(call)
        if self.plan.stages[-1][0] == "norm_pool":
            self.pool32(next(calls), x, None)
        else:
            self.add_layernorm("norm", next(calls), x, None, "norm", final=True)

    # -- the stages
    def patchify(self, call: Call):
        place, p, dtype = "patchify", self.p, self.dtype
        k = 3 * p * p
        k_want = k if p % 8 == 0 else _up(k, 32)
        if call.name == "hip_vit_patchify_h":
            x, patch, out_dtype = call.args
            k_pad = k
        elif call.name == "hip_vit_patchify_f32":  # a pure gather of float32 values: the same statement, bit for bit
            (x, patch, k_pad), out_dtype = call.args, torch.float32
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
        is_int8 = call.name == "hip_linear_int8_rows"
        is_fp8 = call.name == "hip_linear_fp8_rows" or is_int8  # (a quantised GEMM: QuantRows in, the wiring is the same)
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
            self.wired(place, a.codes.dtype == (torch.int8 if is_int8 else torch.uint8), f"codes of {a.codes.dtype}")
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
        if is_int8:  # the weights by the recipe on the CPU, per output channel, from the float32 (folded) ones
            from tiatoolbox_amd.models.architecture.vit_fused import quantize_rows_int8

            wq, ws = quantize_rows_int8(w32)
            ref = gemm_ref64_int8(rows[:, :cin_real], a.scales, wq, ws, b32, res64[:, lanes] if res64 is not None else None)
        elif is_fp8:
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
        if call.name == "hip_layernorm_rows_qi8":
            self.quantised_int8(place, call, ref, (n, s, d))
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
        # over the whole tensor, as test_attention_matches_float64; the float32 kernel's test adds a floor of eight float32 units
        floor = 8.0 * U32 if call.name == "hip_mha_fwd_f32" else 0.0
        ratio = e_new / (2.0 * e_yard + floor)
        self.rows.append((place, call.name, ratio))
        if not ratio <= 1.0:
            idx = tuple(int(i) for i in torch.nonzero(err == err.max())[0])
            self.fail(place, f"{call.name}: e {e_new:.3e} is {ratio:.3g} x its gate 2 e_yard (+ floor) = {2 * e_yard + floor:.3e}; worst element "
                             f"(image, token, channel) {idx}: got {float(out[idx])!r}, reference {float(ref[idx])!r}")
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
        if call.name in ("hip_act_rows_q8", "hip_act_rows_qi8"):
            self.wired(place, call.kwargs.get("swiglu") == self.swiglu, f"swiglu={call.kwargs.get('swiglu')}")
            check = self.quantised if call.name == "hip_act_rows_q8" else self.quantised_int8
            check(place, call, F.pad(ref, (0, h_pad - ref.shape[-1])), shape)
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
            self.gate(place, call.name, out[:, None], *self.pooled(y, skip))
            return
        kw = call.kwargs
        self.wired(place, (kw.get("rows"), kw.get("row_stride"), kw.get("out_dtype")) == (n, s * d, torch.float32),
                   f"rows {kw.get('rows')} at stride {kw.get('row_stride')} to {kw.get('out_dtype')}, not {n} at {s * d} to float32")
        if tuple(out.shape) != (n, d) or out.dtype != torch.float32:
            self.fail(place, f"{call.name}: result {tuple(out.shape)}, {out.dtype}")
            return
        ref = y[:, 0]
        self.gate(place, call.name, out[:, None], ref[:, None], (u32 * ref.abs() + 2.0 ** -16 * float(ref.abs().max()))[:, None])

    @staticmethod
    def pooled(y: torch.Tensor, skip: int) -> tuple[torch.Tensor, torch.Tensor]:
        """``(reference, bound)`` ``[n, 1, 2d]`` of the pooled end from the float64 LayerNorm ``y [n, s, d]``: test_cls_mean_pool's two
        bounds (and test_cls_mean_pool_f32's, which are the same)."""
        u32 = UNIT[torch.float32]
        ref_cls, rows = y[:, 0], y[:, skip:]
        b_cls = u32 * ref_cls.abs() + 2.0 ** -16 * float(ref_cls.abs().max())
        b_mean = u32 * rows.abs().mean(1) + 2.0 ** -16 * float(rows.abs().max())
        return torch.cat([ref_cls, rows.mean(1)], -1)[:, None], torch.cat([b_cls, b_mean], -1)[:, None]

    # -- the stages of the INT8, float32-stream and float32 routes
    def quantised_int8(self, place: str, call: Call, y64: torch.Tensor, shape: tuple) -> None:
        """``_vit_int8_ref.quantised_rows_figures``'s two conditions on an INT8 producer's codes and scales: every row's scale within
        ``SCALE_ULPS`` float32 ulp of ``amax / 127``, every element within half a code step (its bound there); codes in [-127, 127]."""
        q = call.out
        if tuple(q.codes.shape) != shape or q.codes.dtype != torch.int8 or q.scales.numel() != shape[0] * shape[1]:
            self.fail(place, f"{call.name}: codes {tuple(q.codes.shape)}, {q.codes.dtype}, {q.scales.numel()} scales")
            return
        if int(q.codes.min()) < -127:  # noqa: PLR2004
            idx = tuple(int(i) for i in torch.nonzero(q.codes == -128)[0])  # noqa: PLR2004
            self.rows.append((place, call.name, math.inf))
            self.fail(place, f"{call.name}: a code of -128 at (image, token, channel) {idx}: outside the symmetric range [-127, 127]")
            return
        y64 = y64.reshape(-1, shape[-1])
        figures = lambda rows: quantised_rows_figures(y64[rows], q.codes.reshape(y64.shape)[rows], q.scales.reshape(-1)[rows])  # noqa: E731
        ds, worst = (v if v == v else math.inf for v in figures(slice(None)))  # noqa: PLR0124  (a NaN is the worst figure)
        self.rows.append((place, call.name, max(worst, ds / SCALE_ULPS)))
        if ds > SCALE_ULPS or worst > 1.0:  # name the worst row: the figures once more, row by row
            per_row = [figures(slice(r, r + 1)) for r in range(y64.shape[0])]
            nan_last = lambda v: math.inf if v != v else v  # noqa: E731, PLR0124
            if ds > SCALE_ULPS:
                row = max(range(len(per_row)), key=lambda r: nan_last(per_row[r][0]))
                self.fail(place, f"{call.name}: the scale of (image, token) {divmod(row, shape[1])} is {per_row[row][0]:.3g} float32 ulp off amax / 127")
            if worst > 1.0:
                row = max(range(len(per_row)), key=lambda r: nan_last(per_row[r][1]))
                self.fail(place, f"{call.name}: the worst element of (image, token) {divmod(row, shape[1])} is {per_row[row][1]:.3g} x its gate")

    def assemble32(self, call: Call, tok: torch.Tensor) -> None:
        """Token assembly with a float32 result (half or float32 tokens).  (1) The result is ONE float32 add of the call's own arguments,
        bit for bit.  (2) The arguments are the module's: ``cls`` / ``reg`` from the state dict (with the host-side ``cls + pos[0]`` and
        ``reg + pos[1 : 1 + R]`` of ``prefix_pos_embed``), the position table bit for bit on the native grid, and on a resampled grid
        within the project's yardstick rule of the float64 resampling: ``max |pos - ref64| <= 2 max |cpu32 - ref64| + 8 * 2^-24 max |pos|``
        (the CPU's float32 ``F.interpolate`` of the same table as the yardstick; the floor of ``test_vit_f32_gpu``)."""
        place, name, sd, d, r, vit, n = "tokens", call.name, self.sd, self.d, self.r, self.vit, self.n
        tokens, cls, reg, pos = call.args[:4]
        has_cls = call.kwargs.get("pos_has_cls")
        self.wired(place, _same(tokens, tok), "the tokens are not the patch GEMM's output")
        folded = bool(vit.prefix_pos_embed and r)
        self.wired(place, has_cls is (not (folded or vit.no_embed_class)), f"pos_has_cls={has_cls}")
        self.wired(place, (reg is None) == (r == 0), "register tokens " + ("missing" if reg is None else "where the module has none"))
        out, g = call.out, self.grid[0] * self.grid[1]
        if tuple(out.shape) != (n, self.s, d) or out.dtype != torch.float32 or pos.numel() != (g + int(bool(has_cls))) * d or \
                cls.numel() != d or (reg is not None and reg.numel() != r * d):
            self.fail(place, f"{name}: result {tuple(out.shape)}, {out.dtype}; cls {tuple(cls.shape)}, pos {tuple(pos.shape)}")
            return
        pos2 = pos.reshape(-1, d)
        parts = [(cls.reshape(1, d) + pos2[:1] if has_cls else cls.reshape(1, d)).expand(n, 1, d)]
        if reg is not None:
            parts.append(reg.reshape(1, r, d).expand(n, r, d))
        parts.append(tokens.float() + pos2[int(bool(has_cls)):])  # one IEEE float32 add per element
        ratio = self.differ(place, name, out, torch.cat(parts, 1), "not one float32 add of its arguments: ")
        table = sd["pos_embed"].reshape(-1, d)
        g0 = tuple(vit.native_grid)
        npre = 0 if vit.no_embed_class else 1 + (r if vit.prefix_pos_embed else 0)
        assert table.shape[0] == npre + g0[0] * g0[1]
        cls32, reg32 = sd["cls_token"].reshape(d), (sd["reg_token"].reshape(r, d) if r else None)
        if folded:
            cls32, reg32 = cls32 + table[0], reg32 + table[1:1 + r]  # the float32 adds FusedViT._prefix_for makes on the host side
        self.wired(place, _same_bits(cls.reshape(d), cls32), "cls is not the module's class token" + (" + pos[0]" if folded else ""))
        if r and reg is not None:
            self.wired(place, _same_bits(reg.reshape(r, d), reg32), "reg is not the module's register tokens" + (" + pos[1 : 1 + R]" if folded else ""))
        if has_cls:
            self.wired(place, _same_bits(pos2[0], table[0]), "pos[0] is not the table's class entry")
        got, tab = pos2[int(bool(has_cls)):], table[npre:]
        if self.grid == g0:
            self.wired(place, _same_bits(got, tab), "the position table is not the module's, bit for bit, on the native grid")
        else:
            tab = tab.reshape(1, g0[0], g0[1], d).permute(0, 3, 1, 2)
            resample = lambda t: F.interpolate(t, size=self.grid, mode="bicubic", antialias=True, align_corners=False).permute(  # noqa: E731
                0, 2, 3, 1).reshape(-1, d)
            ref, yard = resample(tab.double()), resample(tab)
            e_yard = float((yard.double() - ref).abs().max())
            err = (got.double() - ref).abs().nan_to_num(nan=math.inf)
            gate = 2.0 * e_yard + F32_FLOOR * float(table.abs().max())
            resampled = float(err.max()) / gate
            print(f"trace tokens | position table resampled {g0} -> {self.grid}: max error {float(err.max()):.3e}, the CPU's float32 "
                  f"F.interpolate {e_yard:.3e}: {resampled:.4f} of the gate")
            if not resampled <= 1.0:
                idx = tuple(int(i) for i in torch.nonzero(err == err.max())[0])
                self.fail(place, f"{name}: the resampled position table is {resampled:.3g} x its gate off the float64 resampling; worst "
                                 f"(grid position, channel) {idx}: got {float(got[idx])!r}, reference {float(ref[idx])!r}")
            ratio = max(ratio, resampled if resampled == resampled else math.inf)  # noqa: PLR0124
        self.rows.append((place, name, ratio))

    def add_layernorm(self, place: str, call: Call, x: Stream, branch: Call | None, norm: str, *, final: bool = False):
        """``hip_add_layernorm_rows_f32``: ``x`` after the call is ``x_before + float32(branch)`` bit for bit on the rows the call covers
        and unchanged on every other row (every row when there is no branch); the output is held to the float64 LayerNorm of that
        sum under ``test_vit_resid32_kernels_gpu``'s bound ``UNIT[out type] |ref| + 2^-16 max |ref|``.  ``final``: the class rows alone
        (``rows = n`` at stride ``S D``), float32 out.  ``x.state`` becomes the recorded after-state, which the next pass must be given."""
        n, s, d, name, kw = self.n, self.s, self.d, call.name, call.kwargs
        stream = self.route == "resid32"
        rows, stride = (n, s * d) if final else (n * s, d)
        out_dtype = self.dtype if stream and not final else torch.float32
        before, b = call.args[0], call.args[1]
        after = call.after.get(0)
        self.wired(place, call.live_args[0] is x.live, "x is not the stream object of the previous pass")
        self.wired(place, _same_bits(before, x.state), "x is not in the state the previous pass left it in")
        if branch is None:
            self.wired(place, b is None, "a branch where the graph has none")
        else:
            self.wired(place, call.live_args[1] is branch.live_out and _same(b, branch.out),
                       "the branch is not the previous " + ("proj" if norm.endswith("norm2") else "fc2") + " output")
        self.wired(place, (kw.get("rows"), kw.get("row_stride")) == (rows, stride),
                   f"rows {kw.get('rows')} at stride {kw.get('row_stride')}, not {rows} at {stride}")
        self.wired(place, kw.get("dtype") == self.dtype if stream else kw.get("dtype") in HALVES, f"dtype {kw.get('dtype')}")
        self.wired(place, (kw.get("out_dtype") or kw.get("dtype")) == out_dtype, f"out_dtype {kw.get('out_dtype')}, not {out_dtype}")
        self.wired(place, kw.get("eps") == LN_EPS, f"eps {kw.get('eps')}")
        out = call.out
        if tuple(before.shape) != (n, s, d) or before.dtype != torch.float32 or not isinstance(after, torch.Tensor) or \
                (b is not None and (tuple(b.shape) != (n, s, d) or b.dtype not in HALVES)):
            self.fail(place, f"{name}: x {tuple(before.shape)}, {before.dtype}; branch {None if b is None else (tuple(b.shape), b.dtype)}")
            return out
        want = before.clone()
        covered = _strided_rows(want, rows, d, stride)
        if b is not None:
            covered += _strided_rows(b, rows, d, stride).float()  # one IEEE float32 add per element, as the kernel's
        what = "x after the call is not x + float32(branch) on the rows the call covers, or changed on another row: "
        ratio = self.differ(place, name, after, want, what if b is not None else "x changed without a branch: ")
        x.state = after
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != (rows, d) or out.dtype != out_dtype:
            self.fail(place, f"{name}: result {tuple(out.shape) if isinstance(out, torch.Tensor) else out}, {getattr(out, 'dtype', None)}")
            self.rows.append((place, name, math.inf))
            return out
        ref = layernorm64(covered, self.sd[norm + ".weight"], self.sd[norm + ".bias"], LN_EPS)
        bound = STREAM_UNIT[out_dtype] * ref.abs() + 2.0 ** -16 * float(ref.abs().max())
        shape = (n, 1, d) if final else (n, s, d)
        self.rows.append((place, name, max(ratio, self.measure(place, name, out.reshape(shape), ref.reshape(shape), bound.reshape(shape)))))
        return out.reshape(shape)

    def pool32(self, call: Call, x: Stream, branch: Call | None) -> None:
        """``hip_vit_cls_mean_pool_f32``: the two bounds of ``test_cls_mean_pool_f32`` against the float64 LayerNorm of
        ``x + float32(branch)`` (one float32 add), and ``x`` itself bit for bit as before the call: the header says the branch is
        added on load and nothing is written back."""
        place, name, n, s, d, kw = "norm_pool", call.name, self.n, self.s, self.d, call.kwargs
        before, b = call.args[0], call.args[1]
        after = call.after.get(0)
        self.wired(place, call.live_args[0] is x.live, "x is not the stream object of the previous pass")
        self.wired(place, _same_bits(before, x.state), "x is not in the state the previous pass left it in")
        if branch is None:
            self.wired(place, b is None, "a branch where the graph has none")
        else:
            self.wired(place, call.live_args[1] is branch.live_out and _same(b, branch.out), "the branch is not the last fc2 output")
        skip = 1 + self.r
        self.wired(place, kw.get("skip") == skip, f"skip {kw.get('skip')}, not 1 + reg_tokens = {skip}")
        self.wired(place, kw.get("eps") == LN_EPS, f"eps {kw.get('eps')}")
        self.wired(place, kw.get("dtype") == self.dtype if self.route == "resid32" else kw.get("dtype") in HALVES, f"dtype {kw.get('dtype')}")
        out = call.out
        if tuple(out.shape) != (n, 2 * d) or out.dtype != torch.float32 or tuple(before.shape) != (n, s, d) or not isinstance(after, torch.Tensor):
            self.fail(place, f"{name}: result {tuple(out.shape)}, {out.dtype}; x {tuple(before.shape)}")
            return
        ratio = self.differ(place, name, after, before, "x was written to (the header: nothing is written back): ")
        xs = before + b.float() if b is not None else before  # the kernel's one float32 add
        y = layernorm64(xs, self.sd["norm.weight"], self.sd["norm.bias"], LN_EPS)
        self.rows.append((place, name, max(ratio, self.measure(place, name, out[:, None], *self.pooled(y, skip)))))

    def lanes_of(self, what: str, cout_real: int) -> tuple[torch.Tensor, int]:
        """``(the real output lanes, the width the graph carries)`` of a Linear: a packed SwiGLU ``fc1`` has its gate lanes at
        ``[0, H)`` and its value lanes at ``[h_pad, h_pad + H)``."""
        hidden, h_pad = self.plan.hidden, self.plan.h_pad
        if what == "fc1" and self.swiglu:
            return torch.cat([torch.arange(hidden), h_pad + torch.arange(hidden)]), 2 * h_pad
        return torch.arange(cout_real), cout_real

    def linear_f32(self, place: str, call: Call, x_in: torch.Tensor, layer: str, gamma: str | None, residual):
        """``hip_linear_f32``: the dtype of ``w_packed`` names the kernel (bf16 planes: the split kernel; float32: the plain GEMM) and must
        agree with ``split_rule``; ``x64 @ w32^T + b (+ residual)`` with the unrounded float32 (folded) weights -- the split is exact
        -- under ``test_linear_on_the_split_kernel``'s gate ``max |y - ref| <= 1e-5 max |ref|``, per element; pad lanes exact zeros."""
        w32, b32 = _folded(self.sd, layer, gamma)
        what = layer.rsplit(".", 1)[-1]
        if layer == "patch_embed.proj":
            w32, what = w32.permute(0, 2, 3, 1).reshape(w32.shape[0], -1), "patch"
        cout_real, cin_real = w32.shape
        lanes, cout = self.lanes_of(what, cout_real)
        x, w_packed, out = call.args[0], call.args[1], call.out
        res = call.args[3] if len(call.args) > 3 else call.kwargs.get("residual")  # noqa: PLR2004
        if residual is None:
            self.wired(place, res is None, "a residual where the graph has none")
        else:
            self.wired(place, _same_bits(res, residual),
                       "the residual is not the stream (" + ("the block's input" if what == "proj" else "proj's output") + ")")
        self.wired(place, _same(x, x_in), "the input is not the previous stage's output")
        self.wired(place, call.kwargs.get("cout") == cout, f"cout {call.kwargs.get('cout')}, not {cout}")
        on_split = {torch.bfloat16: True, torch.float32: False}.get(w_packed.dtype)
        self.wired(place, on_split is self.plan.split[what],
                   f"weights of {w_packed.dtype}: on the {'split kernel' if on_split else 'float32 GEMM'}, the rule (cin % 16 == 0 and cout % 128 "
                   f"== 0) says the {'split kernel' if self.plan.split[what] else 'float32 GEMM'}")
        shape_in = tuple(x.shape)
        if len(shape_in) != 3 or tuple(out.shape) != (*shape_in[:2], cout) or out.dtype != torch.float32 or shape_in[-1] < cin_real or \
                (res is not None and tuple(res.shape) != tuple(out.shape)):  # noqa: PLR2004
            self.fail(place, f"{call.name}: {shape_in} -> {tuple(out.shape)}, {out.dtype}; the graph carries {cout} channels")
            return out
        # the operand the kernel multiplies by IS the float32 (folded) weight, zeros in the pad rows and columns: the three bf16 planes
        # sum to it exactly (the header's layout [cin / 16][cout / 128][plane][8-channel chunk][column][channel]; a stand-in hands the
        # planes over as [3, cout, cin]), the float32 GEMM's [cin, cout] operand is it bit for bit
        cin = shape_in[-1]
        full = torch.zeros((cout, cin))
        full[lanes, :cin_real] = w32
        if on_split and w_packed.numel() == 3 * cout * cin and cin % 16 == 0 and cout % 128 == 0:
            planes = w_packed if w_packed.dim() == 3 else w_packed.reshape(cin // 16, cout // 128, 3, 2, 128, 8).permute(2, 1, 4, 0, 3, 5)  # noqa: PLR2004
            self.wired(place, torch.equal(planes.reshape(3, cout, cin).double().sum(0), full.double()),
                       "the three bf16 planes do not sum to the float32 (folded) weight")
        else:
            self.wired(place, on_split is False and w_packed.numel() == cout * cin and _same_bits(w_packed.reshape(cin, cout), full.T.contiguous()),
                       "the packed operand is not the float32 (folded) weight")
        ref = x.double().reshape(-1, cin)[:, :cin_real] @ w32.double().T + b32.double()
        if res is not None:
            ref = ref + res.double().reshape(-1, cout)[:, lanes]
        ref = ref.reshape(*shape_in[:2], -1)
        self.gate(place, call.name, out[..., lanes], ref, torch.full_like(ref, 1e-5 * float(ref.abs().max())))
        pads = torch.ones(cout, dtype=torch.bool)
        pads[lanes] = False
        self.zeros(place, call.name, out[..., pads])
        return out

    def activation_f32(self, place: str, call: Call, fc1_out: torch.Tensor):
        """``hip_gelu_rows_f32_`` / ``hip_swiglu_rows_f32`` under the element bounds of ``test_gelu_rows`` / ``test_swiglu_rows``: twice the
        largest error of torch's float32 CPU form over the same (real) lanes, one float32 unit of ``|ref|`` and the subnormal floor;
        the reference from the real lanes only, pad lanes exact zeros."""
        hidden, h_pad = self.plan.hidden, self.plan.h_pad
        x = call.args[0]
        self.wired(place, _same(x, fc1_out), "the input is not fc1's output")
        out, shape = call.out, (self.n, self.s, h_pad)
        if tuple(x.shape) != (self.n, self.s, 2 * h_pad if self.swiglu else h_pad) or tuple(out.shape) != shape or out.dtype != torch.float32:
            self.fail(place, f"{call.name}: {tuple(x.shape)} -> {tuple(out.shape)}, {out.dtype}")
            return out
        if self.swiglu:
            g32, v32 = x[..., :hidden], x[..., h_pad:h_pad + hidden]
            gate, value = g32.double(), v32.double()
            ref = gate / (1.0 + torch.exp(-gate)) * value
            e_torch = float(((F.silu(g32) * v32).double() - ref).abs().max())
            bound = 2.0 * e_torch + U32 * ref.abs() + TINY32 * (1.0 + (gate * value).abs())
        else:
            xd = x.double()
            ref = 0.5 * xd * torch.special.erfc(-xd / math.sqrt(2.0))  # test_gelu_rows's form: without float64's own cancellation
            e_torch = float((F.gelu(x).double() - ref).abs().max())
            bound = 2.0 * e_torch + U32 * ref.abs() + TINY32
        self.gate(place, call.name, out[..., :hidden], ref, bound)
        self.zeros(place, call.name, out[..., hidden:])
        return out


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
    route: str | None = None  # "int8" / "resid32" / "split" (``fp8=True`` is the FP8 route)


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
    # the three later routes: depth 2 throughout, s = 17 (partial tiles everywhere) and s = 197 (three key tiles and a tail of 5)
    ls, plain = (lambda: tiny_vit(layer_scale=True)), (lambda: tiny_vit(layer_scale=False))
    reg, v1, v2 = (lambda: tiny_foundation(TINY_REG)), (lambda: tiny_virchow(TINY_V1)), (lambda: tiny_virchow(TINY_V2))
    forms += [Form("resid32-tiny-ls-n3-64x64", ls, 3, (64, 64), both, route="resid32"),
              Form("resid32-tiny-plain-n2-224x224", plain, 2, (224, 224), both, route="resid32"),
              Form("resid32-tiny-ls-n3-48x64", ls, 3, (48, 64), both, route="resid32"),  # resampled, not square
              Form("resid32-reg-n3-42x56", reg, 3, (42, 56), both, route="resid32"),
              Form("resid32-v1-n2-28x28", v1, 2, (28, 28), both, route="resid32"),  # the native grid; token_mean
              Form("resid32-v2-n3-42x56", v2, 3, (42, 56), both, route="resid32"),  # the host-folded prefix on a resampled grid
              Form("resid32-u8-tiny-n2-64x64", tiny_vit, 2, (64, 64), both, hook="vit_small_patch16_224", route="resid32")]
    forms += [Form("int8-small-n3-64x64", small, 3, (64, 64), bf16, route="int8"),
              Form("int8-small-n2-224x224", small, 2, (224, 224), bf16, route="int8"),
              Form("int8-reg4-n3-42x56", lambda: tiny_foundation({**TINY_REG, "reg_tokens": 4}), 3, (42, 56), bf16, route="int8"),
              Form("int8-v2-n2-28x28", v2, 2, (28, 28), bf16, route="int8"),  # qkv stays half, H goes to 640
              Form("int8-mlp576-n2-64x64", lambda: tiny_vit(mlp_dim=576), 2, (64, 64), bf16, route="int8"),  # fc2 and its activation stay half
              Form("int8-u8-small-n2-64x64", small, 2, (64, 64), bf16, hook="vit_small_patch16_224", route="int8")]
    f32 = (torch.float32,)
    forms += [Form("split-tiny-ls-n3-64x64", ls, 3, (64, 64), f32, route="split"),
              Form("split-tiny-plain-n2-224x224", plain, 2, (224, 224), f32, route="split"),
              Form("split-tiny-ls-n3-48x64", ls, 3, (48, 64), f32, route="split"),
              Form("split-reg-n3-42x56", reg, 3, (42, 56), f32, route="split"),
              Form("split-v2-n2-28x28", v2, 2, (28, 28), f32, route="split"),  # most layers on the float32 GEMM, head_dim 80, 576 lanes
              # test_vit_f32_gpu's `v2-all-split`: every Linear on the split kernel's multiple, at 80 per head
              Form("split-v2-all-split-n2-28x28", lambda: tiny_virchow(TINY_V2, embed_dim=640, num_heads=8, mlp_dim=1280), 2, (28, 28), f32,
                   route="split")]
    return forms


FORMS = _forms()
CASES = [(form, dtype) for form in FORMS for dtype in form.dtypes]
DTYPE_IDS = {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "f32"}
CASE_IDS = [f"{form.ident}-{DTYPE_IDS[dtype]}" for form, dtype in CASES]

def form_input(form: Form) -> tuple[torch.Tensor, torch.Tensor | None]:
    """``(the NHWC batch, the hook's float32 table or None)``: normal draws, or -- for the uint8 entrance -- noise with every byte value
    in every channel."""
    n, (h, w) = form.n, form.size
    if form.hook is None:
        return torch.randn((n, h, w, 3), generator=torch.Generator().manual_seed(h + w + n)), None
    from _vit_classifier_ref import all_bytes_batch

    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    return torch.from_numpy(all_bytes_batch(n, h, w, seed=h + w)), timm_preproc_func(form.hook).table


def fused_graph(vit, dtype: torch.dtype, *, fp8: bool = False, route: str | None = None, device: str):
    import copy

    from tiatoolbox_amd.models.architecture.vit_fused import FP8_LINEAR, INT8_LINEAR, RESIDUAL_F32, SPLIT_LINEAR, FusedViT

    route = route or ("fp8" if fp8 else None)
    fused = FusedViT(copy.deepcopy(vit).to(device))
    if route == "split":
        fused.prepare(torch.float32, linear_dtype=SPLIT_LINEAR)
        return fused
    fused.prepare(dtype, linear_dtype={"fp8": FP8_LINEAR, "int8": INT8_LINEAR}.get(route),
                  residual_dtype=RESIDUAL_F32 if route == "resid32" else None)
    return fused.to(dtype)


def run_graph(fused, x: torch.Tensor, table32: torch.Tensor | None, dtype: torch.dtype, device: str) -> torch.Tensor:
    with torch.no_grad():
        if table32 is not None:
            return fused.forward_uint8(x.to(device), table32.to(dtype).to(device))
        return fused(x.to(device).permute(0, 3, 1, 2))

"""The stage trace of the ``FusedViT`` graphs without a GPU: the graph runs on torch stand-ins of every wrapper, the recorder wraps
them, and ``_vit_trace_ref.TraceChecker`` holds every stage to its float64 reference.  (a) Faithful stand-ins pass every stage of every
model form the GPU test runs: the checker is not trigger-happy.  (b) Each fault of a list, injected one at a time, fails at its own
stage: the checker is not vacuous -- and beside each the end-to-end criterion of the graph-level tests is printed, which lets most of
them through."""

from __future__ import annotations

import copy
import itertools
from typing import NamedTuple

import pytest
import torch

from _vit_classifier_ref import torch_vit_wrappers
from _vit_f32_ref import torch_f32_wrappers
from _vit_fp8_ref import fake_quantised_module, rel_error
from _vit_int8_ref import fake_quantised_module as fake_quantised_module_int8
from _vit_int8_ref import torch_int8_wrappers
from _vit_ref import tiny_vit
from _vit_resid32_ref import autocast_features, ref64, torch_resid32_wrappers
from _vit_trace_ref import (CASE_IDS, CASES, F32_FLOOR, StageFailure, TraceChecker, form_input, fp8_rule, fused_graph, plan_of, record,
                            run_graph, table_lines, torch_fp8_wrappers)
from _vit_virchow_ref import TINY_V1, TINY_V2, tiny_virchow

BF16 = torch.bfloat16


def _stand_ins(monkeypatch, serves=fp8_rule):
    from tiatoolbox_amd.models.architecture import vit_fused

    for name, fn in {**torch_vit_wrappers({}), **torch_fp8_wrappers(serves), **torch_int8_wrappers(), **torch_resid32_wrappers(),
                     **torch_f32_wrappers()}.items():
        monkeypatch.setattr(vit_fused, name, fn)
    return vit_fused


# ------------------------------------------------------------------------------------------------- (a) faithful stand-ins pass
@pytest.mark.parametrize(("form", "dtype"), CASES, ids=CASE_IDS)
def test_faithful_stand_ins_pass_every_stage(form, dtype, monkeypatch):
    vit_fused = _stand_ins(monkeypatch)
    vit = form.build()
    x, table32 = form_input(form)
    fused = fused_graph(vit, dtype, fp8=form.fp8, route=form.route, device="cpu")
    trace = record(monkeypatch, vit_fused)
    got = run_graph(fused, x, table32, dtype, "cpu")
    assert torch.equal(got, trace[-1].out)  # what the graph returns is the last stage's result
    rows = TraceChecker(vit, trace, x, dtype, fp8=form.fp8, route=form.route, table32=table32).check()
    print("\n".join(table_lines(f"stand-ins {form.ident} {dtype}", rows)))
    assert [place for place, _, _ in rows] == [place for place, _ in plan_of(vit, uint8=table32 is not None, fp8=form.fp8, route=form.route).stages]
    assert all(ratio <= 1.0 for _, _, ratio in rows)


def test_the_plan_takes_the_documented_routes():
    """``mlp_dim = 576``: the half GELU in front of a half ``fc2``, the quantising LayerNorm in front of ``qkv`` and ``fc1``; the
    Virchow2 form: ``qkv`` and ``fc1`` (K = 320) stay half, the SwiGLU half goes 520 -> 544 -> 640 and ``fc2`` (K = 640) to FP8."""
    kinds = lambda plan: {place.split(".", 2)[2]: name for place, name in plan.stages if place.startswith("blocks.0.")}  # noqa: E731
    plan = plan_of(tiny_vit(mlp_dim=576), fp8=True)
    assert kinds(plan) == {"norm1": "hip_layernorm_rows_q8", "qkv": "hip_linear_fp8_rows", "attn": "hip_mha_fwd_h", "proj": "hip_linear_h",
                           "norm2": "hip_layernorm_rows_q8", "fc1": "hip_linear_fp8_rows", "act": "hip_gelu_rows_h_", "fc2": "hip_linear_h"}
    plan = plan_of(tiny_virchow(TINY_V2), fp8=True)
    assert (plan.hidden, plan.h_pad) == (520, 640) and plan.fp8 == {"qkv": False, "fc1": False, "fc2": True}
    assert kinds(plan)["norm1"] == kinds(plan)["norm2"] == "hip_layernorm_rows_h" and kinds(plan)["act"] == "hip_act_rows_q8"
    assert plan.stages[0][1] == "hip_vit_patchify_pad_h" and plan.stages[2][1] == "hip_vit_assemble_prefix_h"
    assert plan.stages[-1] == ("norm_pool", "hip_vit_cls_mean_pool_h")
    plan = plan_of(tiny_virchow(TINY_V1))
    assert (plan.hidden, plan.h_pad) == (520, 544) and not any(plan.fp8.values())
    assert plan_of(tiny_vit(), fp8=True) == plan_of(tiny_vit(), route="fp8")  # the keyword of before and the route are one thing
    _the_plans_of_the_three_later_routes()


def _the_plans_of_the_three_later_routes():
    """INT8 routes as FP8 does, with its own wrappers.  The float32 stream: ``hip_vit_assemble_rows_f32`` first, the adding LayerNorm in
    every per-block place and at the end (or the float32 pool), the GEMMs, attention and activation the half graph's, and no padding
    beyond the half graph's (520 -> 544).  The float32 route: the ``_f32`` wrappers throughout, 520 -> 544 -> 576 because ``fc1`` at 1088
    is off 128, and per layer the GEMM that ``cin % 16 == 0 and cout % 128 == 0`` names."""
    kinds = lambda plan: {place.split(".", 2)[2]: name for place, name in plan.stages if place.startswith("blocks.1.")}  # noqa: E731
    plan = plan_of(tiny_vit(mlp_dim=576), route="int8")
    assert kinds(plan) == {"norm1": "hip_layernorm_rows_qi8", "qkv": "hip_linear_int8_rows", "attn": "hip_mha_fwd_h", "proj": "hip_linear_h",
                           "norm2": "hip_layernorm_rows_qi8", "fc1": "hip_linear_int8_rows", "act": "hip_gelu_rows_h_", "fc2": "hip_linear_h"}
    assert plan.stages[1] == ("patch_embed.proj", "hip_linear_h") and plan.stages[-1] == ("norm", "hip_layernorm_rows_h")
    plan = plan_of(tiny_virchow(TINY_V2), route="int8")
    assert (plan.hidden, plan.h_pad) == (520, 640) and plan.fp8 == {"qkv": False, "fc1": False, "fc2": True}
    assert kinds(plan)["norm1"] == kinds(plan)["norm2"] == "hip_layernorm_rows_h" and kinds(plan)["act"] == "hip_act_rows_qi8"
    assert kinds(plan)["fc2"] == "hip_linear_int8_rows" and kinds(plan)["fc1"] == "hip_linear_h"

    plan = plan_of(tiny_virchow(TINY_V2), route="resid32")
    assert (plan.hidden, plan.h_pad) == (520, 544) and not any(plan.fp8.values())
    assert [name for _, name in plan.stages[:3]] == ["hip_vit_patchify_pad_h", "hip_linear_h", "hip_vit_assemble_rows_f32"]
    assert kinds(plan) == {"norm1": "hip_add_layernorm_rows_f32", "qkv": "hip_linear_h", "attn": "hip_mha_fwd_h", "proj": "hip_linear_h",
                           "norm2": "hip_add_layernorm_rows_f32", "fc1": "hip_linear_h", "act": "hip_swiglu_rows_h", "fc2": "hip_linear_h"}
    assert plan.stages[-1] == ("norm_pool", "hip_vit_cls_mean_pool_f32")
    plan = plan_of(tiny_vit(), uint8=True, route="resid32")
    assert plan.stages[0][1] == "hip_vit_patchify_norm_u8_h" and plan.stages[-1] == ("norm", "hip_add_layernorm_rows_f32")

    plan = plan_of(tiny_virchow(TINY_V2), route="split")
    assert (plan.hidden, plan.h_pad) == (520, 576)  # fc1 carries 1152 channels
    assert plan.split == {"patch": False, "qkv": False, "proj": False, "fc1": True, "fc2": False}  # 320 and 960 are off 128
    assert [name for _, name in plan.stages[:3]] == ["hip_vit_patchify_f32", "hip_linear_f32", "hip_vit_assemble_f32"]
    assert kinds(plan) == {"norm1": "hip_add_layernorm_rows_f32", "qkv": "hip_linear_f32", "attn": "hip_mha_fwd_f32", "proj": "hip_linear_f32",
                           "norm2": "hip_add_layernorm_rows_f32", "fc1": "hip_linear_f32", "act": "hip_swiglu_rows_f32", "fc2": "hip_linear_f32"}
    assert plan.stages[-1] == ("norm_pool", "hip_vit_cls_mean_pool_f32")
    plan = plan_of(tiny_virchow(TINY_V2, embed_dim=640, num_heads=8, mlp_dim=1280), route="split")
    assert (plan.hidden, plan.h_pad) == (640, 640) and all(plan.split.values())
    plan = plan_of(tiny_vit(), route="split")
    assert all(plan.split.values()) and kinds(plan)["act"] == "hip_gelu_rows_f32_" and plan.stages[-1] == ("norm", "hip_add_layernorm_rows_f32")
    plan = plan_of(tiny_virchow(TINY_V1, mlp_dim=1024), route="split")
    assert (plan.hidden, plan.h_pad) == (512, 512)  # fc1 at 1024 is on 128: nothing is padded


# ------------------------------------------------------------------------------------------ (b) every listed fault fails, at its stage
def _on_calls(monkeypatch, vit_fused, name: str, which: set, change) -> None:
    """Replace the results of the calls numbered ``which`` (in call order) of the installed ``name`` by ``change(result)``."""
    fn, count = getattr(vit_fused, name), itertools.count()

    def wrapper(*args, **kwargs):
        out = fn(*args, **kwargs)
        return change(out) if next(count) in which else out

    monkeypatch.setattr(vit_fused, name, wrapper)


def _keep_row0(out):
    out[:, 1:] = 0
    return out


def _last_tokens_from_image0(out):
    out[:, -5:] = out[:1, -5:].clone()
    return out


# the half GEMM's calls of a depth-2 GELU model, in order: patch, then qkv, proj, fc1, fc2 of block 0 (1 .. 4) and of block 1 (5 .. 8)
def _last_block_rows(monkeypatch, vit_fused):
    _on_calls(monkeypatch, vit_fused, "hip_linear_h", {6, 7, 8}, _keep_row0)
    _on_calls(monkeypatch, vit_fused, "hip_gelu_rows_h_", {1}, _keep_row0)


def _attention_rows(monkeypatch, vit_fused):
    _on_calls(monkeypatch, vit_fused, "hip_mha_fwd_h", {0}, _last_tokens_from_image0)


def _no_qkv_bias(fused, vit):  # noqa: ARG001
    fused.layers[1]["qkv"].bias32 = torch.zeros_like(fused.layers[1]["qkv"].bias32)


def _no_norm2_beta(fused, vit):  # noqa: ARG001
    gamma, beta = fused.layers[1]["norm2"]
    fused.layers[1]["norm2"] = (gamma, torch.zeros_like(beta))


def _scale_of_80(fused, vit):  # noqa: ARG001
    fused.scale = 80 ** -0.5


def _fold_without_bias(fused, vit):
    fused.layers[0]["proj"].bias32 = vit.blocks[0].attn.proj.bias.detach().float().clone()


def _pad_lane_bias(fused, vit):  # noqa: ARG001
    fused.layers[0]["fc1"].bias32[520] = 0.5  # the first pad lane of the gate half (520 real lanes of 544)


def _residual_from_block_input(monkeypatch, vit_fused):
    fn, state = vit_fused.hip_linear_h, {"calls": 0}

    def wrapper(x, w, bias, residual=None, *, cout):
        i, state["calls"] = state["calls"], state["calls"] + 1
        if i == 2:  # noqa: PLR2004  (block 0's proj: its residual is the block's input)
            state["x"] = residual
        if i == 4:  # noqa: PLR2004  (block 0's fc2)
            residual = state["x"]
        return fn(x, w, bias, residual, cout=cout)

    monkeypatch.setattr(vit_fused, "hip_linear_h", wrapper)


def _skip_of_1(monkeypatch, vit_fused):
    fn = vit_fused.hip_vit_cls_mean_pool_h
    monkeypatch.setattr(vit_fused, "hip_vit_cls_mean_pool_h", lambda x, gamma, beta, *, eps, skip: fn(x, gamma, beta, eps=eps, skip=1))  # noqa: ARG005


def _with_args(monkeypatch, vit_fused, name: str, which: int, change, result=None) -> None:
    """Call number ``which`` of the installed ``name`` gets ``change(args, kwargs) -> (args, kwargs)`` (and its result ``result(out,
    args, kwargs)``).  Installed after ``record`` the recorder sees the changed arguments (the graph's wiring is wrong); installed
    before it the recorder sees the graph's own and a stand-in that does something else (the kernel is wrong)."""
    fn, count = getattr(vit_fused, name), itertools.count()

    def wrapper(*args, **kwargs):
        if next(count) != which:
            return fn(*args, **kwargs)
        args, kwargs = change(args, kwargs)
        out = fn(*args, **kwargs)
        return out if result is None else result(out, args, kwargs)

    monkeypatch.setattr(vit_fused, name, wrapper)


# hip_add_layernorm_rows_f32's calls of a depth-2 model without token_mean, in order: blocks.0.norm1, blocks.0.norm2 (1), blocks.1.norm1
# (2), blocks.1.norm2 (3), the final norm over the class rows (4); hip_linear_h's / hip_linear_f32's as above the first list
def _last_branch_not_added(monkeypatch, vit_fused):  # the kernel normalises the class rows and leaves them without the last fc2 branch
    _with_args(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32", 4, lambda args, kw: ((args[0], None, *args[2:]), kw))


def _branch_added_twice(monkeypatch, vit_fused):
    def twice(args, kw):
        args[0].add_(args[1].float())
        return args, kw

    _with_args(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32", 1, twice)


def _final_pass_over_every_row(monkeypatch, vit_fused):
    def every_row(args, kw):
        n, s, d = args[0].shape
        return args, {**kw, "rows": n * s, "row_stride": d}

    _with_args(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32", 4, every_row,
               result=lambda out, args, kw: out.view(*args[0].shape)[:, 0].contiguous())  # (the graph still returns [n, D])  # noqa: ARG005


def _proj_with_a_residual(monkeypatch, vit_fused):
    _with_args(monkeypatch, vit_fused, "hip_linear_h", 2, lambda args, kw: ((*args[:3], args[0]), kw))


def _stream_rounded_between_blocks(monkeypatch, vit_fused):
    def rounded(args, kw):
        args[0].copy_(args[0].to(kw["dtype"]).float())
        return args, kw

    _with_args(monkeypatch, vit_fused, "hip_add_layernorm_rows_f32", 2, rounded)


def _one_scale_off(out):
    out.scales[7] *= 1.0 + 2.0 ** -10
    return out


def _code_in_a_pad_lane(out):
    out.codes[1, 3, 600] = 1  # 520 real lanes of 640
    return out


def _code_of_minus_128(out):
    out.codes[2, 5, 17] = -128
    return out


def _int8_fc2_residual_from_block_input(monkeypatch, vit_fused):
    state = {}

    def keep(args, kw):
        state["x"] = args[3]  # block 0's proj: its residual is the block's input
        return args, kw

    _with_args(monkeypatch, vit_fused, "hip_linear_h", 1, keep)  # (the patch GEMM is call 0; qkv is on the INT8 GEMM)
    _with_args(monkeypatch, vit_fused, "hip_linear_int8_rows", 2, lambda args, kw: ((*args[:3], state["x"]), kw))  # block 0's fc2


def _weights_per_tensor(monkeypatch, vit_fused):
    """``pack_linear_weights_int8`` with ONE scale for the whole matrix, ``max |W| / 127``, in every channel's place."""
    from tiatoolbox_amd.models.architecture.vit_fused import QuantRows, quantize_rows_int8

    def pack(weight):
        w = weight.detach().float()
        q, s = quantize_rows_int8(w.reshape(1, -1))
        return QuantRows(q.reshape(w.shape), s.expand(w.shape[0]).contiguous())

    monkeypatch.setattr(vit_fused, "pack_linear_weights_int8", pack)


def _outlier_channel(vit):
    """One weight of ``blocks.0.attn.qkv`` at 64 times the largest: per tensor, every other channel's step grows 64-fold."""
    with torch.no_grad():
        w = vit.blocks[0].attn.qkv.weight
        w[5, 9] = 64.0 * float(w.abs().max())
    return vit


def _only_the_hi_plane(monkeypatch, vit_fused):  # block 1's qkv multiplies by the first of the three bf16 planes alone
    _with_args(monkeypatch, vit_fused, "hip_linear_f32", 5, lambda args, kw: ((args[0], args[1][:1], *args[2:]), kw))


def _f32_proj_without_residual(monkeypatch, vit_fused):
    _with_args(monkeypatch, vit_fused, "hip_linear_f32", 2, lambda args, kw: (args[:3], {k: v for k, v in kw.items() if k != "residual"}))


def _scale_of_64(fused, vit):  # noqa: ARG001
    fused.scale = 64 ** -0.5


def _qkv_on_the_other_gemm(monkeypatch, vit_fused):
    fn = vit_fused.pack_linear_weights_split
    monkeypatch.setattr(vit_fused, "pack_linear_weights_split", lambda w: None if w.shape[0] == 384 else fn(w))  # noqa: PLR2004


def _lo_plane_dropped_in_packing(monkeypatch, vit_fused):
    """The operand packed from ``hi`` and ``mid`` alone: 2^-16 of the weight is missing, which the GEMM's gate of 1e-5 does not see."""
    fn = vit_fused.pack_linear_weights_split

    def pack(weight):
        planes = fn(weight)
        if planes is not None:
            planes[2] = 0
        return planes

    monkeypatch.setattr(vit_fused, "pack_linear_weights_split", pack)


def _f32_pad_lane_bias(fused, vit):  # noqa: ARG001
    fused.layers[0]["fc1"].bias32[530] = 0.5  # a pad lane of the gate half (520 real lanes of 576)


class Fault(NamedTuple):
    ident: str
    place: str           # where the checker has to name it
    build: object
    n: int
    size: tuple
    dtype: torch.dtype
    fp8: bool = False
    below: object = None   # (monkeypatch, vit_fused): wraps a stand-in under the recorder -- its RESULT is wrong
    edit: object = None    # (fused, vit): edits the built graph's plain attributes
    above: object = None   # (monkeypatch, vit_fused): wraps a recorded function -- its ARGUMENTS are wrong
    serves: object = fp8_rule
    route: str | None = None


_small = lambda: tiny_vit(embed_dim=128, num_heads=2, mlp_dim=512)  # noqa: E731
_v2 = lambda: tiny_virchow(TINY_V2)  # noqa: E731
F32 = torch.float32
ROUTE_FAULTS = [
    Fault("resid32-last-branch-not-added-to-the-class-rows", "norm", tiny_vit, 3, (64, 64), BF16, route="resid32", below=_last_branch_not_added),
    Fault("resid32-branch-added-twice", "blocks.0.norm2", tiny_vit, 3, (64, 64), BF16, route="resid32", below=_branch_added_twice),
    Fault("resid32-final-pass-over-every-row", "norm", tiny_vit, 3, (64, 64), BF16, route="resid32", above=_final_pass_over_every_row),
    Fault("resid32-proj-given-a-residual", "blocks.0.proj", tiny_vit, 3, (64, 64), BF16, route="resid32", above=_proj_with_a_residual),
    Fault("resid32-stream-rounded-between-blocks", "blocks.1.norm1", tiny_vit, 3, (64, 64), torch.float16, route="resid32",
          above=_stream_rounded_between_blocks),
    Fault("int8-one-scale-off-by-2^-10", "blocks.1.norm1", _small, 3, (64, 64), BF16, route="int8",
          below=lambda mp, m: _on_calls(mp, m, "hip_layernorm_rows_qi8", {2}, _one_scale_off)),
    Fault("int8-code-in-a-pad-lane", "blocks.0.act", _v2, 2, (28, 28), BF16, route="int8",
          below=lambda mp, m: _on_calls(mp, m, "hip_act_rows_qi8", {0}, _code_in_a_pad_lane)),
    Fault("int8-fc2-residual-from-block-input", "blocks.0.fc2", _small, 3, (64, 64), BF16, route="int8", above=_int8_fc2_residual_from_block_input),
    Fault("int8-code-of-minus-128", "blocks.0.norm2", _small, 3, (64, 64), BF16, route="int8",
          below=lambda mp, m: _on_calls(mp, m, "hip_layernorm_rows_qi8", {1}, _code_of_minus_128)),
    Fault("int8-weights-per-tensor", "blocks.0.qkv", _small, 3, (64, 64), BF16, route="int8", below=_weights_per_tensor),
    Fault("int8-weights-per-tensor-outlier-channel", "blocks.0.qkv", lambda: _outlier_channel(_small()), 3, (64, 64), BF16, route="int8",
          below=_weights_per_tensor),
    Fault("split-only-the-hi-plane", "blocks.1.qkv", tiny_vit, 3, (64, 64), F32, route="split", below=_only_the_hi_plane),
    Fault("split-proj-without-its-residual", "blocks.0.proj", tiny_vit, 3, (64, 64), F32, route="split", above=_f32_proj_without_residual),
    Fault("split-scale-of-64-at-head-dim-80", "blocks.0.attn", _v2, 2, (28, 28), F32, route="split", edit=_scale_of_64),
    Fault("split-qkv-on-the-float32-gemm", "blocks.0.qkv", tiny_vit, 3, (64, 64), F32, route="split", below=_qkv_on_the_other_gemm),
    Fault("split-pad-lane-bias", "blocks.0.fc1", _v2, 2, (28, 28), F32, route="split", edit=_f32_pad_lane_bias),
    Fault("split-lo-plane-dropped-in-packing", "patch_embed.proj", tiny_vit, 3, (64, 64), F32, route="split", below=_lo_plane_dropped_in_packing),
]
FAULTS = [
    Fault("last-block-rows-fp16", "blocks.1.proj", tiny_vit, 3, (64, 64), torch.float16, below=_last_block_rows),
    Fault("last-block-rows-bf16", "blocks.1.proj", tiny_vit, 3, (64, 64), BF16, below=_last_block_rows),
    Fault("last-block-rows-bf16-224", "blocks.1.proj", tiny_vit, 2, (224, 224), BF16, below=_last_block_rows),
    Fault("attention-rows-from-image0", "blocks.0.attn", tiny_vit, 2, (224, 224), BF16, below=_attention_rows),
    Fault("fp8-qkv-bias-dropped", "blocks.1.qkv", _small, 3, (64, 64), BF16, fp8=True, edit=_no_qkv_bias),
    Fault("fp8-norm2-beta-dropped", "blocks.1.norm2", _small, 3, (64, 64), BF16, fp8=True, edit=_no_norm2_beta),
    Fault("fp8-scale-of-80", "blocks.0.attn", _small, 3, (64, 64), BF16, fp8=True, edit=_scale_of_80),
    Fault("fp8-scale-of-80-224", "blocks.0.attn", _small, 2, (224, 224), BF16, fp8=True, edit=_scale_of_80),
    Fault("fold-without-bias", "blocks.0.proj", tiny_vit, 3, (64, 64), BF16, edit=_fold_without_bias),
    Fault("fc2-residual-from-block-input", "blocks.0.fc2", tiny_vit, 3, (64, 64), BF16, above=_residual_from_block_input),
    Fault("swiglu-pad-lane-bias", "blocks.0.fc1", lambda: tiny_virchow(TINY_V1), 2, (28, 28), BF16, edit=_pad_lane_bias),
    Fault("pool-skip-1", "norm_pool", lambda: tiny_virchow(TINY_V2), 2, (28, 28), BF16, above=_skip_of_1),
    Fault("fp8-fc2-off-its-shapes", "blocks.0.act", lambda: tiny_vit(mlp_dim=576), 2, (64, 64), BF16, fp8=True, serves=lambda cout, cin: True),  # noqa: ARG005
    *ROUTE_FAULTS,
]


def _output_criterion(fault, vit, x32: torch.Tensor, got: torch.Tensor) -> tuple[float, float, float]:
    """``(e_fault, e_yardstick, the gate)`` of the route's graph-level test on the same run: ``2 e_yard`` against the float32 module with
    the cast (or fake-quantised, or autocast) module as the yardstick; on the float32 route ``2 e_lib + 8 * 2^-24`` against float64."""
    dtype = fault.dtype
    with torch.no_grad():
        if fault.route == "split":
            ref, yard = ref64(vit, x32), vit(x32)
            return rel_error(got, ref), rel_error(yard, ref), 2.0 * rel_error(yard, ref) + F32_FLOOR
        ref = vit(x32)
        if fault.route == "resid32":
            yard = autocast_features(vit, x32, dtype, "cpu")
        elif fault.fp8 or fault.route == "int8":
            yard = (fake_quantised_module if fault.fp8 else fake_quantised_module_int8)(copy.deepcopy(vit))(x32.to(dtype)).float()
        else:
            yard = copy.deepcopy(vit).to(dtype)(x32.to(dtype)).float()
    return rel_error(got, ref), rel_error(yard, ref), 2.0 * rel_error(yard, ref)


@pytest.mark.parametrize("fault", FAULTS, ids=[f.ident for f in FAULTS])
def test_each_fault_fails_at_its_stage(fault, monkeypatch):
    vit_fused = _stand_ins(monkeypatch, fault.serves)
    vit, dtype = fault.build(), fault.dtype
    n, (h, w) = fault.n, fault.size
    x = torch.randn((n, h, w, 3), generator=torch.Generator().manual_seed(h + w + n))
    if fault.below is not None:
        fault.below(monkeypatch, vit_fused)
    fused = fused_graph(vit, dtype, fp8=fault.fp8, route=fault.route, device="cpu")
    if fault.edit is not None:
        fault.edit(fused, vit)
    trace = record(monkeypatch, vit_fused)
    if fault.above is not None:
        fault.above(monkeypatch, vit_fused)
    got = run_graph(fused, x, None, dtype, "cpu")
    # the graph-level tests' criterion on the same run: e against the float32 module beside the yardstick's, allowed a factor of 2
    e_fault, e_yard, gate = _output_criterion(fault, vit, x.permute(0, 3, 1, 2).contiguous(), got)
    with pytest.raises(StageFailure) as caught:
        TraceChecker(vit, trace, x, dtype, fp8=fault.fp8, route=fault.route).check()
    print(f"fault {fault.ident}: end to end e_fault {e_fault:.3e}  e_yardstick {e_yard:.3e}  ratio {e_fault / e_yard:.2f} "
          f"({'passes' if e_fault <= gate else 'caught by'} the output criterion); the trace: {caught.value}")
    assert caught.value.place == fault.place, str(caught.value)


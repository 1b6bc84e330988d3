"""Host-side references of the ``int8_smoothing`` tests: the smoothed yardstick (``_vit_int8_ref.fake_quantised_module`` with ``W * s``
in front of the weight fake-quantisation and ``x / s`` in front of the input fake-quantisation), a float64 column abs-max, torch
stand-ins of the new wrappers (any device), the calibration statistics of the bfloat16 graph from torch operations, and the two
outlier scenarios the option exists for."""

from __future__ import annotations

import copy

import torch

from _vit_int8_ref import fake_quantised_module, rel_error, torch_int8_wrappers  # noqa: F401  (shared with the test files)

LAYERS = ("qkv", "fc1", "fc2")
_PARENT = {"qkv": "attn", "fc1": "mlp", "fc2": "mlp"}


def routed_linears(module: torch.nn.Module, layers=LAYERS) -> dict[str, torch.nn.Linear]:
    """``blocks.{i}.attn.qkv`` / ``.mlp.fc1`` / ``.mlp.fc2`` (the graph's layer names) -> the module's Linear, for ``layers``."""
    out = {}
    for name, m in module.named_modules():
        parts = name.split(".")
        if isinstance(m, torch.nn.Linear) and len(parts) >= 4 and parts[-4] == "blocks" and parts[-1] in layers and parts[-2] == _PARENT[parts[-1]]:  # noqa: PLR2004
            out[".".join(parts[-4:])] = m
    return out


def smoothed_fake_quantised_module(module: torch.nn.Module, scales: dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16,
                                   layers=None) -> torch.nn.Module:
    """``module`` (float32, changed in place) as the smoothed INT8 graph's yardstick: every routed layer's weight columns times ``s``
    in float32 and its input divided by ``s`` (both exact: powers of two), then ``fake_quantised_module`` -- whose weight
    fake-quantisation so sees ``W * s`` and whose input hook, registered after the division's, sees ``x / s``.  An ``fc2`` entry at
    the graph's padded width is cut to the module's.  ``layers`` defaults to the kinds ``scales`` has entries for: what the graph routes."""
    layers = tuple(n for n in LAYERS if any(k.endswith("." + n) for k in scales)) if layers is None else layers
    targets = routed_linears(module, layers)
    assert targets and set(targets) <= set(scales), sorted(set(targets) - set(scales))
    for name, lin in targets.items():
        s = scales[name].to(lin.weight.device, torch.float32)[:lin.in_features]
        assert s.numel() == lin.in_features
        with torch.no_grad():
            lin.weight.mul_(s)
        lin.register_forward_pre_hook(lambda _mod, args, s=s: ((args[0].float() / s).to(args[0].dtype), *args[1:]))
    return fake_quantised_module(module, dtype, layers)


def absmax64(v: torch.Tensor) -> torch.Tensor:
    """``max_r |v[r, j]|`` per column in float64; a NaN in a column makes that column NaN."""
    return v.double().reshape(-1, v.shape[-1]).abs().amax(dim=0)


# ------------------------------------------------------------------------------------------------- torch stand-ins of the wrappers
def torch_smooth_wrappers() -> dict:
    """Torch restatements of the wrappers smoothing adds, for any device: the smoothed producer multiplies the float32 activation by
    ``inv_smooth`` before ``quantize_rows_int8``; the statistics are column maxima of the float32 values the producers hold."""
    import torch.nn.functional as F  # noqa: N812

    from tiatoolbox_amd.models.architecture.vit_fused import QuantRows, quantize_rows_int8

    def act32(x, swiglu):
        if swiglu:
            gate, value = x.float().chunk(2, -1)
            return F.silu(gate) * value
        return F.gelu(x.float())

    def act_smooth(x, inv_smooth, *, swiglu):
        q, s = quantize_rows_int8(act32(x, swiglu) * inv_smooth)
        return QuantRows(q, s.reshape(-1))

    def layernorm_absmax(x, gamma, beta, amax, *, eps):
        v = F.layer_norm(x.float(), (x.shape[-1],), gamma, beta, eps)
        return amax.copy_(torch.maximum(amax, v.reshape(-1, v.shape[-1]).abs().amax(dim=0)))

    def act_absmax(x, amax, *, swiglu):
        v = act32(x, swiglu)
        return amax.copy_(torch.maximum(amax, v.reshape(-1, v.shape[-1]).abs().amax(dim=0)))

    return {"hip_act_rows_qi8_smooth": act_smooth, "hip_layernorm_rows_absmax_h": layernorm_absmax, "hip_act_rows_absmax_h": act_absmax}


def reference_calibration(vit: torch.nn.Module, batches, alpha: float = 0.5) -> tuple[dict, dict, dict]:
    """``calibrate_int8_smoothing`` with every wrapper of the bfloat16 graph replaced by its torch restatement (the half ones of
    ``_vit_classifier_ref``, the statistics above), on the module's own device: ``(scales, amax_x, amax_w)`` per layer name."""
    import pytest

    from _vit_classifier_ref import torch_vit_wrappers

    from tiatoolbox_amd.models.architecture import vit_fused

    seen = {}
    begin = vit_fused.FusedViT.begin_int8_calibration

    def begin_and_keep(self):
        begin(self)
        seen["graph"] = self

    with pytest.MonkeyPatch.context() as mp:
        for name, fn in {**torch_vit_wrappers({}), **torch_int8_wrappers(), **torch_smooth_wrappers()}.items():
            mp.setattr(vit_fused, name, fn)
        mp.setattr(vit_fused.FusedViT, "begin_int8_calibration", begin_and_keep)
        scales = vit_fused.calibrate_int8_smoothing(vit, batches, alpha=alpha)
    graph = seen["graph"]
    return scales, {k: v.detach().cpu().clone() for k, v in graph._taps.items()}, dict(graph._amax_w)  # noqa: SLF001


# ------------------------------------------------------------------------------------------------------- the outlier scenarios
def add_outliers(vit: torch.nn.Module, scenario: str, *, channel: int = 5, hidden_channel: int = 7) -> torch.nn.Module:
    """``vit`` (changed in place) with the activations the option exists for.  (A): in every block, channel ``channel`` of ``norm1``
    and of ``norm2`` has weight and bias x 60 and the next layer's (``qkv`` / ``fc1``) weight column / 60 -- the module's function is
    unchanged, one LayerNorm output channel is 60 x the rest.  (B): A, and ``fc1``'s output channel ``hidden_channel`` x 30 (weight row
    and bias; of a packed SwiGLU the value half's) with ``fc2``'s column / 30."""
    assert scenario in ("A", "B")
    with torch.no_grad():
        for blk in vit.blocks:
            for norm, lin in ((blk.norm1, blk.attn.qkv), (blk.norm2, blk.mlp.fc1)):
                norm.weight[channel] *= 60.0
                norm.bias[channel] *= 60.0
                lin.weight[:, channel] /= 60.0
            if scenario == "B":
                row = hidden_channel + (blk.mlp.fc2.in_features if blk.mlp.fc1.out_features == 2 * blk.mlp.fc2.in_features else 0)
                blk.mlp.fc1.weight[row] *= 30.0
                blk.mlp.fc1.bias[row] *= 30.0
                blk.mlp.fc2.weight[:, hidden_channel] /= 30.0
    return vit


def with_outliers(vit: torch.nn.Module, scenario: str) -> torch.nn.Module:
    return add_outliers(copy.deepcopy(vit), scenario)


# ------------------------------------------------------------------------------------------------------- the calibration case
def calibration_case() -> tuple[torch.nn.Module, list[torch.Tensor]]:
    """The model and the two calibration batches of the calibration tests (CPU and GPU): scenario B on the tiny model at depth 2."""
    from _vit_ref import tiny_vit

    g = torch.Generator().manual_seed(31)
    return with_outliers(tiny_vit(seed=3), "B"), [torch.randn((5, 3, 64, 64), generator=g), torch.randn((3, 3, 64, 64), generator=g)]


def near_tie_columns(amax_x: torch.Tensor, amax_w: torch.Tensor, alpha: float, within: float = 1e-3) -> torch.Tensor:
    """The columns whose real exponent ``alpha log2 a - (1 - alpha) log2 w`` sits within ``within`` of a rounding tie (``k + 1/2``): the
    only ones where statistics that differ in their last bits may round to neighbouring powers of two."""
    a, w = amax_x.double(), amax_w.double()
    live = (a > 0) & (w > 0)
    e = alpha * torch.log2(torch.where(live, a, torch.ones_like(a))) - (1.0 - alpha) * torch.log2(torch.where(live, w, torch.ones_like(w)))
    return live & ((e - torch.floor(e) - 0.5).abs() <= within)

"""References shared by ``test_unet_half.py`` (host) and ``test_unet_half_gpu.py`` (``-m gpu``): what the half-precision glue
kernels of the UNet compute, stated with plain torch ops on the CPU, and the seeded network the graph / engine tests use.

* upsample-add (``tia_upsample2x_add_act_nhwc_h``): float32 arithmetic, every step rounded on its own --
  ``s = float(x) + float(y)``, ``p = s * scale``, ``a = p + shift``, ``max(a, 0)`` -- then ONE rounding to half.  Two
  deliberately WRONG variants (a fused multiply-add; ``s`` rounded to half before the affine) exist so that the tests can show
  that their inputs tell the contract from its near misses.
* head (``tia_conv1x1_head_nhwc_h``): float64 ``bias + sum_c w * pre(x)`` on the half inputs themselves, with the bound of a
  64-term float32 dot product plus a bias.
* the graph: ``UNetModel(3, 5, "resnet50", decoder_block=[3, 3])`` with RANDOMISED BatchNorm statistics (seeded ones are
  identities and would hide every scale / shift mistake), its float32 CPU logits computed once per input.
"""

from __future__ import annotations

import functools

import torch

HALVES = (torch.float16, torch.bfloat16)
MANTISSA = {torch.float16: 10, torch.bfloat16: 7}  # explicit significand bits


def upsample_add_ref(x, y, scale=None, shift=None, *, variant: str = "contract"):
    """``x`` [n, c, h, w], ``y`` [n, c, 2h, 2w] of one half dtype, ``scale`` / ``shift`` float32 [c] or None; result in that dtype.
    ``variant``: ``"contract"`` (the kernel's specification), ``"fma"`` and ``"round_s"`` (the two wrong ones)."""
    dtype = x.dtype
    s = x.float().repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) + y.float()
    if scale is None:
        return s.to(dtype)
    sc, sh = scale.float()[None, :, None, None], shift.float()[None, :, None, None]
    if variant == "contract":
        p = s * sc
        a = p + sh
    elif variant == "fma":  # the product enters the sum unrounded (float64 holds the 48-bit product exactly)
        a = (s.double() * sc.double() + sh.double()).float()
    elif variant == "round_s":  # the sum goes through the half type before the affine
        p = s.to(dtype).float() * sc
        a = p + sh
    else:
        raise ValueError(variant)
    return torch.clamp_min(a, 0.0).to(dtype)


def hand_example(dtype):
    """One input pixel, 8 channels, worked by hand; returns ``(x, y, scale, shift, expected_act, expected_plain)``.

    With ``m`` the significand bits of the half type (10 / 7) and ``k = 24 - m``:
      ch 0: s = 1 + 2^-m; scale = 1 + 2^-k: the exact product 1 + 2^-m + 2^-k + 2^-24 is a float32 tie and rounds (to even) to
            1 + 2^-m + 2^-k; shift = -(1 + 2^-m) leaves exactly 2^-k.  A fused multiply-add keeps the 2^-24: 2^-k (1 + 2^-m), which the
            half type holds exactly -- another number.
      ch 1: x = 1, y = 2^-(m+1): s = 1 + 2^-(m+1) is exact in float32 but a tie in the half type (rounds to 1); scale 1, shift -1 give
            2^-(m+1).  Rounding s to half first gives 0.  Without the affine the output is that tie: 1.
      ch 2: (-3 + 1) * 2 + 1 = -3 -> 0 (the ReLU cuts)         ch 3: (0.5 + 0.25) * 4 - 1 = 2
      ch 4: (2 - 2) * 5 + 0.125 = 0.125                        ch 5: (1.5 + 1.5) * -1 + 3 = 0
      ch 6: (3 + 4) * 0.5 + 0.25 = 3.75                        ch 7: (-1 - 1) * -0.5 + 0 = 1
    """
    m = MANTISSA[dtype]
    k = 24 - m
    xs = [1.0, 1.0, -3.0, 0.5, 2.0, 1.5, 3.0, -1.0]
    ys = [2.0 ** -m, 2.0 ** -(m + 1), 1.0, 0.25, -2.0, 1.5, 4.0, -1.0]
    sc = [1.0 + 2.0 ** -k, 1.0, 2.0, 4.0, 5.0, -1.0, 0.5, -0.5]
    sh = [-(1.0 + 2.0 ** -m), -1.0, 1.0, -1.0, 0.125, 3.0, 0.25, 0.0]
    act = [2.0 ** -k, 2.0 ** -(m + 1), 0.0, 2.0, 0.125, 0.0, 3.75, 1.0]
    plain = [1.0 + 2.0 ** -m, 1.0, -2.0, 0.75, 0.0, 3.0, 7.0, -2.0]
    x = torch.tensor(xs, dtype=torch.float64).to(dtype).view(1, 8, 1, 1)
    y = torch.tensor(ys, dtype=torch.float64).to(dtype).view(1, 8, 1, 1).expand(1, 8, 2, 2).contiguous()
    assert x.double().flatten().tolist() == xs and y[0, :, 0, 0].double().tolist() == ys  # the inputs are half numbers as written
    scale, shift = torch.tensor(sc, dtype=torch.float64).float(), torch.tensor(sh, dtype=torch.float64).float()
    assert scale.double().tolist() == sc and shift.double().tolist() == sh  # and the affine float32 numbers
    expand = lambda v: torch.tensor(v, dtype=torch.float64).view(1, 8, 1, 1).expand(1, 8, 2, 2)  # noqa: E731
    return x, y, scale, shift, expand(act), expand(plain)


def head_ref(x, weight, bias, pre_scale=None, pre_shift=None):
    """float64 head on the half inputs themselves: ``x`` [npix, 64] half, ``weight`` [cout, 64], ``bias`` [cout] float32 -> (value, bound)
    with ``bound = 66 * 2^-24 * (sum_c |w * pre(x)| + |bias|)`` per element: a 64-term float32 dot product plus a bias."""
    v = x.double()
    if pre_scale is not None:
        v = torch.clamp_min(v * pre_scale.double()[None] + pre_shift.double()[None], 0.0)
    w = weight.double()
    ref = v @ w.T + bias.double()[None]
    bound = 66 * 2.0 ** -24 * (v.abs() @ w.abs().T + bias.double().abs()[None])
    return ref, bound


def randomise_bn(model, seed: int):
    """The recipe of ``test_semantic.py::test_fused_unet_forward_matches_plain_module``."""
    g = torch.Generator().manual_seed(seed)
    for mod in model.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.05, generator=g)
            mod.running_var.uniform_(0.8, 1.2, generator=g)
            mod.weight.data.uniform_(0.8, 1.2, generator=g)
            mod.bias.data.normal_(0, 0.05, generator=g)
    return g


GRAPH_SHAPES = ((2, 3, 96, 128), (1, 3, 256, 320))


@functools.lru_cache(maxsize=1)
def graph_case():
    """``(model, [(x_float_nchw, ref_logits), ...])``: built and run on the CPU once per session; callers must not modify it."""
    from tiatoolbox_amd.models.architecture.unet import UNetModel

    torch.manual_seed(1)
    model = UNetModel(3, 5, "resnet50", decoder_block=[3, 3]).eval()
    g = randomise_bn(model, 5)
    cases = []
    with torch.inference_mode():
        for shape in GRAPH_SHAPES:
            x = torch.randint(0, 256, shape, generator=g).float()
            cases.append((x, model(x)))
    return model, cases


def rel_err(got, ref) -> float:
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.abs().max()), 1.0)

"""Inference copy of :class:`HoVerNet` / :class:`HoVerNetPlus` on the hand-written MFMA convolutions (float32; fp16 / bf16 after
``FusedHoVerNet.prepare(dtype)``, see there).

Same arithmetic graph as ``HoVerNet.forward`` (reference ``models/architecture/hovernet.py:405-454``), re-expressed so
that every convolution with ``cin % 32 == 0`` and ``cout % 64 == 0`` -- all 1x1 / 3x3 convolutions of the
pre-activation ResNet-50 encoder, the decoders' ``conva`` / ``convf`` and the dense units' 1x1 -- runs on
``tia_conv2d_nhwc_f32_ex`` with its epilogue fused:

* ``conv -> BN -> ReLU`` (``conv1`` / ``conv2`` of every unit, the stem): BN folded into the weights, bias + ReLU in the
  convolution's epilogue;
* ``conv3 + shortcut``: the residual add rides in the epilogue of ``conv3``;
* ``BN -> ReLU -> conv1`` (the pre-activation of residual units 2..n): applied to the operand while ``conv1`` loads it
  (``tia_conv1x1_pre_nhwc_f32``) -- the unit reads the previous raw sum, no activated copy exists in memory; ``blk_bna``
  (after the last unit) comes out of ``conv3``'s epilogue as its only output (``tia_conv2d_post_nhwc_f32``); the dense
  units' pre-activations are one ``tia_scale_shift_act_nhwc_f32`` pass;
* TensorFlow "same" padding of the strided 3x3: expressed by the convolution's explicit front padding / output size.

The other convolutions are hand-written too: the 3-channel 7x7 stem runs on the same MFMA kernel in its row-packed
thin-input form (``tia_conv2d_thin_nhwc_f32``), the dense units' grouped convolutions (32 -> 8 channels per group) on
``tia_grouped_conv_valid_nhwc_f32``, and the final ``BN -> ReLU -> 64 -> n_out`` 1x1 of every branch is one launch of
``tia_conv1x1_head_nhwc_f32``.  Built from a loaded model (reference parameter names), never the object that loads
weights; CUDA, channels-last only.  Which kernel a layer runs on, in float32 and in half, is `_Conv`'s to know and nobody else's.
"""

from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn.functional as F  # noqa: N812
from torch import nn

from tiatoolbox_amd.models.architecture.fused import (hip_bias_act_, hip_conv1x1_head, hip_conv1x1_pre, hip_conv2d_ex, hip_conv2d_h,
                                                      hip_conv2d_h_ex, hip_conv2d_post, hip_conv3x3_wino, pack_conv_weights_h,
                                                      pack_conv_weights_wino, hip_conv2d_thin, hip_grouped_conv_valid,
                                                      hip_grouped_conv_valid_h, hip_scale_shift_act, hip_scale_shift_act_view,
                                                      hip_upsample2x_add, pack_conv_weights, pack_grouped_conv_valid_weights_h,
                                                      pack_thin_conv_weights)
from tiatoolbox_amd.models.architecture.hovernet import centre_crop_to_shape
from tiatoolbox_amd.models.architecture.utils import centre_crop


def _cl(x: torch.Tensor) -> torch.Tensor:
    return x if x.is_contiguous(memory_format=torch.channels_last) else x.contiguous(memory_format=torch.channels_last)


def _bn_affine(bn: nn.BatchNorm2d) -> tuple[torch.Tensor, torch.Tensor]:
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float().contiguous()
    shift = (bn.bias - bn.running_mean * scale).detach().float().contiguous()
    return scale, shift


def _same_pads(size: int, ksize: int, stride: int) -> tuple[int, int]:
    """``TFSamepaddingLayer`` (ref. :30-69): total pad from the HEIGHT's remainder, smaller half in front."""
    rem = size % stride
    pad = max(ksize - (stride if rem == 0 else rem), 0)
    return pad // 2, pad - pad // 2


class _Conv(nn.Module):
    """One convolution of the graph (optionally with a following BN folded in) and the one owner of every kernel form of it: which
    kernel the layer runs on is fixed here, once (``route``), and so is which packed operands it holds in float32 and -- after
    ``prepare(dtype)`` -- in fp16 / bf16.  ``forward`` is the only way in.

    ===========  =========================================  ============================  =====================================
    ``route``    layer                                      float32                       fp16 / bf16 (``prepare``)
    ===========  =========================================  ============================  =====================================
    ``head``     1x1, 64 -> at most 8 channels              ``.weight``                   ``_weight32`` (float32 ``[cout, 64]``)
    ``thin``     cin * k <= 32 (the RGB stem)               ``_packed``                   ``_packed`` (float32; stride 1 only)
    ``grouped``  32 -> 8 channels per group, no bias        ``_packed``                   ``_packed_h`` (3x3 / 5x5)
    ``mfma``     cin % 32 == 0, cout % 64 == 0              ``_packed``, ``_wino``        ``_packed_h``
    ``torch``    anything else                              library convolution           refused (``TypeError``)
    ===========  =========================================  ============================  =====================================

    A call outside its kernel's form (a head with a ReLU, a grouped layer with padding) takes the library convolution in float32 and
    raises in half.  The bias is ``.bias`` in float32 and its float32 copy ``_bias32`` in half."""

    def __init__(self, conv: nn.Conv2d, bn: nn.BatchNorm2d | None = None) -> None:
        super().__init__()
        w = conv.weight.detach().float()
        bias = conv.bias.detach().float() if conv.bias is not None else None
        if bn is not None:
            scale, shift = _bn_affine(bn)
            w = w * scale[:, None, None, None]
            bias = shift if bias is None else bias * scale + shift
        self.kernel, self.stride = conv.kernel_size[0], conv.stride[0]
        self.mfma_ok = conv.groups == 1 and conv.in_channels % 32 == 0 and conv.out_channels % 64 == 0
        self.groups = conv.groups
        # few input channels (the RGB stem): row-packed form of the MFMA kernel; few output channels (a class head): the head kernel
        self.thin_ok = (conv.groups == 1 and conv.in_channels < 32 and conv.in_channels * conv.kernel_size[1] <= 32  # noqa: PLR2004
                        and conv.out_channels % 64 == 0 and conv.kernel_size[0] == conv.kernel_size[1])
        self.head_ok = (conv.groups == 1 and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.in_channels == 64  # noqa: PLR2004
                        and conv.out_channels <= 8)  # noqa: PLR2004
        # the dense units' grouped convolution: 32 -> 8 channels per group, stride 1, no bias
        self.grouped_ok = (conv.groups > 1 and conv.in_channels // conv.groups == 32 and conv.out_channels // conv.groups == 8
                           and conv.stride[0] == 1 and bias is None)
        # the four flags exclude one another (groups; cin < 32, == 64, % 32 == 0; cout <= 8, % 64 == 0)
        self.route = next((r for r in ("head", "thin", "grouped", "mfma") if getattr(self, r + "_ok")), "torch")
        self.weight = nn.Parameter(w.contiguous(), requires_grad=False)
        self.bias = nn.Parameter(bias.contiguous(), requires_grad=False) if bias is not None else None
        self._packed: torch.Tensor | None = None  # the route's float32 operand (`_operand`)
        # opt-in (`set_conv_algo(model, "winograd")`, engine kwarg `conv_algo`): plain 3x3 / stride-1 layers through the Winograd
        # F(2x2, 3x3) kernel (float32 in / float32 accumulate; csrc/conv3x3_wino.hip)
        self.conv_algo = "direct"
        self.wino_ok = self.mfma_ok and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.dilation == (1, 1)
        self._wino: torch.Tensor | None = None
        # half-precision form (`prepare`): plain attributes, so that casting the module leaves them as they are
        self.half_dtype: torch.dtype | None = None
        self._packed_h: torch.Tensor | None = None   # halves: [kh, kw, cin/8, cout, 8] (mfma), [groups, k, k, 4, 8, 8] (grouped)
        self._weight32: torch.Tensor | None = None   # [cout, 64] float32 (class heads)
        self._bias32: torch.Tensor | None = None

    def prepare(self, dtype: torch.dtype) -> None:
        """Switch this convolution to fp16 / bf16 activations on the half form of its kernel (``tia_conv2d_nhwc_h(_ex)``,
        ``tia_conv1x1_head_nhwc_h``, ``tia_grouped_conv_valid_nhwc_h``, ``tia_conv2d_thin_nhwc``) -- call it on the device BEFORE the
        module is cast: the operands are packed NOW from the float32, BN-folded parameters (one rounding to half, after the folding;
        the head's and the thin kernel's stay float32), never again from the cast ones, and the bias stays float32 in a plain
        attribute that ``module.to(dtype)`` does not touch.  ``torch.float32`` switches back.  A layer without a half kernel raises
        ``TypeError``: there is no library fall-back in half precision (``conv_algo`` has no effect there either: no Winograd form
        in half)."""
        if dtype == torch.float32:
            self.half_dtype = self._packed_h = self._weight32 = self._bias32 = None
            return
        if dtype not in (torch.float16, torch.bfloat16) or self.weight.dtype != torch.float32:
            msg = f"_Conv.prepare packs float32 parameters for fp16 / bf16; got {self.weight.dtype} parameters for {dtype}."
            raise ValueError(msg)
        if self.route == "head":
            self._weight32 = self.weight.detach().reshape(self.weight.shape[0], 64).clone().contiguous()
        elif self.route == "mfma":
            self._packed_h = pack_conv_weights_h(self, dtype)  # reads `.weight` (OIHW, BN folded, float32)
        elif self.route == "grouped" and self.kernel in (3, 5):
            self._packed_h = pack_grouped_conv_valid_weights_h(self.weight, self.groups, dtype)
        elif self.route == "thin" and self.stride == 1:
            self._packed = pack_thin_conv_weights(self.weight)  # float32 arithmetic; the output is written in `dtype`
        else:
            msg = (f"no {dtype} kernel for a convolution {tuple(self.weight.shape)} with groups = {self.groups}, stride {self.stride}: "
                   "tia_conv2d_nhwc_h takes cin % 32 == 0 and cout % 64 == 0, tia_conv1x1_head_nhwc_h 64 -> at most 8 channels, "
                   "tia_grouped_conv_valid_nhwc_h 32 -> 8 channels per group, 3x3 or 5x5, stride 1, no bias, tia_conv2d_thin_nhwc "
                   "c * k <= 32, cout % 64 == 0, stride 1.")
            raise TypeError(msg)
        self._bias32 = self.bias.detach().clone().contiguous() if self.bias is not None else None
        self.half_dtype = dtype

    @property
    def activates_on_load(self) -> bool:
        """Whether ``forward(pre=...)`` applies the BN + ReLU to the operand while the kernel loads it (``tia_conv1x1_pre_nhwc_f32``:
        float32 1x1 MFMA layers; the half kernel fills its LDS by DMA and cannot)."""
        return self.route == "mfma" and self.kernel == 1 and self.half_dtype is None

    def _operand(self) -> torch.Tensor:
        """The packed weights of this layer's kernel.  A prepared layer holds them since ``prepare`` (its parameters have been rounded
        by the cast); an unprepared float32 one packs them on first use, and again after a move to another device."""
        if self.half_dtype is not None:
            return self._packed if self.route == "thin" else self._packed_h
        if self._packed is None or self._packed.device != self.weight.device:
            if self.route == "thin":
                self._packed = pack_thin_conv_weights(self.weight)
            elif self.route == "grouped":
                g, k = self.groups, self.kernel
                self._packed = self.weight.view(g, 8, 32, k, k).permute(0, 3, 4, 2, 1).contiguous()  # [g][ky][kx][c][j]
            else:
                self._packed = pack_conv_weights(self)  # reads `.weight` (OIHW)
        return self._packed

    def forward(self, x: torch.Tensor, *, pads: tuple[int, int] = (0, 0), relu: bool = False, residual: torch.Tensor | None = None,  # noqa: C901, PLR0911, PLR0912
                out: torch.Tensor | None = None, pre: "_BnAct | None" = None, post: "_BnAct | None" = None, want_raw: bool = True):
        """``v = act(conv(x) + bias + residual)``.  ``pre``: the convolution of ``relu(bn(x))`` instead, the BN + ReLU applied on load
        where the kernel can (a head, ``activates_on_load``), as a pass of its own otherwise.  ``post``: returns ``(v, relu(bn(v)))``
        -- ``(None, relu(bn(v)))`` with ``want_raw=False`` -- both from one epilogue on the MFMA kernels (half: the activated copy
        comes from the unrounded sum).  ``out``: where a grouped layer writes (a channel slice / window of a wider buffer)."""
        half = self.half_dtype
        bias = self.bias if half is None else self._bias32
        plain = pads == (0, 0) and not relu and residual is None
        if post is not None and self.route != "mfma":  # no second epilogue output off the MFMA kernels: a pass of its own (float32)
            v = self(x, pads=pads, relu=relu, residual=residual, pre=pre)
            return (v if want_raw else None), post(v)
        if self.route == "head" and plain:
            sc, sh = pre.affine32() if pre is not None else (None, None)
            return hip_conv1x1_head(_cl(x), self.weight if half is None else self._weight32, bias, pre_scale=sc, pre_shift=sh)
        if pre is not None:
            if self.activates_on_load and pads == (0, 0) and post is None:
                return hip_conv1x1_pre(_cl(x), *pre.affine32(), self._operand(), bias, residual, stride=self.stride, relu=relu)
            if half is not None:
                msg = f"half-precision _Conv {tuple(self.weight.shape)}: the {self.route} kernel takes no activation on load."
                raise TypeError(msg)
            x = pre(x)
        if self.route == "thin" and residual is None:
            return hip_conv2d_thin(x, self._operand(), bias, kernel=self.kernel, stride=self.stride, pad_lo=pads[0], pad_hi=pads[1],
                                   relu=relu, **({} if half is None else {"out_dtype": half}))
        if self.route == "grouped" and plain:
            conv = hip_grouped_conv_valid if half is None else hip_grouped_conv_valid_h
            return conv(_cl(x), self._operand(), groups=self.groups, kernel=self.kernel, out=out)
        if half is not None and self.route != "mfma":
            msg = (f"half-precision _Conv {tuple(self.weight.shape)}: no {half} form of the {self.route} kernel for pads {pads}, "
                   f"relu {relu}, residual {'given' if residual is not None else 'none'}.")
            raise TypeError(msg)
        if self.route == "mfma":
            sc, sh = post.affine32() if post is not None else (None, None)
            if half is not None:
                geometry = {"cout": self.weight.shape[0], "kernel": self.kernel, "stride": self.stride}
                if post is not None or pads[0] != pads[1]:
                    # a second output, or TensorFlow "same" padding of a strided layer: the extended entry point (only the plain
                    # one may take the tap-reuse route, so the two stay apart)
                    return hip_conv2d_h_ex(_cl(x), self._packed_h, bias, residual, **geometry, pad_lo=pads[0], pad_hi=pads[1],
                                           relu=relu, post_scale=sc, post_shift=sh, want_raw=want_raw)
                return hip_conv2d_h(_cl(x), self._packed_h, bias, residual, **geometry, padding=pads[0], relu=relu)
            if post is not None:
                return hip_conv2d_post(_cl(x), self._operand(), bias, residual, kernel=self.kernel, stride=self.stride, pad_lo=pads[0],
                                       pad_hi=pads[1], relu=relu, post_scale=sc, post_shift=sh, want_raw=want_raw)
            if self.wino_ok and self.conv_algo == "winograd" and max(pads) <= 2:  # noqa: PLR2004
                if self._wino is None or self._wino.device != self.weight.device:
                    self._wino = pack_conv_weights_wino(self)  # reads `.weight` (OIHW, BN folded)
                return hip_conv3x3_wino(_cl(x), self._wino, bias, residual, padding=pads[0], pad_hi=pads[1], relu=relu)
            return hip_conv2d_ex(_cl(x), self._operand(), bias, residual, kernel=self.kernel, stride=self.stride,
                                 pad_lo=pads[0], pad_hi=pads[1], relu=relu)
        if pads != (0, 0):
            x = F.pad(x, (pads[0], pads[1], pads[0], pads[1]))
        y = _cl(F.conv2d(x, self.weight, None, self.stride, 0, 1, self.groups))
        if bias is not None or relu or residual is not None:
            bias = bias if bias is not None else torch.zeros(y.shape[1], device=y.device)
            if y.shape[1] % 4 == 0:
                return hip_bias_act_(y, bias, residual, relu=relu)
            y = y + bias[None, :, None, None]
            y = y + residual if residual is not None else y
            return F.relu(y) if relu else y
        return y


def set_conv_algo(model: nn.Module, algo: str) -> int:
    """``"direct"`` | ``"winograd"`` for every plain 3x3 / stride-1 MFMA convolution of a fused segmentation network (``FusedHoVerNet``,
    ``FusedUNet``); returns how many layers the switch applies to.  Layers with a second epilogue output or an activation on load
    keep their own kernels."""
    if algo not in ("direct", "winograd"):
        msg = f"conv_algo must be 'direct' or 'winograd', got {algo!r}."
        raise ValueError(msg)
    count = 0
    for mod in model.modules():
        if isinstance(mod, _Conv):
            mod.conv_algo = algo
            count += int(mod.wino_ok)
    return count


class _BnAct(nn.Module):
    def __init__(self, bn: nn.BatchNorm2d) -> None:
        super().__init__()
        scale, shift = _bn_affine(bn)
        self.register_buffer("scale", scale)
        self.register_buffer("shift", shift)
        self._affine32: tuple[torch.Tensor, torch.Tensor] | None = None

    def prepare(self, dtype: torch.dtype) -> None:
        """Keep float32 copies of scale / shift in a plain attribute before the module is cast to ``dtype`` (the half kernels
        take them in float32; the buffers would be rounded)."""
        self._affine32 = None if dtype == torch.float32 else (self.scale.detach().float().clone(), self.shift.detach().float().clone())

    def affine32(self) -> tuple[torch.Tensor, torch.Tensor]:
        return self._affine32 if self._affine32 is not None else (self.scale, self.shift)

    def forward(self, x: torch.Tensor, *, inplace: bool = False) -> torch.Tensor:
        return hip_scale_shift_act(_cl(x), self.scale, self.shift, relu=True, inplace=inplace)

    def view(self, x: torch.Tensor) -> torch.Tensor:
        """The same for a channel-prefix / window view of a wider channels-last buffer; dense result (half: the float32 affine)."""
        scale, shift = self.affine32()
        return hip_scale_shift_act_view(x, scale, shift, relu=True)


class _FusedResidualBlock(nn.Module):
    def __init__(self, blk: nn.Module) -> None:
        super().__init__()
        self.pre = nn.ModuleList()
        self.c1, self.c2, self.c3 = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for unit in blk.units:
            mods = dict(unit.named_children())
            self.pre.append(_BnAct(mods["preact/bn"]) if "preact/bn" in mods else nn.Identity())
            self.c1.append(_Conv(mods["conv1"], mods["conv1/bn"]))
            self.c2.append(_Conv(mods["conv2"], mods["conv2/bn"]))
            self.c3.append(_Conv(mods["conv3"]))
        self.shortcut = _Conv(blk.shortcut) if blk.shortcut is not None else None
        self.out = _BnAct(blk.blk_bna.bn)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        shortcut = x if self.shortcut is None else self.shortcut(x)
        units = len(self.c1)
        a = x  # the first unit has no pre-activation
        raw_in = False  # `a` is the raw residual sum: the unit's pre-activation is applied by conv1 on load
        for i, (c1, c2, c3) in enumerate(zip(self.c1, self.c2, self.c3)):
            a = c1(a, relu=True, pre=self.pre[i] if raw_in else None)
            a = c2(a, pads=_same_pads(a.shape[2], c2.kernel, c2.stride), relu=True)
            last = i + 1 == units
            raw_in = not last and c3.mfma_ok and self.c1[i + 1].activates_on_load  # (never in half: no activation on load there)
            if raw_in:
                # conv3 + shortcut only: the next unit reads this raw sum twice (conv1 activates it on load, conv3 adds it),
                # so the activated copy is neither written nor read back -- 3 instead of 4 passes over the widest tensor
                a = shortcut = c3(a, residual=_cl(shortcut))
            else:
                # conv3 + shortcut, and the BN + ReLU that follows the sum (the block's blk_bna; in half the next unit's
                # pre-activation, taken from the unrounded sum), from one epilogue; the last unit writes the activated copy only
                shortcut, a = c3(a, residual=_cl(shortcut), post=self.out if last else self.pre[i + 1], want_raw=not last)
        return a


class _FusedDenseBlock(nn.Module):
    def __init__(self, blk: nn.Module) -> None:
        super().__init__()
        self.pre, self.c1, self.c2 = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for unit in blk.units:
            mods = dict(unit.named_children())
            self.pre.append(_BnAct(mods["preact_bna/bn"]))
            self.c1.append(_Conv(mods["conv1"], mods["conv1/bn"]))
            self.c2.append(_Conv(mods["conv2"]))
        self.out = _BnAct(blk.blk_bna.bn)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # x_{i+1} = cat(centre_crop(x_i), new_i): instead of re-concatenating the growing stack, one buffer holds all
        # channels at the input size; unit i reads the channel prefix / shrinking window it owns and writes its 32 new
        # channels into the next slice (valid k x k convolutions crop (k - 1) / 2 pixels per side and unit)
        n, c0, h0, w0 = x.shape
        units = len(self.c1)
        grow = self.c2[0].weight.shape[0]
        r = (self.c2[0].kernel - 1) // 2
        buf = torch.empty((n, c0 + grow * units, h0, w0), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        buf[:, :c0] = x
        c = c0
        for i, (pre, c1, c2) in enumerate(zip(self.pre, self.c1, self.c2)):
            view = buf[:, :c, i * r:h0 - i * r, i * r:w0 - i * r]
            dst = buf[:, c:c + grow, (i + 1) * r:h0 - (i + 1) * r, (i + 1) * r:w0 - (i + 1) * r]
            new = c2(c1(pre.view(view), relu=True), out=dst)  # the grouped kernel writes straight into its slice
            if new is not dst:  # any other layer (float32 only: `prepare` refuses it)
                dst.copy_(new)
            c += grow
        return self.out.view(buf[:, :, units * r:h0 - units * r, units * r:w0 - units * r])


class _FusedBranch(nn.Module):
    def __init__(self, branch: nn.Sequential) -> None:
        super().__init__()
        u3, u2, u1, u0 = branch[0], branch[1], branch[2], branch[3]
        self.u3a, self.u3d, self.u3f = _Conv(u3.conva), _FusedDenseBlock(u3.dense), _Conv(u3.convf)
        self.u2a, self.u2d, self.u2f = _Conv(u2.conva), _FusedDenseBlock(u2.dense), _Conv(u2.convf)
        self.u1a = _Conv(u1.conva)
        self.u1_ksize = u1.conva.kernel_size[0]
        self.u0bn = _BnAct(u0.bn)
        self.u0 = _Conv(u0.conv)


class FusedHoVerNet(nn.Module):
    """``forward(x)`` == ``HoVerNet.forward(x)`` (``{branch: logits}``, float32) on a CUDA device, in float32 or -- after
    ``prepare(dtype)`` -- with fp16 / bf16 activations."""

    def __init__(self, model: nn.Module) -> None:
        super().__init__()
        model = model.eval()
        self.mode = model.mode
        stem = dict(model.conv0.named_children())
        self.stem = _Conv(stem["/"], stem["bn"])
        self.stem_pad = "pad" in stem
        self.d0, self.d1 = _FusedResidualBlock(model.d0), _FusedResidualBlock(model.d1)
        self.d2, self.d3 = _FusedResidualBlock(model.d2), _FusedResidualBlock(model.d3)
        self.conv_bot = _Conv(model.conv_bot)
        self.decoder = nn.ModuleDict(OrderedDict((name, _FusedBranch(branch)) for name, branch in model.decoder.items()))
        self.half_dtype: torch.dtype | None = None  # fp16 / bf16 once `prepare(dtype)` has switched every layer

    def prepare(self, dtype: torch.dtype) -> None:
        """fp16 / bf16 activations on the same graph (the engines' ``compute_dtype``): call this on the device, on the float32
        copy, BEFORE ``.to(dtype)``.  Every MFMA convolution packs its BN-folded float32 weights for ``tia_conv2d_nhwc_h(_ex)``
        (rounded once, after the folding) and keeps its bias in float32; every BN scale / shift and the heads' weights stay
        float32 in plain attributes that the cast does not reach; the dense units' grouped convolutions are packed for
        ``tia_grouped_conv_valid_nhwc_h``.  Each layer does this for itself (``_Conv.prepare``, ``_BnAct.prepare``).  The stem stays the float32-arithmetic thin kernel writing its map in ``dtype`` (under
        1 % of the forward; exactly one rounding of the float32 stem); residual units take their pre-activations from the second
        epilogue output of conv3 (no activation on load in half); the logits come back in float32.  A layer without a half kernel
        raises ``TypeError``: there is no library fall-back, and ``conv_algo`` has no effect in half.  ``torch.float32``
        switches back (on a module that has not been cast)."""
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            msg = f"FusedHoVerNet runs in float32, float16 or bfloat16; got {dtype}."
            raise ValueError(msg)
        if self.stem.weight.dtype != torch.float32:
            msg = f"FusedHoVerNet.prepare starts from the float32 parameters (call it before the cast); got {self.stem.weight.dtype}."
            raise ValueError(msg)
        for mod in self.modules():
            if isinstance(mod, (_Conv, _BnAct)):
                mod.prepare(dtype)
        self.half_dtype = None if dtype == torch.float32 else dtype

    def forward(self, input_tensor: torch.Tensor) -> dict:
        half = self.half_dtype
        # (half: the batch arrives in `half`, where 0 .. 255 are exact; the division is the float32 copy's)
        x = _cl(input_tensor / 255.0) if half is None else _cl(input_tensor.float() / 255.0)
        pads = _same_pads(x.shape[2], self.stem.kernel, 1) if self.stem_pad else (0, 0)
        stem = self.stem(x, pads=pads, relu=True)  # (half: the float32 stem rounded once)
        d0 = self.d0(stem)
        d1 = self.d1(d0)
        d2 = self.d2(d1)
        d3 = self.conv_bot(self.d3(d2))
        if self.mode == "original":
            d0, d1 = centre_crop(d0, [184, 184]), centre_crop(d1, [72, 72])
        else:
            d0, d1 = centre_crop(d0, [92, 92]), centre_crop(d1, [36, 36])
        up3 = hip_upsample2x_add(_cl(d3), d2)  # shared by the branches
        out = OrderedDict()
        for name, br in self.decoder.items():
            u3 = br.u3f(br.u3d(br.u3a(up3)))
            u2 = br.u2f(br.u2d(br.u2a(hip_upsample2x_add(_cl(u3), d1))))
            u1_in = hip_upsample2x_add(_cl(u2), d0)
            u1 = br.u1a(u1_in, pads=_same_pads(u1_in.shape[2], br.u1_ksize, 1))
            out[name] = br.u0(u1, pre=br.u0bn)  # BN + ReLU + 1x1 head: one launch
        return out

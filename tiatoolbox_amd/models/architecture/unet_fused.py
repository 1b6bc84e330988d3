"""Inference copies of :class:`UNetModel` on the hand-written MFMA convolutions (float32; fp16 / bf16 after ``prepare(dtype)``):
``FusedUNet`` for the ResNet-50 encoder, ``FusedPlainUNet`` (at the end of this file) for the plain one, each with additive or
concatenated skip connections.

``FusedUNet``:

Same arithmetic graph as ``UNetModel.forward`` (reference ``models/architecture/unet.py:356-417``):

* encoder = torchvision-layout ResNet-50: every Bottleneck as three launches -- ``conv1 + BN + ReLU``, ``conv2 + BN +
  ReLU`` and ``conv3 + BN + identity + ReLU`` -- with the BNs folded into the weights and the residual add / ReLU in the
  convolution epilogues (the down-sampling 1x1 likewise, without ReLU);
* decoder (pre-activation blocks ``BN -> ReLU -> conv -> BN -> ReLU -> conv`` after ``upsample2x(x) + skip`` or
  ``cat(upsample2x(x), skip)``): the up-sampling, the skip add / concatenation and the first BN + ReLU in one pass, the second BN
  folded into the first convolution;
* the stem -- ``x / 255`` (on load, from the uint8 patch), 7x7 / 2 convolution + BN + ReLU AND the 3x3 / 2 max-pool -- is ONE
  launch of the hand-written stem kernel, which also writes the pre-pool activation (the decoder's first skip connection);
* the final ``64 -> n_classes`` 1x1 is the class-head kernel.

Built from a loaded model (reference parameter names); CUDA, channels-last only.  float32 by default; ``prepare(dtype)`` switches the
same graph to fp16 / bf16 activations: ``tia_conv2d_nhwc_h`` for the 61 convolutions, the half forms of the up-sampling pass and
of the head, the float32-arithmetic stem writing halves; float32 logits either way.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F  # noqa: N812
from torch import nn

from tiatoolbox_amd.models.architecture.fused import (hip_avgpool2x2, hip_stem_conv_pool, hip_upsample2x_add, hip_upsample2x_concat,
                                                      pack_stem_weights)
from tiatoolbox_amd.models.architecture.hovernet_fused import _BnAct, _cl, _Conv
from tiatoolbox_amd.models.architecture.resnet import Bottleneck


class UnsupportedLayerError(TypeError):
    """A fused UNet cannot be built from this model: its encoder or block layout is not the one the class covers, or a layer has
    no hand-written kernel.  A ``TypeError`` of its own, so that a caller who falls back to the torch module (the engines) does
    so for this reason only and never swallows a programming error."""


def library_convolutions(fused: nn.Module) -> list[str]:
    """Names of the ``_Conv`` layers of a fused graph that no hand-written kernel takes (``route == "torch"``): in float32 each of
    them calls the library convolution, in half ``prepare`` refuses them.  ``FusedPlainUNet`` never has one (its constructor
    refuses); ``FusedUNet`` builds around such a layer, and the engines say so with this list."""
    return [name for name, mod in fused.named_modules() if isinstance(mod, _Conv) and mod.route == "torch"]


class _FusedBottleneckMfma(nn.Module):
    def __init__(self, blk: Bottleneck) -> None:
        super().__init__()
        self.c1, self.c2, self.c3 = _Conv(blk.conv1, blk.bn1), _Conv(blk.conv2, blk.bn2), _Conv(blk.conv3, blk.bn3)
        self.pad = blk.conv2.padding[0]
        self.down = _Conv(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = x if self.down is None else self.down(x)
        out = self.c1(x, relu=True)
        out = self.c2(out, pads=(self.pad, self.pad), relu=True)
        return self.c3(out, relu=True, residual=_cl(identity))


class FusedUNet(nn.Module):
    """``forward(x)`` == ``UNetModel.forward(x)`` (class logits, float32) on a CUDA device, in float32 or -- after ``prepare(dtype)`` --
    fp16 / bf16 activations; ResNet-50 encoder, pre-activation
    decoder, ``skip_type="add"`` (the layout of ``fcn-tissue_mask`` / ``fcn_resnet50_unet-bcss``) or ``"concat"``."""

    def __init__(self, model: nn.Module) -> None:
        super().__init__()
        model = model.eval()
        bb = model.backbone
        if not hasattr(bb, "layer1"):
            msg = "FusedUNet covers the ResNet-50 encoder (FusedPlainUNet runs the plain one)."
            raise UnsupportedLayerError(msg)
        self.concat = model.skip_type == "concat"  # the decoder's first BN then covers both halves of the concatenation
        self.stem = _Conv(bb.conv1, bb.bn1)  # BN folded; executed by the stem kernel (7x7 / stride 2 / pad 3 + 3x3 / 2 max-pool)
        mp = bb.maxpool
        if (bb.conv1.stride != (2, 2) or bb.conv1.padding != (3, 3) or (mp.kernel_size, mp.stride, mp.padding) != (3, 2, 1)
                or bb.conv1.weight.shape != (64, 3, 7, 7)):
            msg = "FusedUNet expects the torchvision ResNet stem (conv 7x7 / 2 / pad 3, 3 -> 64; max-pool 3 / 2 / 1)."
            raise UnsupportedLayerError(msg)
        self._stem_packed: torch.Tensor | None = None
        self._stem_bias32: torch.Tensor | None = None
        self.half_dtype: torch.dtype | None = None  # fp16 / bf16 once `prepare(dtype)` has packed the half form
        self.layers = nn.ModuleList(nn.Sequential(*[_FusedBottleneckMfma(b) for b in layer])
                                    for layer in (bb.layer1, bb.layer2, bb.layer3, bb.layer4))
        self.conv1x1 = _Conv(model.conv1x1)
        self.up = nn.ModuleList()
        for block in model.uplist:
            mods = list(block)
            # [BN_a, ReLU, conv_a, BN_b, ReLU, conv_b, ...]: BN_a stays a pass of its own, every later BN folds backwards
            if not (isinstance(mods[0], nn.BatchNorm2d) and len(mods) % 3 == 0):
                msg = "FusedUNet expects pre-activation decoder blocks."
                raise UnsupportedLayerError(msg)
            convs = [mods[i] for i in range(2, len(mods), 3)]
            bns = [mods[i] for i in range(3, len(mods), 3)]
            stage = nn.ModuleList([_BnAct(mods[0])])
            for i, conv in enumerate(convs):
                stage.append(_Conv(conv, bns[i] if i < len(bns) else None))
            self.up.append(stage)
        self.clf = _Conv(model.clf)

    accepts_uint8 = True  # `infer_batch` hands the uint8 batch over as it is: the stem kernel divides by 255 while it loads

    def prepare(self, dtype: torch.dtype) -> None:
        """fp16 / bf16 activations on the same graph (the engines' ``compute_dtype``): call this on the device, on the float32
        copy, BEFORE ``.to(dtype)``.  Every convolution packs its BN-folded float32 weights for ``tia_conv2d_nhwc_h`` (rounded
        once, after the folding) and keeps its bias in float32; the decoder's BN scale / shift, the head's weights and the stem's
        packed weights and bias stay float32 in plain attributes that the cast does not reach.  The stem stays the float32-
        arithmetic kernel writing both of its maps in ``dtype`` (< 2 % of the flops, and exactly one rounding of the float32
        stem), the up-sampling passes and the head run on their half forms, the logits come back in float32.  A layer without
        a half kernel raises ``TypeError``.  ``torch.float32`` switches back (on a module that has not been cast)."""
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            msg = f"FusedUNet runs in float32, float16 or bfloat16; got {dtype}."
            raise ValueError(msg)
        if self.stem.weight.dtype != torch.float32:
            msg = f"FusedUNet.prepare starts from the float32 parameters (call it before the cast); got {self.stem.weight.dtype}."
            raise ValueError(msg)
        for mod in self.modules():
            if isinstance(mod, (_Conv, _BnAct)) and mod is not self.stem:
                mod.prepare(dtype)
        self._stem_packed = pack_stem_weights(self.stem.weight)
        self._stem_bias32 = self.stem.bias.detach().clone().contiguous()
        self.half_dtype = None if dtype == torch.float32 else dtype

    def forward(self, imgs: torch.Tensor, *args, **kwargs) -> torch.Tensor:  # noqa: ARG002
        half = self.half_dtype
        if half is None and (self._stem_packed is None or self._stem_packed.device != self.stem.weight.device):
            self._stem_packed = pack_stem_weights(self.stem.weight)
        x = imgs.permute(0, 2, 3, 1)  # the NHWC batch under the NCHW view
        if x.dtype == torch.uint8:
            x = x.contiguous()
        elif half is None:
            x = (x.to(torch.float32) / 255.0).contiguous()
        else:
            # the quotient through float64: correctly rounded for the integers 0 .. 255 (the device's `x / 255.0` multiplies by the
            # rounded reciprocal), so a float batch and the same bytes give the same logits
            x = (x.to(torch.float64) / 255.0).to(torch.float32).contiguous()
        # (half: float32 arithmetic, both maps rounded once to `half`; the parameter `stem.bias` has been cast, its float32 copy has not)
        x, conv = hip_stem_conv_pool(x, self._stem_packed, self.stem.bias if half is None else self._stem_bias32,
                                     out_dtype=half or torch.float32, return_conv=True)
        feats = [conv]
        for layer in self.layers:
            x = layer(x)
            feats.append(x)
        x = self.conv1x1(feats[-1])
        skips = feats[:-1]
        for idx, stage in enumerate(self.up, start=1):
            up = hip_upsample2x_concat if self.concat else hip_upsample2x_add
            x = up(_cl(x), _cl(skips[-idx]), *stage[0].affine32())  # + the block's pre-activation
            for j, conv in enumerate(list(stage)[1:]):
                last = j == len(stage) - 2
                p = (conv.kernel - 1) // 2
                x = conv(x, pads=(p, p), relu=not last)
        return self.clf(x)


class FusedPlainUNet(nn.Module):
    """``forward(x)`` == ``UNetModel.forward(x)`` (class logits, float32) for ``encoder="unet"`` on a CUDA device, in float32 or --
    after ``prepare(dtype)`` -- fp16 / bf16 activations; ``skip_type`` ``"add"`` or ``"concat"``.  Built from ``_Conv`` only:

    * encoder block ``conv, BN, ReLU, conv, BN, ReLU``: two convolutions with the BN folded and the ReLU in the epilogue; the first
      convolution of the network (3 channels) on the thin-input form of the MFMA kernel; ``AvgPool2d(2, 2)`` on
      ``hip_avgpool2x2`` (the pooling behind the last block feeds nothing and is not run);
    * decoder: ``hip_upsample2x_add`` or ``hip_upsample2x_concat`` (no affine: the blocks are post-activation), then every
      ``conv, BN, ReLU`` as one convolution; ``conv1x1`` and the class head ``clf`` likewise.

    A layer that ``_Conv`` would hand to the library convolution (``route == "torch"``) is refused here with a ``TypeError`` that
    names it (``UnsupportedLayerError``): this graph has no library fall-back, in float32 either."""

    accepts_uint8 = False  # the thin first layer reads float32: `infer_batch` hands the batch over in the parameters' dtype

    def __init__(self, model: nn.Module) -> None:
        super().__init__()
        model = model.eval()
        bb = model.backbone
        if not hasattr(bb, "blocks"):
            msg = "FusedPlainUNet covers the plain conv-BN-ReLU x2 + average-pool encoder (FusedUNet runs the ResNet-50 one)."
            raise UnsupportedLayerError(msg)
        self.concat = model.skip_type == "concat"
        self.half_dtype: torch.dtype | None = None  # fp16 / bf16 once `prepare(dtype)` has packed the half form
        names = {id(mod): name for name, mod in model.named_modules()}

        def conv_bn_relu(mods: list[nn.Module], what: str) -> nn.ModuleList:
            ok = len(mods) % 3 == 0 and all(isinstance(mods[i], nn.Conv2d) and isinstance(mods[i + 1], nn.BatchNorm2d)
                                            and isinstance(mods[i + 2], nn.ReLU) for i in range(0, len(mods) - 2, 3))
            if not ok or not mods:
                msg = f"FusedPlainUNet expects {what} made of (conv, BN, ReLU) triples; got {[type(m).__name__ for m in mods]}."
                raise UnsupportedLayerError(msg)
            return nn.ModuleList(self._conv(mods[i], mods[i + 1], names) for i in range(0, len(mods), 3))

        self.enc = nn.ModuleList()
        for block in bb.blocks:
            pool = block[1]
            # (floor division of odd maps and the plain mean of four are all the kernel does: no ceil_mode, no divisor_override)
            if (not isinstance(pool, nn.AvgPool2d) or (pool.kernel_size, pool.stride, pool.padding) not in ((2, 2, 0), ((2, 2), (2, 2), (0, 0)))
                    or pool.ceil_mode or pool.divisor_override is not None):
                msg = f"FusedPlainUNet expects AvgPool2d(2, stride=2) without ceil_mode or divisor_override behind every encoder block; got {pool}."
                raise UnsupportedLayerError(msg)
            self.enc.append(conv_bn_relu(list(block[0]), "encoder blocks"))
        self.conv1x1 = self._conv(model.conv1x1, None, names)
        self.up = nn.ModuleList(conv_bn_relu(list(block), "post-activation decoder blocks") for block in model.uplist)
        self.clf = self._conv(model.clf, None, names)

    @staticmethod
    def _conv(conv: nn.Conv2d, bn: nn.BatchNorm2d | None, names: dict) -> _Conv:
        layer = _Conv(conv, bn)
        same = conv.padding == ((conv.kernel_size[0] - 1) // 2,) * 2 and conv.dilation == (1, 1)  # what `forward` passes as `pads`
        if layer.route == "torch" or not same:
            msg = (f"FusedPlainUNet: no hand-written kernel for layer `{names.get(id(conv), '?')}` ({conv}): the MFMA kernels take "
                   "cin % 32 == 0 and cout % 64 == 0, the thin-input form cin * k <= 32 and cout % 64 == 0, the class head 64 -> at "
                   "most 8 channels, all with 'same' padding and no dilation.")
            raise UnsupportedLayerError(msg)
        return layer

    def prepare(self, dtype: torch.dtype) -> None:
        """fp16 / bf16 activations on the same graph (the engines' ``compute_dtype``): call this on the device, on the float32
        copy, BEFORE ``.to(dtype)``.  Every convolution packs its BN-folded float32 weights (rounded once, after the folding) and
        keeps its bias in float32 in a plain attribute that the cast does not reach (``_Conv.prepare``); the thin first layer stays
        float32 arithmetic on float32 weights and writes ``dtype``; pooling and up-sampling run on their half forms; the logits
        come back in float32.  A layer without a half kernel (a thin first layer with a stride) raises ``TypeError``.
        ``torch.float32`` switches back (on a module that has not been cast)."""
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            msg = f"FusedPlainUNet runs in float32, float16 or bfloat16; got {dtype}."
            raise ValueError(msg)
        if self.clf.weight.dtype != torch.float32:
            msg = f"FusedPlainUNet.prepare starts from the float32 parameters (call it before the cast); got {self.clf.weight.dtype}."
            raise ValueError(msg)
        for mod in self.modules():
            if isinstance(mod, _Conv):
                mod.prepare(dtype)
        self.half_dtype = None if dtype == torch.float32 else dtype

    def forward(self, imgs: torch.Tensor, *args, **kwargs) -> torch.Tensor:  # noqa: ARG002
        half = self.half_dtype
        # the quotient through float64: correctly rounded for the integers 0 .. 255 (the device's `x / 255.0` multiplies by the
        # rounded reciprocal), so a float batch and the same bytes give the same logits
        x = (imgs.to(torch.float64) / 255.0).to(torch.float32)
        if half is not None and self.enc[0][0].route != "thin":  # (the thin kernel reads float32 and writes `half` itself)
            x = x.to(half)
        feats = []
        for level, block in enumerate(self.enc):
            if level:
                x = hip_avgpool2x2(_cl(x))
            for conv in block:
                p = (conv.kernel - 1) // 2
                x = conv(x, pads=(p, p), relu=True)
            feats.append(x)
        x = self.conv1x1(feats[-1])
        skips = feats[:-1]
        up = hip_upsample2x_concat if self.concat else hip_upsample2x_add
        for idx, stage in enumerate(self.up, start=1):
            x = up(_cl(x), _cl(skips[-idx]))
            for conv in stage:
                p = (conv.kernel - 1) // 2
                x = conv(x, pads=(p, p), relu=True)
        return self.clf(x)

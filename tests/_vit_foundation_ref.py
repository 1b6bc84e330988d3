"""Host-only helpers of the foundation-model tests (``UNI2``, ``H-optimus``, ``prov-gigapath``): the tiny configurations, weights that
make every term visible (register tokens included), and an independent float64 restatement of the extended forward -- register
tokens, a position table without a class entry, timm's ``SwiGLUPacked`` -- written from the state dict with explicit slicing."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F  # noqa: N812

from _vit_ref import randomise

# patch 14, three register tokens, a grid-only position table, packed SwiGLU (the UNI2 / H-optimus form); 128 / 2 = 64 per head
TINY_REG = {"embed_dim": 128, "depth": 2, "num_heads": 2, "mlp_dim": 512, "patch_size": 14, "img_size": 28, "init_values": 1e-5,
            "reg_tokens": 3, "no_embed_class": True, "mlp_layer": "swiglu_packed", "dynamic_img_size": True}
# patch 16, no register tokens, a class entry in the table, packed SwiGLU (the prov-gigapath form)
TINY_GIGA = {"embed_dim": 128, "depth": 2, "num_heads": 2, "mlp_dim": 512, "patch_size": 16, "img_size": 32, "init_values": 1e-5,
             "mlp_layer": "swiglu_packed", "dynamic_img_size": True}


def tiny_foundation(cfg: dict, *, seed: int = 0, **over):
    from tiatoolbox_amd.models.architecture.vit import VisionTransformer

    torch.manual_seed(seed)
    vit = randomise(VisionTransformer(**{**cfg, **over}), seed)
    if "reg_token" in dict(vit.named_parameters()):  # (timm's std 1e-6 would hide it, and `_vit_ref.randomise` does not know it)
        with torch.no_grad():
            vit.reg_token.copy_(torch.randn(vit.reg_token.shape, generator=torch.Generator().manual_seed(2000 + seed)) * 0.5)
    return vit.eval()


def forward64(sd: dict, imgs: torch.Tensor, *, heads: int, patch: int, native_grid: tuple[int, int], no_embed_class: bool) -> torch.Tensor:
    """The extended forward from the state dict alone, in float64.  Register tokens are there when ``reg_token`` is a key; the MLP is
    the packed SwiGLU when ``fc2`` takes half of ``fc1``'s width (gate = the FIRST half of ``fc1``'s rows), else the exact GELU."""
    sd = {k: v.double() for k, v in sd.items()}
    x = imgs.double()
    b, _, h, w = x.shape
    gh, gw = h // patch, w // patch
    cols = F.unfold(x, kernel_size=patch, stride=patch)  # [B, 3 p p, g] in (c, ky, kx) order: the OIHW flattening
    tok = cols.transpose(1, 2) @ sd["patch_embed.proj.weight"].flatten(1).T + sd["patch_embed.proj.bias"]
    pos = sd["pos_embed"]
    npre = 0 if no_embed_class else 1
    d = pos.shape[-1]
    assert pos.shape[1] == npre + native_grid[0] * native_grid[1]
    if (gh, gw) != tuple(native_grid):
        tab = pos[:, npre:].float().reshape(1, native_grid[0], native_grid[1], d).permute(0, 3, 1, 2)
        tab = F.interpolate(tab, size=(gh, gw), mode="bicubic", antialias=True, align_corners=False)
        pos = torch.cat([pos[:, :npre], tab.permute(0, 2, 3, 1).reshape(1, gh * gw, d).double()], dim=1)
    cls = sd["cls_token"].expand(b, -1, -1)
    if no_embed_class:
        rows = [cls] + ([sd["reg_token"].expand(b, -1, -1)] if "reg_token" in sd else [])
        x = torch.cat([*rows, tok + pos], dim=1)
    else:
        assert "reg_token" not in sd
        x = torch.cat([cls, tok], dim=1) + pos
    hd = d // heads

    def ln(t, wgt, bias):
        mu = t.mean(-1, keepdim=True)
        var = ((t - mu) ** 2).mean(-1, keepdim=True)
        return (t - mu) / torch.sqrt(var + 1e-6) * wgt + bias

    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    for i in range(depth):
        pre = f"blocks.{i}."
        a = ln(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"])
        wq, bq = sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]
        outs = []
        for hh in range(heads):
            q = a @ wq[hh * hd:(hh + 1) * hd].T + bq[hh * hd:(hh + 1) * hd]
            k = a @ wq[d + hh * hd:d + (hh + 1) * hd].T + bq[d + hh * hd:d + (hh + 1) * hd]
            v = a @ wq[2 * d + hh * hd:2 * d + (hh + 1) * hd].T + bq[2 * d + hh * hd:2 * d + (hh + 1) * hd]
            sc = q @ k.transpose(1, 2) / math.sqrt(hd)
            outs.append(torch.softmax(sc, -1) @ v)
        a = torch.cat(outs, -1) @ sd[pre + "attn.proj.weight"].T + sd[pre + "attn.proj.bias"]
        if pre + "ls1.gamma" in sd:
            a = a * sd[pre + "ls1.gamma"]
        x = x + a
        a = ln(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"])
        w1, b1, w2 = sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"], sd[pre + "mlp.fc2.weight"]
        if 2 * w2.shape[1] == w1.shape[0]:
            hid = w2.shape[1]
            gate = a @ w1[:hid].T + b1[:hid]
            val = a @ w1[hid:].T + b1[hid:]
            a = gate / (1.0 + torch.exp(-gate)) * val
        else:
            a = a @ w1.T + b1
            a = 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))
        a = a @ w2.T + sd[pre + "mlp.fc2.bias"]
        if pre + "ls2.gamma" in sd:
            a = a * sd[pre + "ls2.gamma"]
        x = x + a
    return ln(x[:, 0], sd["norm.weight"], sd["norm.bias"])

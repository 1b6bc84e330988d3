"""Host-only helpers of the ``Virchow`` / ``Virchow2`` tests: the tiny configurations (80 dimensions per head, a packed SwiGLU whose
half is off the GEMM's multiple of 32, the class + mean-patch output, register tokens with entries of their own in the position
table), weights that make every term visible, and an independent float64 restatement of the forward -- pooled output included --
written from the state dict with explicit slicing."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F  # noqa: N812

from _vit_ref import randomise

# 320 / 4 = 80 per head; mlp_dim 1040: H = 520 -> 544 in the fused graph (the pad route); a class-entry table, no register tokens
TINY_V1 = {"embed_dim": 320, "depth": 2, "num_heads": 4, "mlp_dim": 1040, "patch_size": 14, "img_size": 28, "init_values": 1e-5,
           "mlp_layer": "swiglu_packed", "global_pool": "token_mean", "dynamic_img_size": True}
# the same with three register tokens that have position entries of their own (timm's default form: Virchow2)
TINY_V2 = {**TINY_V1, "reg_tokens": 3, "prefix_pos_embed": True}
NO_PAD = {"mlp_dim": 1024}  # H = 512: on the GEMM's multiple, nothing is padded


def tiny_virchow(cfg: dict, *, seed: int = 0, **over):
    from tiatoolbox_amd.models.architecture.vit import VisionTransformer

    torch.manual_seed(seed)
    vit = randomise(VisionTransformer(**{**cfg, **over}), seed)  # (`pos_embed`, its prefix rows included, is drawn at std 0.5 there)
    if "reg_token" in dict(vit.named_parameters()):  # (timm's std 1e-6 would hide it, and `_vit_ref.randomise` does not know it)
        with torch.no_grad():
            vit.reg_token.copy_(torch.randn(vit.reg_token.shape, generator=torch.Generator().manual_seed(3000 + seed)) * 0.5)
    return vit.eval()


def forward64(sd: dict, imgs: torch.Tensor, *, heads: int, patch: int, native_grid: tuple[int, int], pool_skip: int | None = None) -> torch.Tensor:
    """The forward from the state dict alone, in float64.  The position table has ``1 + R`` leading entries (``R`` register tokens when
    ``reg_token`` is a key) which resampling leaves alone; the sequence is ``cat([cls, reg, patches]) + pos``; the MLP is the packed
    SwiGLU (gate = the FIRST half of ``fc1``'s rows); the output is ``cat([y[:, 0], mean_{i >= pool_skip} y[:, i]])`` of the final norm
    ``y``, ``pool_skip = 1 + R`` unless given (a test passes 1 to show what including the register rows would do)."""
    sd = {k: v.double() for k, v in sd.items()}
    x = imgs.double()
    b, _, h, w = x.shape
    gh, gw = h // patch, w // patch
    cols = F.unfold(x, kernel_size=patch, stride=patch)  # [B, 3 p p, g] in (c, ky, kx) order: the OIHW flattening
    tok = cols.transpose(1, 2) @ sd["patch_embed.proj.weight"].flatten(1).T + sd["patch_embed.proj.bias"]
    pos = sd["pos_embed"]
    nreg = sd["reg_token"].shape[1] if "reg_token" in sd else 0
    npre = 1 + nreg
    d = pos.shape[-1]
    assert pos.shape[1] == npre + native_grid[0] * native_grid[1]
    if (gh, gw) != tuple(native_grid):
        tab = pos[:, npre:].float().reshape(1, native_grid[0], native_grid[1], d).permute(0, 3, 1, 2)
        tab = F.interpolate(tab, size=(gh, gw), mode="bicubic", antialias=True, align_corners=False)
        pos = torch.cat([pos[:, :npre], tab.permute(0, 2, 3, 1).reshape(1, gh * gw, d).double()], dim=1)
    rows = [sd["cls_token"][0] + pos[0, :1]]
    if nreg:
        rows.append(sd["reg_token"][0] + pos[0, 1:npre])
    x = torch.cat([torch.cat(rows, dim=0).expand(b, -1, -1), tok + pos[:, npre:]], dim=1)
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
        x = x + a * sd[pre + "ls1.gamma"]
        a = ln(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"])
        w1, b1, w2 = sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"], sd[pre + "mlp.fc2.weight"]
        hid = w2.shape[1]
        assert w1.shape[0] == 2 * hid
        gate = a @ w1[:hid].T + b1[:hid]
        val = a @ w1[hid:].T + b1[hid:]
        a = (gate / (1.0 + torch.exp(-gate)) * val) @ w2.T + sd[pre + "mlp.fc2.bias"]
        x = x + a * sd[pre + "ls2.gamma"]
    y = ln(x, sd["norm.weight"], sd["norm.bias"])
    skip = npre if pool_skip is None else pool_skip
    mean = sum(y[:, i] for i in range(skip, y.shape[1])) / (y.shape[1] - skip)
    return torch.cat([y[:, 0], mean], dim=-1)

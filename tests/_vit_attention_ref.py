"""Host-only helpers of the attention-map tests: float64 restatements of the two map definitions (``return_attention="class"`` and
``"rollout"``) -- from a qkv tensor, for the kernels, and from a state dict, for the graph, independent of
``VisionTransformer.forward_with_attention`` (explicit per-head slices and loops, in the style of ``_vit_ref.forward64``)."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F  # noqa: N812


def probs64(qkv: torch.Tensor, heads: int, scale: float, q_rows: int | None = None) -> torch.Tensor:
    """``[n, heads, q_rows, S]`` float64 from ``qkv`` ``[n, S, 3 * heads * hd]`` (the qkv Linear's own order ``[n, S, 3, heads, hd]``),
    exactly the values given (widened): ``softmax_j(scale * q[i] . k[j])``, the row maximum subtracted."""
    n, s, c3 = qkv.shape
    hd = c3 // (3 * heads)
    x = qkv.detach().cpu().double().reshape(n, s, 3, heads, hd)
    rows = s if q_rows is None else q_rows
    out = torch.empty(n, heads, rows, s, dtype=torch.float64)
    for h in range(heads):
        q, k = x[:, :rows, 0, h], x[:, :, 1, h]
        sc = torch.einsum("bid,bjd->bij", q, k) * scale
        e = torch.exp(sc - sc.amax(-1, keepdim=True))
        out[:, h] = e / e.sum(-1, keepdim=True)
    return out


def probs32(qkv: torch.Tensor, heads: int, scale: float, q_rows: int | None = None, *, head_mean: bool = False) -> torch.Tensor:
    """The same formula in float32 torch on the CPU from the same half values: the yardstick of the kernel's error."""
    n, s, c3 = qkv.shape
    hd = c3 // (3 * heads)
    x = qkv.detach().cpu().float().reshape(n, s, 3, heads, hd)
    rows = s if q_rows is None else q_rows
    q, k = x[:, :rows, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    p = torch.softmax((q @ k.transpose(-2, -1)) * scale, -1)
    if head_mean:
        acc = p[:, 0]
        for h in range(1, heads):
            acc = acc + p[:, h]
        return acc / heads
    return p


def rollout_step64(a: torch.Tensor, r_in: torch.Tensor | None) -> torch.Tensor:
    a = a.detach().cpu().double()
    r = torch.eye(a.shape[-1], dtype=torch.float64).expand_as(a) if r_in is None else r_in.detach().cpu().double()
    return 0.5 * (a @ r) + 0.5 * r


def row_error(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """``max_rows(max_j |p - p64| / max_j p64)``: every entry counts."""
    got = got.detach().cpu().double()
    return float(((got - ref64).abs().amax(-1) / ref64.amax(-1)).max())


def maps64(sd: dict, imgs: torch.Tensor, kind: str, *, heads: int, patch: int, native_grid: tuple[int, int], no_embed_class: bool = False,
           prefix_pos_embed: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """``(maps, prefix mass or rollout row)`` in float64 from the state dict alone.  The sequence is built as the three forms build it
    (a class-entry table; ``no_embed_class`` with register tokens; ``prefix_pos_embed``), the blocks run with per-head slices of the
    qkv weight, and the maps follow the definitions: "class" -- the last block's ``softmax(scale q[0] . k[j])`` per head, columns
    ``1 + R:`` on the grid (second value: the mass on the ``1 + R`` prefix columns, ``[B, H]``); "rollout" -- ``A_l`` the head mean,
    ``R_1 = A_1 / 2 + I / 2``, ``R_l = A_l R_{l-1} / 2 + R_{l-1} / 2``, row 0, columns ``1 + R:`` (second value: the whole row 0)."""
    sd = {k: v.detach().cpu().double() for k, v in sd.items()}
    x = imgs.detach().cpu().double()
    b, _, h, w = x.shape
    gh, gw = h // patch, w // patch
    cols = F.unfold(x, kernel_size=patch, stride=patch)
    tok = cols.transpose(1, 2) @ sd["patch_embed.proj.weight"].flatten(1).T + sd["patch_embed.proj.bias"]
    pos = sd["pos_embed"]
    nreg = sd["reg_token"].shape[1] if "reg_token" in sd else 0
    npre = 0 if no_embed_class else 1 + (nreg if prefix_pos_embed else 0)
    d = pos.shape[-1]
    if (gh, gw) != tuple(native_grid):
        tab = pos[:, npre:].float().reshape(1, native_grid[0], native_grid[1], d).permute(0, 3, 1, 2)
        tab = F.interpolate(tab, size=(gh, gw), mode="bicubic", antialias=True, align_corners=False)
        pos = torch.cat([pos[:, :npre], tab.permute(0, 2, 3, 1).reshape(1, gh * gw, d).double()], dim=1)
    front = [sd["cls_token"].expand(b, -1, -1)] + ([sd["reg_token"].expand(b, -1, -1)] if nreg else [])
    x = torch.cat([*front, tok + pos], dim=1) if no_embed_class else torch.cat([*front, tok], dim=1) + pos
    s, hd, prefix = x.shape[1], d // heads, 1 + nreg

    def ln(t, wgt, bias):
        mu = t.mean(-1, keepdim=True)
        var = ((t - mu) ** 2).mean(-1, keepdim=True)
        return (t - mu) / torch.sqrt(var + 1e-6) * wgt + bias

    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    roll, last = None, None
    for i in range(depth):
        pre = f"blocks.{i}."
        a = ln(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"])
        wq, bq = sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]
        outs, ps = [], []
        for hh in range(heads):
            q = a @ wq[hh * hd:(hh + 1) * hd].T + bq[hh * hd:(hh + 1) * hd]
            k = a @ wq[d + hh * hd:d + (hh + 1) * hd].T + bq[d + hh * hd:d + (hh + 1) * hd]
            v = a @ wq[2 * d + hh * hd:2 * d + (hh + 1) * hd].T + bq[2 * d + hh * hd:2 * d + (hh + 1) * hd]
            p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), -1)
            ps.append(p)
            outs.append(p @ v)
        last = torch.stack(ps, 1)  # [B, H, S, S]
        mean = sum(ps) / heads
        prev = torch.eye(s, dtype=torch.float64).expand(b, s, s) if roll is None else roll
        roll = 0.5 * (mean @ prev) + 0.5 * prev
        a = torch.cat(outs, -1) @ sd[pre + "attn.proj.weight"].T + sd[pre + "attn.proj.bias"]
        x = x + (a * sd[pre + "ls1.gamma"] if pre + "ls1.gamma" in sd else a)
        a = ln(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"])
        w1, b1, w2 = sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"], sd[pre + "mlp.fc2.weight"]
        if w1.shape[0] == 2 * w2.shape[1]:  # packed SwiGLU: the gate is the FIRST half of fc1's rows
            hid = w2.shape[1]
            gate, val = a @ w1[:hid].T + b1[:hid], a @ w1[hid:].T + b1[hid:]
            a = gate / (1.0 + torch.exp(-gate)) * val
        else:
            a = a @ w1.T + b1
            a = 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))
        a = a @ w2.T + sd[pre + "mlp.fc2.bias"]
        x = x + (a * sd[pre + "ls2.gamma"] if pre + "ls2.gamma" in sd else a)
    if kind == "class":
        return last[:, :, 0, prefix:].reshape(b, heads, gh, gw), last[:, :, 0, :prefix].sum(-1)
    return roll[:, 0, prefix:].reshape(b, gh, gw), roll[:, 0]


def maps64_of(vit, imgs: torch.Tensor, kind: str) -> tuple[torch.Tensor, torch.Tensor]:
    """:func:`maps64` with the arguments read off a ``VisionTransformer``."""
    return maps64(vit.state_dict(), imgs, kind, heads=vit.num_heads, patch=vit.patch_size, native_grid=vit.native_grid,
                  no_embed_class=vit.no_embed_class, prefix_pos_embed=vit.prefix_pos_embed)


def map_error(got, ref64: torch.Tensor) -> float:
    """``max |m - m64| / max m64`` over the whole batch of maps."""
    got = torch.as_tensor(got).detach().cpu().double()
    return float((got - ref64).abs().max() / ref64.max())

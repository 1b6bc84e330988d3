"""Vision Transformer backbones (the models the reference's ``TimmBackbone`` builds through timm, ``vanilla.py``), restated in plain
torch: timm's ``VisionTransformer`` with ``num_classes=0`` and ``global_pool="token"`` -- no head, no ``fc_norm``; the output is the
class token of the final norm, ``[B, D]``.  Parameter names and shapes are timm's, so its checkpoints load with ``strict=True``;
``UNI`` is ViT-L/16 with LayerScale (``init_values=1e-5``) and ``dynamic_img_size``.  The pathology foundation models (``UNI2``,
``H-optimus-0`` / ``-1``, ``prov-gigapath``) add timm's ``reg_tokens``, ``no_embed_class`` and ``mlp_layer=SwiGLUPacked``; ``Virchow`` /
``Virchow2`` (ViT-H/14, 80 dimensions per head) add the class + mean-patch output (``global_pool="token_mean"``) and timm's default
position table beside register tokens (``prefix_pos_embed``).

The fp16 / bf16 forward on the hand-written kernels is :class:`~tiatoolbox_amd.models.architecture.vit_fused.FusedViT`.
"""

from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F  # noqa: N812
from torch import nn

# name -> constructor arguments (timm's `vit_*_patch16_224`; UNI: MahmoodLab/UNI's timm configuration)
VIT_CONFIGS: dict[str, dict] = {
    "UNI": {"embed_dim": 1024, "depth": 24, "num_heads": 16, "mlp_dim": 4096, "patch_size": 16, "img_size": 224,
            "init_values": 1e-5, "dynamic_img_size": True},
    "vit_large_patch16_224": {"embed_dim": 1024, "depth": 24, "num_heads": 16, "mlp_dim": 4096, "patch_size": 16, "img_size": 224},
    "vit_base_patch16_224": {"embed_dim": 768, "depth": 12, "num_heads": 12, "mlp_dim": 3072, "patch_size": 16, "img_size": 224},
    "vit_small_patch16_224": {"embed_dim": 384, "depth": 12, "num_heads": 6, "mlp_dim": 1536, "patch_size": 16, "img_size": 224},
    # the foundation models' published timm configurations (ViT-H / ViT-g widths); `mlp_dim` is the packed fc1 width, int(1536 * 5.33334)
    "UNI2": {"embed_dim": 1536, "depth": 24, "num_heads": 24, "mlp_dim": 8192, "patch_size": 14, "img_size": 224, "init_values": 1e-5,
             "reg_tokens": 8, "no_embed_class": True, "dynamic_img_size": True, "mlp_layer": "swiglu_packed"},
    "H-optimus-0": {"embed_dim": 1536, "depth": 40, "num_heads": 24, "mlp_dim": 8192, "patch_size": 14, "img_size": 224, "init_values": 1e-5,
                    "reg_tokens": 4, "no_embed_class": True, "mlp_layer": "swiglu_packed"},
    "H-optimus-1": {"embed_dim": 1536, "depth": 40, "num_heads": 24, "mlp_dim": 8192, "patch_size": 14, "img_size": 224, "init_values": 1e-5,
                    "reg_tokens": 4, "no_embed_class": True, "mlp_layer": "swiglu_packed"},
    "prov-gigapath": {"embed_dim": 1536, "depth": 40, "num_heads": 24, "mlp_dim": 8192, "patch_size": 16, "img_size": 224, "init_values": 1e-5,
                      "mlp_layer": "swiglu_packed"},
}
# paige-ai/Virchow and Virchow2's published timm configurations (`vit_huge_patch14_224`, SwiGLUPacked / SiLU, mlp_ratio 5.3375:
# fc1 width int(1280 * 5.3375) = 6832); 1280 / 16 = 80 per head; the embedding is cat(class token, mean of the patch tokens).
# `create_vit` builds them and `FusedViT` runs them.  They are a table of their own because `VIT_CONFIGS` is the list of names
# `TimmBackbone` accepts, and `TimmBackbone` refuses these two (`tests/test_vit_foundation.py` pins that).
VIRCHOW_CONFIGS: dict[str, dict] = {
    "Virchow": {"embed_dim": 1280, "depth": 32, "num_heads": 16, "mlp_dim": 6832, "patch_size": 14, "img_size": 224, "init_values": 1e-5,
                "dynamic_img_size": True, "mlp_layer": "swiglu_packed", "global_pool": "token_mean"},
    "Virchow2": {"embed_dim": 1280, "depth": 32, "num_heads": 16, "mlp_dim": 6832, "patch_size": 14, "img_size": 224, "init_values": 1e-5,
                 "reg_tokens": 4, "prefix_pos_embed": True, "dynamic_img_size": True, "mlp_layer": "swiglu_packed",
                 "global_pool": "token_mean"},
}
MLP_LAYERS = ("mlp", "swiglu_packed")
GLOBAL_POOLS = ("token", "token_mean")
ATTENTION_KINDS = ("class", "rollout")  # the maps of `forward_with_attention` (the engines' run kwarg `return_attention`)
LN_EPS = 1e-6


def resample_pos_embed(pos_embed: torch.Tensor, native_grid: tuple[int, int], grid: tuple[int, int], *, dynamic: bool,
                       num_prefix: int = 1) -> torch.Tensor:
    """``pos_embed`` ``[1, num_prefix + g0h * g0w, D]`` for a ``grid`` of patches, in float32: the ``num_prefix`` leading entries (the
    class entry; none for a ``no_embed_class`` table, which is the grid alone) as they are, the grid part resampled with
    ``F.interpolate(mode="bicubic", antialias=True, align_corners=False)`` (timm's ``resample_abs_pos_embed``).  At the native grid
    this is ``pos_embed`` itself (no arithmetic); any other grid needs ``dynamic`` (``dynamic_img_size``) and
    raises ``ValueError`` without it.  The one helper of the plain module and of the fused graph."""
    grid, native_grid = tuple(grid), tuple(native_grid)
    if grid == native_grid:
        return pos_embed
    if not dynamic:
        msg = (f"This VisionTransformer takes a {native_grid[0]} x {native_grid[1]} grid of patches only; got {grid[0]} x {grid[1]} "
               "(dynamic_img_size is off).")
        raise ValueError(msg)
    dim = pos_embed.shape[-1]
    cls, tab = pos_embed[:, :num_prefix], pos_embed[:, num_prefix:]
    tab = tab.to(torch.float32).reshape(1, native_grid[0], native_grid[1], dim).permute(0, 3, 1, 2)
    tab = F.interpolate(tab, size=grid, mode="bicubic", antialias=True, align_corners=False)
    tab = tab.permute(0, 2, 3, 1).reshape(1, grid[0] * grid[1], dim)
    return torch.cat([cls.to(torch.float32), tab], dim=1).to(pos_embed.dtype)


class PatchEmbed(nn.Module):
    def __init__(self, patch_size: int, embed_dim: int) -> None:
        super().__init__()
        self.proj = nn.Conv2d(3, embed_dim, kernel_size=patch_size, stride=patch_size)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.proj(x).flatten(2).transpose(1, 2)  # [B, g, D], patches in raster order


class Attention(nn.Module):
    def __init__(self, dim: int, num_heads: int) -> None:
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        b, s, d = x.shape
        qkv = self.qkv(x).reshape(b, s, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)  # [B, H, S, D/H] each
        attn = ((q * self.scale) @ k.transpose(-2, -1)).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(b, s, d))


class LayerScale(nn.Module):
    def __init__(self, dim: int, init_values: float) -> None:
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x * self.gamma


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int) -> None:
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()  # the exact (erf) form
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc2(self.act(self.fc1(x)))


class SwiGLUPacked(nn.Module):
    """timm's ``SwiGLUPacked`` (``GluMlp`` with ``act_layer=SiLU``, ``gate_last=False``): ONE ``fc1`` of width ``hidden`` whose first
    half is the gate, ``fc2(silu(x1) * x2)`` on the ``hidden / 2`` products."""

    def __init__(self, dim: int, hidden: int) -> None:
        super().__init__()
        if hidden % 2 != 0:
            msg = f"SwiGLUPacked: the packed fc1 width {hidden} is odd."
            raise ValueError(msg)
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.SiLU()
        self.fc2 = nn.Linear(hidden // 2, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x1, x2 = self.fc1(x).chunk(2, dim=-1)
        return self.fc2(self.act(x1) * x2)


class Block(nn.Module):
    def __init__(self, dim: int, num_heads: int, mlp_dim: int, init_values: float | None, mlp_layer: str = "mlp") -> None:
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = Attention(dim, num_heads)
        self.ls1 = LayerScale(dim, init_values) if init_values else nn.Identity()
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = SwiGLUPacked(dim, mlp_dim) if mlp_layer == "swiglu_packed" else Mlp(dim, mlp_dim)
        self.ls2 = LayerScale(dim, init_values) if init_values else nn.Identity()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class VisionTransformer(nn.Module):
    """``forward(imgs [B, 3, H, W]) -> [B, D]``: the class token of ``norm(blocks(tokens))``; with ``global_pool="token_mean"``
    ``[B, 2D]``: the class token beside the mean of the patch tokens (register tokens left out), ``cat([x[:, 0], x[:, 1 + R:].mean(1)])``.

    ``reg_tokens`` register tokens follow the class token (``reg_token [1, R, D]``); with ``no_embed_class`` the position table is the
    grid alone (``[1, g0 * g0, D]``), added to the patch tokens before the prefix is prepended: ``cat([cls, reg, patches + pos])``.
    ``mlp_layer="swiglu_packed"`` puts :class:`SwiGLUPacked` in the blocks (``mlp_dim`` is then the packed ``fc1`` width).
    ``prefix_pos_embed`` is timm's default form beside register tokens (``no_embed_class=False``): ``pos_embed`` is
    ``[1, 1 + R + g0 * g0, D]`` and the sequence is ``cat([cls, reg, patches]) + pos``; resampling leaves the ``1 + R`` prefix entries
    as they are."""

    def __init__(self, *, embed_dim: int, depth: int, num_heads: int, mlp_dim: int, patch_size: int = 16, img_size: int = 224,
                 init_values: float | None = None, dynamic_img_size: bool = False, reg_tokens: int = 0, no_embed_class: bool = False,
                 mlp_layer: str = "mlp", global_pool: str = "token", prefix_pos_embed: bool = False) -> None:
        super().__init__()
        if mlp_layer not in MLP_LAYERS:
            msg = f"VisionTransformer: mlp_layer is one of {MLP_LAYERS}; got {mlp_layer!r}."
            raise ValueError(msg)
        if global_pool not in GLOBAL_POOLS:
            msg = f"VisionTransformer: global_pool is one of {GLOBAL_POOLS}; got {global_pool!r}."
            raise ValueError(msg)
        if prefix_pos_embed and no_embed_class:
            msg = "VisionTransformer: prefix_pos_embed (a table with class and register entries) contradicts no_embed_class=True."
            raise ValueError(msg)
        if reg_tokens < 0 or (reg_tokens and not (no_embed_class or prefix_pos_embed)):
            msg = (f"VisionTransformer: reg_tokens={reg_tokens} needs no_embed_class=True (a grid-only position table) or "
                   "prefix_pos_embed=True (a table with class and register entries) and cannot be negative.")
            raise ValueError(msg)
        if embed_dim % num_heads != 0 or img_size % patch_size != 0:
            msg = f"VisionTransformer: embed_dim {embed_dim} / heads {num_heads} or img_size {img_size} / patch {patch_size} does not divide."
            raise ValueError(msg)
        self.embed_dim, self.num_heads, self.patch_size = embed_dim, num_heads, patch_size
        self.dynamic_img_size = dynamic_img_size
        self.reg_tokens, self.no_embed_class, self.mlp_layer = reg_tokens, no_embed_class, mlp_layer
        self.global_pool, self.prefix_pos_embed = global_pool, prefix_pos_embed
        # entries of `pos_embed` in front of the grid: none, the class entry, or (prefix_pos_embed) the class and register entries
        self.pos_prefix = 0 if no_embed_class else 1 + (reg_tokens if prefix_pos_embed else 0)
        g0 = img_size // patch_size
        self.native_grid = (g0, g0)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        if reg_tokens:
            self.reg_token = nn.Parameter(torch.zeros(1, reg_tokens, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.pos_prefix + g0 * g0, embed_dim))
        self.patch_embed = PatchEmbed(patch_size, embed_dim)
        self.blocks = nn.Sequential(*[Block(embed_dim, num_heads, mlp_dim, init_values, mlp_layer) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=LN_EPS)
        self._pos_cache: dict[tuple, torch.Tensor] = {}
        if self.pos_embed.device.type != "meta":
            self.init_weights()

    def init_weights(self) -> None:
        """timm's: truncated normal (std 0.02) on the weights and ``pos_embed``, zero biases, ``cls_token`` (and ``reg_token``) std
        1e-6, LayerNorm ones / zeros; LayerScale keeps ``init_values``."""
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        if self.reg_tokens:
            nn.init.normal_(self.reg_token, std=1e-6)
        for mod in self.modules():
            if isinstance(mod, (nn.Linear, nn.Conv2d)):
                nn.init.trunc_normal_(mod.weight, std=0.02)
                nn.init.zeros_(mod.bias)
            elif isinstance(mod, nn.LayerNorm):
                nn.init.ones_(mod.weight)
                nn.init.zeros_(mod.bias)

    def grid_of(self, height: int, width: int) -> tuple[int, int]:
        p = self.patch_size
        if height % p != 0 or width % p != 0:
            msg = f"VisionTransformer: the input size {height} x {width} is no multiple of the patch size {p}."
            raise ValueError(msg)
        return height // p, width // p

    def pos_embed_for(self, grid: tuple[int, int]) -> torch.Tensor:
        """``pos_embed`` for ``grid`` (:func:`resample_pos_embed`), resampled once per grid shape and cached until the parameter
        changes (a load, a cast or a move makes a new version, dtype or device)."""
        grid = tuple(grid)
        if grid == self.native_grid:
            return self.pos_embed
        pe = self.pos_embed
        # (a tensor made under inference_mode keeps no version counter; a load clears the cache itself, below)
        key = (grid, pe.device, pe.dtype, None if pe.is_inference() else pe._version, pe.data_ptr())  # noqa: SLF001
        hit = self._pos_cache.get(grid)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, resample_pos_embed(pe.detach(), self.native_grid, grid, dynamic=self.dynamic_img_size,
                                                   num_prefix=self.pos_prefix))
            self._pos_cache[grid] = hit
        return hit[1]

    def _load_from_state_dict(self, *args, **kwargs) -> None:
        self._pos_cache.clear()  # a new `pos_embed` is on its way
        super()._load_from_state_dict(*args, **kwargs)

    def forward(self, imgs: torch.Tensor) -> torch.Tensor:
        grid = self.grid_of(imgs.shape[-2], imgs.shape[-1])
        pos = self.pos_embed_for(grid)  # (refuses an off-grid size before any arithmetic)
        x = self.patch_embed(imgs)
        if self.no_embed_class:
            prefix = [self.cls_token.expand(x.shape[0], -1, -1)]
            if self.reg_tokens:
                prefix.append(self.reg_token.expand(x.shape[0], -1, -1))
            x = torch.cat([*prefix, x + pos], dim=1)
        else:
            prefix = [self.cls_token.expand(x.shape[0], -1, -1)]
            if self.reg_tokens:  # (prefix_pos_embed: the table has an entry for every prefix token)
                prefix.append(self.reg_token.expand(x.shape[0], -1, -1))
            x = torch.cat([*prefix, x], dim=1) + pos
        x = self.norm(self.blocks(x))
        if self.global_pool == "token_mean":
            return torch.cat([x[:, 0], x[:, 1 + self.reg_tokens:].mean(1)], dim=-1)
        return x[:, 0]

    def forward_with_attention(self, imgs: torch.Tensor, kind: str, head_fusion: str = "mean", discard_ratio: float = 0.0, *,
                               trace: dict | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """``(forward(imgs), maps)``: the features bit for bit, and float32 attention maps on the patch grid ``(gh, gw)`` of the input.
        With ``S`` tokens, the prefix ``P = 1 + reg_tokens`` (class token, then registers), ``H`` heads and ``q``, ``k`` the ``qkv``
        Linear's own output of a block (in the module's dtype):

        * ``kind="class"`` -> ``[B, H, gh, gw]``: in the LAST block, per head, ``p = softmax_j(scale * q[0] . k[j])`` over all ``S``
          keys, and ``p[P:]`` on the grid.  Not renormalised: a map sums to 1 minus the mass the class token puts on the prefix tokens.
        * ``kind="rollout"`` -> ``[B, gh, gw]``: attention rollout (Abnar & Zuidema 2020) with mean head fusion and nothing discarded:
          ``A_l = (1 / H) sum_h softmax(scale * Q_h K_h^T)`` (heads added in ascending order), ``R_1 = A_1 / 2 + I / 2``,
          ``R_l = (A_l R_{l-1}) / 2 + R_{l-1} / 2``, no renormalisation (the rows sum to 1 already); the map is ``R_L[0, P:]``.

          ``head_fusion`` ("mean" | "max" | "min") and ``discard_ratio`` (``0 <= r < 1``) are the other forms of the rollout
          (``models/engine/_rollout_options.py`` states them): the heads' maximum or minimum in place of their mean; per block the
          ``k = min(int(r S^2), S^2 - 1)`` smallest entries of the fused ``S x S`` matrix set to 0 (``torch.kthvalue`` on the flattened
          matrix gives ``v``; everything ``<= v`` goes, entry ``(0, 0)`` never); then ``A^ = (F' + I) / 2`` with every row divided by
          its sum, ``R_1 = A^_1``, ``R_l = A^_l R_{l-1}``.  "mean" with ``k == 0`` is the path above, untouched.  A ``ValueError``
          that names the option for anything else, and for a non-default value beside ``kind="class"``.  ``trace``, a dict, receives
          the per-block lists ``"fused"`` (``F``) and ``"normalised"`` (``A^``) of that route.

        The probabilities are the softmax of the module's own scores, widened to float32; the head mean and ``R`` are float32
        throughout.  A hook records what each block's ``qkv`` returns while ``forward`` itself runs, so the features cannot differ."""
        from tiatoolbox_amd.models.engine import _rollout_options as ro

        if kind not in ATTENTION_KINDS:
            msg = f"VisionTransformer.forward_with_attention: kind is one of {ATTENTION_KINDS}; got {kind!r}."
            raise ValueError(msg)
        head_fusion, discard_ratio = ro.check_options(head_fusion, discard_ratio, who="VisionTransformer.forward_with_attention")
        if kind != "rollout" and not ro.is_default(head_fusion, discard_ratio):
            msg = (f"VisionTransformer.forward_with_attention: attention_head_fusion={head_fusion!r} / attention_discard_ratio="
                   f"{discard_ratio!r} apply to kind=\"rollout\" only; got kind={kind!r}.")
            raise ValueError(msg)
        gh, gw = self.grid_of(imgs.shape[-2], imgs.shape[-1])
        prefix, heads = 1 + self.reg_tokens, self.num_heads
        state: dict[str, torch.Tensor] = {}

        def probs(attn: Attention, qkv: torch.Tensor, rows: int | None) -> torch.Tensor:  # float32 [B, H, rows or S, S]
            b, s, _ = qkv.shape
            q, k, _ = qkv.reshape(b, s, 3, heads, attn.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
            return ((q[:, :, :rows] * attn.scale) @ k.transpose(-2, -1)).softmax(dim=-1).to(torch.float32)

        def tap(attn: Attention, last: bool):  # noqa: ANN202, FBT001
            @torch.no_grad()
            def hook(_mod: nn.Module, _inp: tuple, qkv: torch.Tensor) -> None:
                if kind == "class":
                    if last:
                        state["class"] = probs(attn, qkv, 1)[:, :, 0, prefix:]
                    return
                p = probs(attn, qkv, None)
                k = ro.discard_count(discard_ratio, p.shape[-1])
                if head_fusion != "mean" or k:
                    a = _discard_normalise(_fuse_heads(p, head_fusion), k, trace)
                    r = state.get("r")
                    state["r"] = a if r is None else a @ r
                    return
                a = p[:, 0]
                for h in range(1, heads):  # ascending head order, float32
                    a = a + p[:, h]
                a = a / heads
                r = state.get("r")
                if r is None:
                    r = torch.eye(a.shape[-1], dtype=torch.float32, device=a.device).expand_as(a)
                state["r"] = 0.5 * (a @ r) + 0.5 * r
            return hook

        handles = [blk.attn.qkv.register_forward_hook(tap(blk.attn, i == len(self.blocks) - 1)) for i, blk in enumerate(self.blocks)]
        try:
            feats = type(self).forward(self, imgs)  # (the class's own forward: `capturing_attention` shadows the instance's)
        finally:
            for h in handles:
                h.remove()
        if kind == "class":
            return feats, state["class"].reshape(-1, heads, gh, gw).contiguous()
        return feats, state["r"][:, 0, prefix:].reshape(-1, gh, gw).contiguous()

    @contextlib.contextmanager
    def capturing_attention(self, kind: str, head_fusion: str = "mean", discard_ratio: float = 0.0):  # noqa: ANN201
        """Inside the scope every CALL of this module (``model(x)`` of whatever model holds it) returns ``forward``'s features and appends
        the maps of :meth:`forward_with_attention` to the list the scope yields -- how an engine gets both from a model's own
        ``infer_batch``.  ``forward`` itself is not touched: the scope shadows it on the instance and removes the shadow again."""
        maps: list[torch.Tensor] = []

        def forward(imgs: torch.Tensor) -> torch.Tensor:
            feats, m = self.forward_with_attention(imgs, kind, head_fusion, discard_ratio)
            maps.append(m)
            return feats

        self.__dict__["forward"] = forward
        try:
            yield maps
        finally:
            self.__dict__.pop("forward", None)


def _fuse_heads(p: torch.Tensor, head_fusion: str) -> torch.Tensor:
    """``[B, H, S, S]`` float32 -> ``[B, S, S]``: the heads' mean (added in ascending order, one division), maximum or minimum."""
    if head_fusion == "max":
        return p.amax(1)
    if head_fusion == "min":
        return p.amin(1)
    a = p[:, 0]
    for h in range(1, p.shape[1]):
        a = a + p[:, h]
    return a / p.shape[1]


def _discard_normalise(f: torch.Tensor, k: int, trace: dict | None) -> torch.Tensor:
    """``A^`` ``[B, S, S]`` of the fused matrices ``f`` (``_rollout_options``: ``discard`` and ``normalise``).  The row sums follow the
    stated order -- 64 strided partial sums, folded by the exchange tree -- so that this route, the NumPy statement and the kernel
    agree bit for bit from the same ``f``."""
    b, s, _ = f.shape
    kept = f
    if k:
        v = torch.kthvalue(f.reshape(b, s * s), k, dim=1).values.reshape(b, 1, 1)
        drop = f <= v
        drop[:, 0, 0] = False
        kept = torch.where(drop, torch.zeros((), dtype=f.dtype, device=f.device), f)
    a = (kept + torch.eye(s, dtype=f.dtype, device=f.device)) * 0.5
    parts = torch.zeros((b, s, 64), dtype=f.dtype, device=f.device)
    for j0 in range(0, s, 64):
        chunk = a[:, :, j0:j0 + 64]
        parts[:, :, :chunk.shape[-1]] += chunk
    lanes = torch.arange(64, device=f.device)
    for off in (32, 16, 8, 4, 2, 1):
        parts = parts + parts[:, :, lanes ^ off]
    a = a / parts[:, :, :1]
    if trace is not None:
        trace.setdefault("fused", []).append(f)
        trace.setdefault("normalised", []).append(a)
    return a


def create_vit(name: str, *, device: torch.device | str | None = None) -> VisionTransformer:
    """The configuration ``name`` (``VIT_CONFIGS``, or ``VIRCHOW_CONFIGS``: ``Virchow`` / ``Virchow2``); ``device="meta"`` builds the shapes
    only.  The Virchow names are no ``TimmBackbone`` names; to run one in an engine, put it into a backbone of another name:
    ``m = TimmBackbone("vit_small_patch16_224"); m.feat_extract = create_vit("Virchow2")`` (then load its weights)."""
    cfg = vit_config(name)
    if device is not None:
        with torch.device(device):
            return VisionTransformer(**cfg)
    return VisionTransformer(**cfg)


def vit_config(name: str) -> dict:
    """The constructor arguments of ``name`` from ``VIT_CONFIGS`` or ``VIRCHOW_CONFIGS``."""
    for table in (VIT_CONFIGS, VIRCHOW_CONFIGS):
        if name in table:
            return table[name]
    msg = f"Backbone `{name}` is not supported."
    raise ValueError(msg)

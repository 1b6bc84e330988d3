"""Vision Transformer backbones (``architecture/vit.py``, ``TimmBackbone``, the registry names, ``DeepFeatureExtractor``) on the CPU,
and the host-side LayerScale fold of ``FusedViT``."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from _vit_ref import forward64, randomise, tiny_vit

PARAMETERS = {"UNI": 303_350_784, "vit_large_patch16_224": 303_301_632, "vit_base_patch16_224": 85_798_656,
              "vit_small_patch16_224": 21_665_664}


@pytest.mark.parametrize("name", sorted(PARAMETERS))
def test_parameter_counts(name):
    from tiatoolbox_amd.models.architecture.vit import create_vit

    vit = create_vit(name, device="meta")  # shapes only: nothing is allocated
    assert all(p.device.type == "meta" for p in vit.parameters())
    assert sum(p.numel() for p in vit.parameters()) == PARAMETERS[name]
    assert vit.dynamic_img_size == (name == "UNI")


def _expected_keys(depth: int, layer_scale: bool) -> list[str]:
    keys = ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(depth):
        b = f"blocks.{i}."
        keys += [b + "norm1.weight", b + "norm1.bias", b + "attn.qkv.weight", b + "attn.qkv.bias", b + "attn.proj.weight",
                 b + "attn.proj.bias"]
        keys += [b + "ls1.gamma"] if layer_scale else []
        keys += [b + "norm2.weight", b + "norm2.bias", b + "mlp.fc1.weight", b + "mlp.fc1.bias", b + "mlp.fc2.weight", b + "mlp.fc2.bias"]
        keys += [b + "ls2.gamma"] if layer_scale else []
    return [*keys, "norm.weight", "norm.bias"]


@pytest.mark.parametrize("layer_scale", [False, True])
def test_state_dict_keys_are_timms(layer_scale):
    vit = tiny_vit(layer_scale=layer_scale)
    sd = vit.state_dict()
    assert list(sd) == _expected_keys(2, layer_scale)
    assert sd["cls_token"].shape == (1, 1, 128) and sd["pos_embed"].shape == (1, 5, 128)
    assert sd["patch_embed.proj.weight"].shape == (128, 3, 16, 16) and sd["blocks.0.attn.qkv.weight"].shape == (384, 128)
    assert sd["blocks.1.mlp.fc1.weight"].shape == (512, 128) and sd["blocks.1.mlp.fc2.weight"].shape == (128, 512)
    # strict round trip into a differently initialised model
    other = tiny_vit(layer_scale=layer_scale, seed=5)
    assert not torch.equal(other.blocks[0].attn.qkv.weight, vit.blocks[0].attn.qkv.weight)
    other.load_state_dict(sd, strict=True)
    x = torch.randn(2, 3, 32, 32)
    with torch.inference_mode():
        assert torch.equal(other(x), vit(x))
    with pytest.raises(RuntimeError):
        tiny_vit(layer_scale=not layer_scale).load_state_dict(sd, strict=True)


def test_initialisation_is_timms():
    from tiatoolbox_amd.models.architecture.vit import VisionTransformer

    torch.manual_seed(0)
    vit = VisionTransformer(embed_dim=128, depth=2, num_heads=2, mlp_dim=512, img_size=32, init_values=1e-5)
    assert float(vit.blocks[0].attn.qkv.bias.detach().abs().max()) == 0.0 and float(vit.patch_embed.proj.bias.detach().abs().max()) == 0.0
    assert torch.equal(vit.norm.weight, torch.ones(128)) and float(vit.blocks[1].norm2.bias.detach().abs().max()) == 0.0
    assert torch.equal(vit.blocks[0].ls1.gamma, torch.full((128,), 1e-5))
    w = vit.blocks[0].mlp.fc1.weight.detach()
    assert 0.015 < float(w.std()) < 0.025 and float(w.abs().max()) <= 2.0  # (timm truncates at the absolute bounds +-2)
    assert 0.0 < float(vit.cls_token.detach().abs().max()) < 1e-4 and 0.01 < float(vit.pos_embed.detach().std()) < 0.03


@pytest.mark.parametrize("layer_scale", [False, True])
@pytest.mark.parametrize("size", [(32, 32), (48, 64)])
def test_forward_matches_float64_restatement(size, layer_scale):
    vit = tiny_vit(layer_scale=layer_scale, dynamic=True)
    x = torch.randn((2, 3, *size), generator=torch.Generator().manual_seed(3))
    with torch.inference_mode():
        got = vit(x)
    ref = forward64(vit.state_dict(), x, heads=2, patch=16, native_grid=(2, 2))
    assert got.shape == (2, 128) and got.dtype == torch.float32
    err = float((got.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"{size} layer_scale={layer_scale}: {err:.3e}")
    assert err <= 1e-5
    # the blocks are visible in the output: without them the features differ grossly
    sd0 = {k: v for k, v in vit.state_dict().items() if not k.startswith("blocks.1.")}
    assert float((forward64(sd0, x, heads=2, patch=16, native_grid=(2, 2)) - ref).abs().max()) > 1e-2 * float(ref.abs().max())


def test_pos_embed_resampling():
    from tiatoolbox_amd.models.architecture.vit import resample_pos_embed

    vit = tiny_vit(dynamic=True)
    assert vit.pos_embed_for((2, 2)) is vit.pos_embed
    assert resample_pos_embed(vit.pos_embed, (2, 2), (2, 2), dynamic=False) is vit.pos_embed  # bit for bit: the tensor itself
    up = vit.pos_embed_for((3, 4))
    assert up.shape == (1, 13, 128) and torch.equal(up[:, 0], vit.pos_embed[:, 0])
    assert vit.pos_embed_for((3, 4)) is up  # cached per grid shape
    with torch.no_grad():
        vit.pos_embed.mul_(2.0)  # a new version of the parameter: resampled again
    assert torch.allclose(vit.pos_embed_for((3, 4)), 2.0 * up, rtol=1e-6, atol=1e-7)
    fixed = tiny_vit(dynamic=False)
    with pytest.raises(ValueError, match="dynamic_img_size"):
        fixed(torch.zeros(1, 3, 48, 64))
    with pytest.raises(ValueError, match="multiple of the patch size"):
        vit(torch.zeros(1, 3, 40, 32))
    assert fixed(torch.zeros(1, 3, 32, 32)).shape == (1, 128)


def test_timm_backbone_and_registry():
    from tiatoolbox_amd.models.architecture import get_pretrained_model
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone
    from tiatoolbox_amd.models.architecture.vit import VisionTransformer
    from tiatoolbox_amd.models.models_abc import ModelABC

    for bad in ("resnet50", "vit_huge_patch14_224", "uni"):
        with pytest.raises(ValueError, match=f"Backbone `{bad}` is not supported."):
            TimmBackbone(bad)
    model, ioconfig = get_pretrained_model("vit_small_patch16_224")
    assert type(model) is TimmBackbone and isinstance(model, ModelABC) and ioconfig is None
    assert isinstance(model.feat_extract, VisionTransformer) and model.feat_extract.embed_dim == 384
    again, _ = get_pretrained_model("vit_small_patch16_224")
    assert torch.equal(again.feat_extract.blocks[3].mlp.fc2.weight, model.feat_extract.blocks[3].mlp.fc2.weight)  # seeded
    other, _ = get_pretrained_model("vit_small_patch16_224", seed=1)
    assert not torch.equal(other.feat_extract.blocks[3].mlp.fc2.weight, model.feat_extract.blocks[3].mlp.fc2.weight)


def test_timm_backbone_pretrained_reads_local_weights_only(tmp_path, monkeypatch, caplog):
    """``pretrained=True``: ``<name>.pth`` (a timm state dict: no ``feat_extract.`` prefix) from the local weight directory, strict;
    without the file the registry's "no local weights" warning and the seeded initialisation."""
    import logging

    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    monkeypatch.setenv("TIA_WEIGHTS_DIR", str(tmp_path))
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    monkeypatch.delenv("TIATOOLBOX_HOME", raising=False)
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        torch.manual_seed(0)
        first = TimmBackbone("vit_small_patch16_224", pretrained=True)
    assert sum("No local weights for `vit_small_patch16_224`" in r.getMessage() for r in caplog.records) == 1
    sd = {k: v.clone() for k, v in first.feat_extract.state_dict().items()}
    sd["norm.bias"] += 1.0
    torch.save(sd, tmp_path / "vit_small_patch16_224.pth")
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        second = TimmBackbone("vit_small_patch16_224", pretrained=True)
    assert not caplog.records
    assert torch.equal(second.feat_extract.norm.bias, sd["norm.bias"])


def test_deep_feature_extractor_vit_cpu():
    from tiatoolbox_amd.models import DeepFeatureExtractor, IOPatchPredictorConfig
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    eng = DeepFeatureExtractor("vit_small_patch16_224", batch_size=2)
    assert type(eng.model) is TimmBackbone and eng.ioconfig is None
    randomise(eng.model.feat_extract)
    patches = np.random.default_rng(0).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    cfg = IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                 stride_shape=(224, 224))
    out = eng.run(patches, patch_mode=True, ioconfig=cfg)
    assert set(out) == {"probabilities"} and out["probabilities"].shape == (2, 384)
    with torch.inference_mode():
        ref = eng.model.eval()(torch.from_numpy(patches).float().permute(0, 3, 1, 2)).numpy()
    np.testing.assert_allclose(out["probabilities"], ref, atol=1e-5)


def test_fused_vit_folds_layer_scale_in_float32():
    """``FusedViT`` keeps ``gamma * W`` and ``gamma * b`` in float32 until ``prepare`` rounds them: applied to a vector they reproduce
    ``gamma * (W a + b)`` to float32 rounding (against float64), and the patch weight is the ``(ky, kx, c)`` permutation."""
    from tiatoolbox_amd.models.architecture.unet_fused import UnsupportedLayerError
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    vit = tiny_vit(layer_scale=True)
    fused = FusedViT(vit)  # host only: the constructor folds and checks, nothing is launched
    g = torch.Generator().manual_seed(1)
    for i, blk in enumerate(vit.blocks):
        for name, lin, ls, width in (("proj", blk.attn.proj, blk.ls1, 128), ("fc2", blk.mlp.fc2, blk.ls2, 512)):
            layer = fused.layers[i][name]
            assert layer.weight32.dtype == torch.float32 and layer.bias32.dtype == torch.float32
            a = torch.randn(width, generator=g)
            ref = ls.gamma.double() * (lin.weight.double() @ a.double() + lin.bias.double())
            got = layer.weight32.double() @ a.double() + layer.bias32.double()
            bound = 2.0 ** -24 * float((lin.weight.detach().double().abs() @ a.double().abs() + lin.bias.detach().double().abs()).max()) * 1.5  # one float32 rounding of gamma * w and of gamma * b, gamma < 1.5
            assert float((got - ref).abs().max()) <= bound, (i, name)
            assert not torch.equal(layer.weight32, lin.weight)  # gamma in [0.5, 1.5): the fold is visible
        assert torch.equal(fused.layers[i]["qkv"].weight32, blk.attn.qkv.weight) and torch.equal(fused.layers[i]["fc1"].bias32, blk.mlp.fc1.bias)
    w = vit.patch_embed.proj.weight
    assert torch.equal(fused.patch.weight32.reshape(128, 16, 16, 3), w.permute(0, 2, 3, 1))
    with pytest.raises(RuntimeError, match="prepare"):
        fused(torch.zeros(1, 3, 32, 32))
    with pytest.raises(UnsupportedLayerError, match="head_dim 64"):
        FusedViT(tiny_vit(num_heads=4))
    with pytest.raises(UnsupportedLayerError, match="cout % 64"):
        FusedViT(tiny_vit(embed_dim=128, mlp_dim=96))

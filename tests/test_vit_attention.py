"""``return_attention``: the torch module's ``forward_with_attention`` against the float64 restatement of both map definitions, and the
engines' run kwarg on the CPU -- shapes, the untouched outputs, the refusals, the per-call rule, the gather under gloo."""

from __future__ import annotations

import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from _vit_attention_ref import map_error, maps64_of
from _vit_classifier_ref import timm_model, torch_vit_wrappers
from _vit_foundation_ref import TINY_REG, tiny_foundation
from _vit_ref import tiny_vit
from _vit_virchow_ref import TINY_V2, tiny_virchow

from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

U32 = 2.0 ** -24
MODELS = {"vit": lambda: tiny_vit(), "registers": lambda: tiny_foundation(TINY_REG), "virchow2": lambda: tiny_virchow(TINY_V2)}  # noqa: PLW0108
KINDS = ("class", "rollout")


def _images(vit, *, square: bool, n: int = 2, seed: int = 0) -> torch.Tensor:
    p = vit.patch_size
    h, w = (2 * p, 2 * p) if square else (3 * p, 2 * p)  # the native 2 x 2 grid, or a resampled 3 x 2 one
    return torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("square", [True, False], ids=["native", "resampled-3x2"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(MODELS))
def test_forward_with_attention_matches_the_float64_restatement(name, kind, square):
    """The float32 module's maps within ``64 * 2^-24 * max(map64)`` of the state-dict restatement (a depth-2 float32 module sits near
    1e-7); the features bit for bit ``forward``'s; a class map plus its prefix mass is 1, a rollout row sums to 1."""
    vit = MODELS[name]()
    x = _images(vit, square=square)
    with torch.inference_mode():
        feats, maps = vit.forward_with_attention(x, kind)
        assert torch.equal(feats, vit(x))
    gh, gw = x.shape[-2] // vit.patch_size, x.shape[-1] // vit.patch_size
    assert maps.dtype == torch.float32
    assert tuple(maps.shape) == ((2, vit.num_heads, gh, gw) if kind == "class" else (2, gh, gw))
    ref, extra = maps64_of(vit, x, kind)
    err = float((maps.double() - ref).abs().max())
    print(f"{name} {kind} {'square' if square else '3x2'}: max |m - m64| = {err:.3e}, bound {64 * U32 * float(ref.max()):.3e}, "
          f"max m64 = {float(ref.max()):.3e}")
    assert err <= 64 * U32 * float(ref.max())
    if kind == "class":  # not renormalised: the map and the mass on the class / register columns make the whole row
        total = maps.double().sum((-2, -1)) + extra
        assert float((total - 1).abs().max()) <= 64 * U32
        assert float(extra.min()) > 0
    else:
        assert float((extra.sum(-1) - 1).abs().max()) <= 1e-12  # (the float64 row itself)
        prefix = 1 + vit.reg_tokens
        assert float((maps.double().sum((-2, -1)) + extra[:, :prefix].sum(-1) - 1).abs().max()) <= 64 * U32


def test_forward_with_attention_refuses_another_kind_and_leaves_the_module_as_it_was():
    vit = tiny_vit()
    x = _images(vit, square=True)
    with pytest.raises(ValueError, match="kind is one of"):
        vit.forward_with_attention(x, "mean")
    before = len(vit.blocks[0].attn.qkv._forward_hooks)  # noqa: SLF001
    vit.forward_with_attention(x, "rollout")
    assert len(vit.blocks[0].attn.qkv._forward_hooks) == before == 0  # noqa: SLF001
    with vit.capturing_attention("class") as maps:
        feats = vit(x)
    assert len(maps) == 1 and torch.equal(feats, vit(x)) and "forward" not in vit.__dict__


def _backbone(vit):
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    with torch.device("meta"):
        model = TimmBackbone("vit_small_patch16_224")  # (the named trunk's shapes only: it is replaced)
    model.feat_extract = vit
    model.preproc_func = timm_preproc_func("vit_small_patch16_224")
    return model.eval()


def _cfg(vit):
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    side = 2 * vit.patch_size
    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(side, side),
                                  stride_shape=(side, side))


def _normalised(model, patches: np.ndarray) -> torch.Tensor:
    """The NCHW float32 batch the model sees: the hook's batched form of the uint8 patches."""
    return model.preproc_func.device_batch(torch.from_numpy(patches), torch.float32).permute(0, 3, 1, 2).contiguous()


def _patches(vit, n: int = 5, seed: int = 3) -> np.ndarray:
    p = vit.patch_size
    return np.random.default_rng(seed).integers(0, 256, (n, 2 * p, 2 * p, 3), dtype=np.uint8)


@pytest.mark.parametrize("name", list(MODELS))
def test_engine_returns_the_maps_beside_unchanged_features_and_only_when_asked(name):
    from tiatoolbox_amd.models.engine.deep_feature_extractor import DeepFeatureExtractor

    vit = MODELS[name]()
    eng = DeepFeatureExtractor(_backbone(vit), batch_size=2)
    patches, cfg = _patches(vit), _cfg(vit)
    plain = eng.run(patches, patch_mode=True, ioconfig=cfg)
    assert "attention" not in plain
    for kind in KINDS:
        out = eng.run(patches, patch_mode=True, ioconfig=cfg, return_attention=kind)
        assert out["attention"].dtype == np.float32
        assert out["attention"].shape == ((5, vit.num_heads, 2, 2) if kind == "class" else (5, 2, 2))
        assert np.array_equal(out["probabilities"], plain["probabilities"])
        ref, _ = maps64_of(vit, _normalised(eng.model, patches), kind)
        assert map_error(out["attention"], ref) <= 64 * U32
    after = eng.run(patches, patch_mode=True, ioconfig=cfg)  # decided per call
    assert "attention" not in after and eng.return_attention is None
    assert np.array_equal(after["probabilities"], plain["probabilities"])


def test_a_classifier_keeps_its_predictions():
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor

    model = timm_model()
    model.preproc_func = timm_preproc_func("vit_small_patch16_224")
    eng = PatchPredictor(model, batch_size=4)
    patches, cfg = _patches(model.feat_extract), _cfg(model.feat_extract)
    plain = eng.run(patches, patch_mode=True, ioconfig=cfg, return_probabilities=True)
    out = eng.run(patches, patch_mode=True, ioconfig=cfg, return_probabilities=True, return_attention="rollout")
    assert out["attention"].shape == (5, 2, 2)
    assert np.array_equal(out["predictions"], plain["predictions"]) and np.array_equal(out["probabilities"], plain["probabilities"])
    quiet = eng.run(patches, patch_mode=True, ioconfig=cfg, return_attention="class")
    assert "probabilities" not in quiet and quiet["attention"].shape == (5, 2, 2, 2) and np.array_equal(quiet["predictions"], plain["predictions"])


def test_each_refusal_comes_with_its_message_and_leaves_nothing_behind(tmp_path):
    from tiatoolbox_amd.models.engine.deep_feature_extractor import DeepFeatureExtractor
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor

    vit = tiny_vit()
    eng = DeepFeatureExtractor(_backbone(vit), batch_size=2)
    patches, cfg = _patches(vit), _cfg(vit)
    with pytest.raises(ValueError, match=r"return_attention is None, \"class\" or \"rollout\".*got return_attention='mean'"):
        eng.run(patches, patch_mode=True, ioconfig=cfg, return_attention="mean")
    assert eng.return_attention is None
    with pytest.raises(ValueError, match="got compute_dtype='bfloat16x3', whose float32 graph has no attention-map kernel"):
        eng.run(patches, patch_mode=True, ioconfig=cfg, return_attention="class", compute_dtype="bfloat16x3")
    assert eng.return_attention is None
    eng.compute_dtype = "float32"
    with pytest.raises(ValueError, match="got patch_mode=False"):
        eng.run([tmp_path / "slide.npy"], patch_mode=False, ioconfig=cfg, save_dir=tmp_path / "out", return_attention="rollout")
    assert eng.return_attention is None
    cnn = PatchPredictor("resnet18-kather100k", batch_size=2)
    with pytest.raises(ValueError, match="got CNNModel, which has no VisionTransformer"):
        cnn.run(np.zeros((2, 64, 64, 3), np.uint8), patch_mode=True, return_attention="class", patch_input_shape=(64, 64))
    assert cnn.return_attention is None
    assert "attention" not in eng.run(patches, patch_mode=True, ioconfig=cfg)


NEW_WRAPPERS = ("hip_mha_probs_h", "hip_rollout_step_f32")


def _stand_in_maps(calls: dict) -> dict:
    from _vit_attention_ref import probs32

    def probs(qkv, heads, scale, *, q_rows, head_mean):
        calls["hip_mha_probs_h"] = calls.get("hip_mha_probs_h", 0) + 1
        return probs32(qkv, heads, scale, q_rows, head_mean=head_mean)

    def step(a, r_in):
        calls["hip_rollout_step_f32"] = calls.get("hip_rollout_step_f32", 0) + 1
        r = torch.eye(a.shape[-1]).expand_as(a) if r_in is None else r_in
        return 0.5 * (a @ r) + 0.5 * r

    return {"hip_mha_probs_h": probs, "hip_rollout_step_f32": step}


def test_the_graph_with_maps_off_calls_neither_new_wrapper_and_counts_its_launches_with_them(monkeypatch):
    """Maps off: both new wrappers are replaced by functions that fail and the graph still runs.  "class": one probability launch per
    forward; "rollout": two launches per block.  The stand-ins state the wrappers' contract in torch, so the wiring (which block,
    which rows, the prefix columns, the grid) is checked against the float64 restatement on any device."""
    from tiatoolbox_amd.models.architecture import vit_fused

    def fail(*_a, **_k):
        raise AssertionError("a map wrapper was called with return_attention=None")

    for name, fn in torch_vit_wrappers({}).items():
        monkeypatch.setattr(vit_fused, name, fn)
    for name in NEW_WRAPPERS:
        monkeypatch.setattr(vit_fused, name, fail)
    vit = tiny_virchow(TINY_V2)
    fused = vit_fused.FusedViT(vit)
    fused.prepare(torch.bfloat16)
    x = _images(vit, square=False)
    with torch.inference_mode():
        plain = fused(x)
    assert fused.attention_maps is None and fused.return_attention is None
    calls: dict = {}
    for name, fn in _stand_in_maps(calls).items():
        monkeypatch.setattr(vit_fused, name, fn)
    for kind, want in (("class", {"hip_mha_probs_h": 1}), ("rollout", {"hip_mha_probs_h": 2, "hip_rollout_step_f32": 2})):
        calls.clear()
        fused.return_attention = kind
        with torch.inference_mode():
            assert torch.equal(fused(x), plain)
        assert calls == want
        ref, _ = maps64_of(vit, x, kind)
        assert tuple(fused.attention_maps.shape) == tuple(ref.shape) and fused.attention_maps.dtype == torch.float32
        assert map_error(fused.attention_maps, ref) <= 0.05  # (bf16 weights and activations: only the wiring is looked at here)
    fused.return_attention = None
    with torch.inference_mode():
        fused(x)
    assert fused.attention_maps is None
    fused.return_attention = "mean"
    with pytest.raises(ValueError, match="return_attention is None, 'class' or 'rollout'"), torch.inference_mode():
        fused(x)


def test_library_lists_the_two_entry_points():
    import ctypes as C  # noqa: N812

    from tiatoolbox_amd import _lib

    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert _lib._SIGNATURES["tia_mha_probs_h"] == ([p, p, i64, i64, i64, i64, C.c_float, i64, i32, i32, p], C.c_int)  # noqa: SLF001
    assert _lib._SIGNATURES["tia_rollout_step_f32"] == ([p, p, p, i64, i64, p], C.c_int)  # noqa: SLF001


def _gloo_worker(rank: int, world: int, port: int, n: int, out_dir: str) -> None:
    from tiatoolbox_amd import distributed as tdist
    from tiatoolbox_amd.models.engine.deep_feature_extractor import DeepFeatureExtractor

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    tdist.init_from_env("gloo")
    vit = tiny_foundation(TINY_REG)
    out = DeepFeatureExtractor(_backbone(vit), batch_size=1).run(_patches(vit, n), patch_mode=True, ioconfig=_cfg(vit), return_attention="rollout")
    np.save(os.path.join(out_dir, f"a{rank}.npy"), out["attention"])
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize(("world", "n"), [(2, 5), (3, 2)])
def test_maps_are_gathered_across_ranks(tmp_path, world, n):
    """Five patches on two ranks (shards of 3 and 2), and two patches on three (the last rank's shard is EMPTY: it probes one patch
    for the row shape and contributes zero rows): every rank returns all the maps, equal to the single-process maps."""
    from tiatoolbox_amd.models.engine.deep_feature_extractor import DeepFeatureExtractor

    port = 29350 + (os.getpid() % 200) + 7 * world
    mp.spawn(_gloo_worker, args=(world, port, n, str(tmp_path)), nprocs=world, join=True)
    vit = tiny_foundation(TINY_REG)
    single = DeepFeatureExtractor(_backbone(vit), batch_size=1).run(_patches(vit, n), patch_mode=True, ioconfig=_cfg(vit),
                                                                    return_attention="rollout")["attention"]
    a0 = np.load(tmp_path / "a0.npy")
    assert a0.shape == (n, 2, 2) and all(np.array_equal(a0, np.load(tmp_path / f"a{r}.npy")) for r in range(1, world))
    assert np.array_equal(a0, single)  # (one patch per forward on either side: the same arithmetic)

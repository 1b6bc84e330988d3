"""``attention_head_fusion`` / ``attention_discard_ratio`` on the device: ``FusedViT`` and the engines.  The discard step is
discontinuous -- a last-bit difference between two softmax implementations moves ``v`` and flips entries -- so the maps are compared
by EQUALITY with the NumPy restatement applied to the fused matrices the device itself produced for each block; only max / min
without discarding are also held against the CPU module under the project's criterion."""

from __future__ import annotations

import copy

import numpy as np
import pytest
import torch
from _vit_ref import tiny_vit
from _vit_rollout_options_ref import discard_count, rollout

from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FUSIONS = ("mean", "max", "min")
NEW_KERNELS = ("kth_smallest_kernel", "discard_normalize_kernel", "rollout_step_kernel<false>", "rollout_step_kernelILb0E")


def _fused(vit, dtype: torch.dtype = BF16):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(copy.deepcopy(vit).cuda())
    fused.prepare(dtype)
    return fused.to(dtype)


def _device_input(x: torch.Tensor, dtype: torch.dtype = BF16) -> torch.Tensor:
    return x.cuda().to(dtype).contiguous(memory_format=torch.channels_last)


@pytest.fixture
def recorded(monkeypatch):
    """The fused matrices ``tia_mha_probs_fused_h`` wrote, in launch order (one per block of every forward)."""
    from tiatoolbox_amd.models.architecture import vit_fused

    seen: list[np.ndarray] = []
    real = vit_fused.hip_mha_probs_fused_h

    def recording(qkv, heads, scale, head_fusion):
        out = real(qkv, heads, scale, head_fusion)
        seen.append(out.cpu().numpy())
        return out

    monkeypatch.setattr(vit_fused, "hip_mha_probs_fused_h", recording)
    return seen


def test_graph_maps_equal_the_reference_on_the_device_s_own_matrices(recorded):
    """Tiny seeded model, depth 2, three 64 x 64 images (S = 17).  Per fusion and r in {0, 0.9}: the features are those of the run
    without maps; with the defaults the maps are today's rollout and none of the new kernels is launched; otherwise the map equals,
    bit for bit, the reference's rollout (selection, normalisation, one fma chain per element of the product) of the recorded
    matrices."""
    from test_vit_gpu import _device_kernels

    vit = tiny_vit()
    fused = _fused(vit)
    x = _device_input(torch.randn((3, 3, 64, 64), generator=torch.Generator().manual_seed(21)))
    s = 17
    with torch.inference_mode():
        plain = fused(x)
        fused.return_attention = "rollout"
        assert torch.equal(fused(x), plain)
        today = fused.attention_maps
        for fusion in FUSIONS:
            for r in (0.0, 0.9):
                recorded.clear()
                fused.attention_head_fusion, fused.attention_discard_ratio = fusion, r
                assert torch.equal(fused(x), plain), (fusion, r)
                maps = fused.attention_maps
                assert maps.dtype == torch.float32 and tuple(maps.shape) == (3, 4, 4)
                if fusion == "mean" and r == 0.0:
                    assert torch.equal(maps, today) and not recorded
                    kernels = _device_kernels(lambda: fused(x))
                    assert any("rollout_step_kernel" in k for k in kernels) and any("mha_probs_kernel" in k for k in kernels)
                    assert not [k for k in kernels if any(new in k for new in NEW_KERNELS)], kernels
                    continue
                assert len(recorded) == 2 and discard_count(r, s) == (260 if r else 0)
                ref = rollout(list(recorded), fusion, r)[:, 0, 1:].reshape(3, 4, 4)
                got = maps.cpu().numpy()
                assert np.array_equal(got, ref), (fusion, r, float(np.abs(got - ref).max()))
                assert not torch.equal(maps, today)
        fused.attention_head_fusion, fused.attention_discard_ratio = "max", 0.9
        kernels = _device_kernels(lambda: fused(x))
        for wanted in ("mha_probs_kernel", "kth_smallest_kernel", "discard_normalize_kernel", "rollout_step_kernel"):
            assert any(wanted in k for k in kernels), (wanted, kernels)
        fused.return_attention = None
        assert torch.equal(fused(x), plain) and fused.attention_maps is None


@pytest.mark.parametrize("fusion", ["max", "min"])
def test_max_and_min_without_discarding_match_the_cpu_module(fusion):
    """``r = 0`` is continuous in the probabilities, so the criterion of the rollout graph test applies: with the float32 CPU module's
    ``forward_with_attention`` as the reference, ``e = max |m - ref| / max ref`` of the hand-written graph is at most twice that of
    the torch module cast to bf16 on the same device (16 images on a 6 x 5 grid: some hundreds of entries under the maximum)."""
    vit = tiny_vit()
    x = torch.randn((16, 3, 96, 80), generator=torch.Generator().manual_seed(11))
    with torch.inference_mode():
        ref = vit.forward_with_attention(x, "rollout", fusion, 0.0)[1].double()
        lib = copy.deepcopy(vit).cuda().to(BF16).forward_with_attention(x.cuda().to(BF16), "rollout", fusion, 0.0)[1].cpu().double()
        fused = _fused(vit)
        fused.return_attention, fused.attention_head_fusion = "rollout", fusion
        fused(_device_input(x))
        new = fused.attention_maps.cpu().double()
    e_new, e_lib = float((new - ref).abs().max() / ref.max()), float((lib - ref).abs().max() / ref.max())
    print(f"fused maps {fusion} r=0: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
    assert tuple(new.shape) == (16, 6, 5) and e_new <= 2.0 * e_lib


def _engine(kind: str):
    from _vit_classifier_ref import timm_model

    from tiatoolbox_amd.models import DeepFeatureExtractor, PatchPredictor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    if kind == "classifier":
        model = timm_model(tiny_vit())
        model.preproc_func = timm_preproc_func("vit_small_patch16_224")
        return PatchPredictor(model, batch_size=6, device="cuda")
    with torch.device("meta"):
        model = TimmBackbone("vit_small_patch16_224")  # (the named trunk's shapes only: it is replaced)
    model.feat_extract = copy.deepcopy(tiny_vit())
    model.preproc_func = timm_preproc_func("vit_small_patch16_224")
    return DeepFeatureExtractor(model.eval(), batch_size=6, device="cuda")


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "mpp", "resolution": 0.5}], patch_input_shape=(64, 64), stride_shape=(32, 32))


def test_patch_predictor_patch_mode_with_both_options(recorded):
    """Ten uint8 patches in batches of 6 and 4 through ``PatchPredictor``: predictions and probabilities are those of the run without
    maps; the maps equal the reference's rollout of the matrices the device wrote; the next call has forgotten the options."""
    eng = _engine("classifier")
    patches = np.random.default_rng(6).integers(0, 256, (10, 64, 64, 3), dtype=np.uint8)
    kw = {"patch_mode": True, "ioconfig": _cfg(), "compute_dtype": "bfloat16", "return_probabilities": True}
    plain = eng.run(patches, **kw)
    today = eng.run(patches, return_attention="rollout", **kw)
    assert not recorded
    out = eng.run(patches, return_attention="rollout", attention_head_fusion="max", attention_discard_ratio=0.9, **kw)
    for key in plain:
        assert np.array_equal(out[key], plain[key]), key
    assert len(recorded) == 4 and [m.shape[0] for m in recorded] == [6, 6, 4, 4]
    ref = np.concatenate([rollout(recorded[0:2], "max", 0.9), rollout(recorded[2:4], "max", 0.9)])[:, 0, 1:].reshape(10, 4, 4)
    assert out["attention"].dtype == np.float32 and np.array_equal(out["attention"], ref)
    assert not np.array_equal(out["attention"], today["attention"])
    again = eng.run(patches, return_attention="rollout", **kw)
    assert np.array_equal(again["attention"], today["attention"]) and not hasattr(eng, "attention_head_fusion")
    with pytest.raises(ValueError, match="attention_discard_ratio=0.9"):
        eng.run(patches, return_attention="class", attention_discard_ratio=0.9, **kw)


def test_wsi_mode_merge_with_both_options(tmp_path):
    """A 208 x 152 slide, 64 x 64 patches at stride 32, ``merge_attention="rollout"`` with ("min", 0.5): ``attention`` in the file is
    bit for bit the patch-mode maps of the same options for the patches at ``coordinates``; ``merged_attention`` is the static merge
    of them; the features are those of the run without the kwargs."""
    from tiatoolbox_amd.models import PatchPredictor
    from tiatoolbox_amd.utils import synth
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    def load(path) -> dict:
        with np.load(path) as data:
            return {k: data[k] for k in data.files}

    cfg = _cfg()
    base = ArrayWSIReader(synth.g_he(1, 152, 208, seed=5)[0], mpp=0.5, power=20.0)
    eng = _engine("features")
    options = {"attention_head_fusion": "min", "attention_discard_ratio": 0.5}
    kw = {"patch_mode": False, "ioconfig": cfg, "compute_dtype": "bfloat16", "auto_get_mask": False, "return_probabilities": True}
    plain = load(eng.run([base], save_dir=tmp_path / "plain", **kw)[0])
    today = load(eng.run([base], save_dir=tmp_path / "today", merge_attention="rollout", merge_resolution=5.0, merge_units="power", **kw)[0])
    out = load(eng.run([base], save_dir=tmp_path / "opts", merge_attention="rollout", merge_resolution=5.0, merge_units="power", **options, **kw)[0])
    assert sorted(out) == sorted(today) == sorted([*plain, "attention", "attention_coverage", "merged_attention"])
    for key in plain:
        assert np.array_equal(out[key], plain[key]), key
    coords = out["coordinates"]
    patches = eng._reader_at_input_resolution(base).read_bounds_batch(coords).cpu().numpy()  # noqa: SLF001
    per_patch = eng.run(patches, patch_mode=True, ioconfig=cfg, compute_dtype="bfloat16", return_attention="rollout", **options)["attention"]
    assert per_patch.shape == (len(coords), 4, 4) and np.array_equal(out["attention"], per_patch)
    assert not np.array_equal(out["attention"], today["attention"])
    told = out | {"resolution": 0.5, "units": "mpp"}
    assert np.array_equal(PatchPredictor.merge_attention(base, told, resolution=5.0), out["merged_attention"])
    assert np.array_equal(out["attention_coverage"], today["attention_coverage"])
    assert not np.array_equal(out["merged_attention"], today["merged_attention"])
    with pytest.raises(ValueError, match="attention_head_fusion='min'"):
        eng.run([base], save_dir=tmp_path / "bad", merge_attention="class", **options, **kw)
    assert sorted(load(eng.run([base], save_dir=tmp_path / "after", **kw)[0])) == sorted(plain)

"""``attention_head_fusion`` / ``attention_discard_ratio`` on the host: the rule on a hand-computed 3 x 3 matrix, the plain-torch route
(``VisionTransformer.forward_with_attention``) against the independent restatement in ``_vit_rollout_options_ref``, the defaults,
every refusal at the model and at both engines, the declarations of the new entry points."""

from __future__ import annotations

import numpy as np
import pytest
import torch
from _vit_ref import tiny_vit
from _vit_rollout_options_ref import a_hat, discard, discard_count, fma_matmul, fuse, normalise, rollout, row_sums, threshold

from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

F32 = np.float32
FUSIONS = ("mean", "max", "min")
RATIOS = (0.0, 0.5, 0.9)


def test_discard_count_known_answers():
    """``k = min(int(r S^2), S^2 - 1)``: ``r S^2 < 1`` gives 0, ``r`` just below 1 is clamped; 0.9 x 17^2 = 260.1 and 0.9 x 197^2."""
    assert discard_count(0.0, 3) == 0 and discard_count(0.1, 3) == 0 and discard_count(0.112, 3) == 1
    assert discard_count(0.5, 3) == 4 and discard_count(0.9, 3) == 8 and discard_count(0.999999, 3) == 8
    assert discard_count(np.nextafter(1.0, 0.0), 3) == 8 and discard_count(np.nextafter(1.0, 0.0), 1) == 0
    assert discard_count(0.9, 17) == 260 and discard_count(0.9, 197) == 34928 and discard_count(0.5, 1) == 0
    from tiatoolbox_amd.models.engine import _rollout_options as ro

    for r in (0.0, 0.1, 0.5, 0.9, 0.999, float(np.nextafter(1.0, 0.0))):
        for s in (1, 2, 3, 17, 197, 261):
            assert ro.discard_count(r, s) == discard_count(r, s)


HAND = np.array([[[0.125, 0.5, 0.375],
                  [0.25, 0.25, 0.5],
                  [0.125, 0.75, 0.125]]], F32)  # sorted: .125 .125 .125 .25 .25 .375 .5 .5 .75


def test_hand_computed_three_by_three():
    """``k = 2``: ``v = 0.125`` with a three-way tie -- all three tied entries are named, and (0, 0) stays; (2, 0) and (2, 2) go.
    ``k = 4``: ``v = 0.25``, five entries ``<= v``, four go.  Every number below is a dyadic rational: the arithmetic is exact."""
    assert threshold(HAND, 2)[0] == F32(0.125) and threshold(HAND, 3)[0] == F32(0.125) and threshold(HAND, 4)[0] == F32(0.25)
    assert threshold(HAND, 8)[0] == F32(0.5) and threshold(HAND, 1)[0] == F32(0.125)
    kept = discard(HAND, 2)
    assert kept.tolist() == [[[0.125, 0.5, 0.375], [0.25, 0.25, 0.5], [0.0, 0.75, 0.0]]]
    assert discard(HAND, 1).tolist() == kept.tolist() == discard(HAND, 3).tolist()  # the tie goes as a whole
    assert discard(HAND, 4).tolist() == [[[0.125, 0.5, 0.375], [0.0, 0.0, 0.5], [0.0, 0.75, 0.0]]]
    assert discard(HAND, 8).tolist() == [[[0.125, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.75, 0.0]]]
    assert discard(HAND, 0).tolist() == HAND.tolist()
    assert discard(HAND, 2, strict=True).tolist() == HAND.tolist()  # the wrong rule keeps the ties: the two differ
    # k = 2:  (F' + I) / 2 = [[.5625 .25 .1875] [.125 .625 .25] [0 .375 .5]],  row sums 1, 1, .875
    got = a_hat(HAND, 2)
    assert row_sums(((kept + np.eye(3, dtype=F32)) * F32(0.5)).astype(F32)).tolist() == [[1.0, 1.0, 0.875]]
    want = np.array([[[0.5625, 0.25, 0.1875], [0.125, 0.625, 0.25], [0.0, F32(0.375) / F32(0.875), F32(0.5) / F32(0.875)]]], F32)
    assert np.array_equal(got, want)
    # the package's statement on the same matrix
    from tiatoolbox_amd.models.engine import _rollout_options as ro

    for k in (0, 1, 2, 4, 8):
        assert np.array_equal(ro.normalise(ro.discard(HAND, k)), a_hat(HAND, k)), k
    two = np.concatenate([a_hat(HAND, 2), a_hat(HAND, 4)])
    assert np.array_equal(ro.fma_matmul(two, two[::-1].copy()), fma_matmul(two, two[::-1].copy()))


def test_both_statements_agree_on_random_matrices():
    """The package's NumPy statement against this suite's restatement, bit for bit: fusion, selection, row sums over more than one
    64-entry chunk, and the fma chain (two-sum with rounding to odd against exact rational arithmetic)."""
    from tiatoolbox_amd.models.engine import _rollout_options as ro

    rng = np.random.default_rng(5)
    for s in (1, 5, 17, 70, 131):
        x = rng.standard_normal((2, 3, s, s)) * 2.0
        p = np.exp(x - x.max(-1, keepdims=True))
        p = (p / p.sum(-1, keepdims=True)).astype(F32)
        for fusion in FUSIONS:
            f = fuse(p, fusion)
            assert np.array_equal(ro.fuse_heads(p, fusion), f)
            assert np.array_equal(ro.row_sums(f), row_sums(f))
            for r in (0.5, 0.9, 0.999):
                k = discard_count(r, s)
                if k:
                    assert np.array_equal(ro.kth_smallest(f, k), threshold(f, k))
                assert np.array_equal(ro.normalise(ro.discard(f, k)), a_hat(f, k))
    a, b = a_hat(fuse(p[:, :, :9, :9], "max"), 40), a_hat(fuse(p[:, :, :9, :9], "min"), 40)
    assert np.array_equal(ro.fma_matmul(a, b), fma_matmul(a, b))
    tiny = (a * F32(2.0 ** -100)).astype(F32), (b * F32(2.0 ** -40)).astype(F32)  # products in the subnormal range
    assert np.array_equal(ro.fma_matmul(*tiny), fma_matmul(*tiny))


def _images(side: int, n: int = 2) -> torch.Tensor:
    return torch.randn((n, 3, side, side), generator=torch.Generator().manual_seed(side))


@pytest.mark.parametrize("side", [32, 64])
def test_torch_route_matches_the_reference(side):
    """The seeded tiny model (depth 2, two heads) at 32^2 (S = 5) and 64^2 (S = 17), mean / max / min x r in {0, 0.5, 0.9}.

    From the torch route's own fused matrices the reference's ``A^`` equals the route's bit for bit (selection, the (0, 0) rule, the
    row-sum order).  The map then differs by the summation order of the products alone: a float32 dot product of ``S``
    non-negative terms is within ``S 2^-23`` of its value in any order, once per block after the first, so with the depth 2 of this
    model ``|map - ref| <= (2 - 1) S 2^-23 max|map|`` = 17 x 2^-23 = 2.0e-6 of the largest entry at 64^2 (5 x 2^-23 = 6.0e-7 at 32^2)."""
    vit = tiny_vit()
    x = _images(side)
    s = (side // 16) ** 2 + 1
    with torch.inference_mode():
        plain = vit(x)
        for fusion in FUSIONS:
            for r in RATIOS:
                trace: dict = {}
                feats, maps = vit.forward_with_attention(x, "rollout", fusion, r, trace=trace)
                assert torch.equal(feats, plain) and maps.dtype == torch.float32 and tuple(maps.shape) == (2, side // 16, side // 16)
                k = discard_count(r, s)
                if fusion == "mean" and k == 0:
                    assert not trace and torch.equal(maps, vit.forward_with_attention(x, "rollout")[1])
                    continue
                assert len(trace["fused"]) == len(trace["normalised"]) == 2
                fused = [f.numpy() for f in trace["fused"]]
                for f, a in zip(fused, trace["normalised"]):
                    assert np.array_equal(a_hat(f, k), a.numpy()), (fusion, r)
                    if k:
                        zeros = int((a.numpy() == 0).sum(axis=(1, 2)).min())
                        assert zeros >= k - s  # the k smallest are gone, but for (0, 0) and the diagonal (halves of 1 are added there)
                ref = rollout(fused, fusion, r)[:, 0, 1:].reshape(maps.shape)
                bound = (2 - 1) * s * 2.0 ** -23 * float(np.abs(ref).max())
                err = float(np.abs(maps.numpy().astype(np.float64) - ref).max())
                print(f"torch route side={side} {fusion} r={r}: max |map - ref| {err:.3e}, bound {bound:.3e}")
                assert err <= bound


def test_fused_matrices_of_the_torch_route_are_the_heads_mean_max_min():
    """``trace["fused"]`` is the fusion of the per-head probabilities the default route averages: recomputed here from the qkv output."""
    vit = tiny_vit()
    x = _images(64)
    seen = []
    handle = vit.blocks[0].attn.qkv.register_forward_hook(lambda _m, _i, out: seen.append(out))
    with torch.inference_mode():
        traces = {}
        for fusion in FUSIONS:
            traces[fusion] = {}
            vit.forward_with_attention(x, "rollout", fusion, 0.5, trace=traces[fusion])
    handle.remove()
    qkv = seen[0]
    b, s, _ = qkv.shape
    q, k, _ = qkv.reshape(b, s, 3, 2, 64).permute(2, 0, 3, 1, 4).unbind(0)
    p = ((q * 64 ** -0.5) @ k.transpose(-2, -1)).softmax(-1).numpy()
    for fusion in FUSIONS:
        assert np.array_equal(traces[fusion]["fused"][0].numpy(), fuse(p, fusion)), fusion
    assert not np.array_equal(traces["max"]["fused"][0].numpy(), traces["min"]["fused"][0].numpy())


def test_defaults_are_the_call_without_the_arguments():
    vit = tiny_vit()
    x = _images(64)
    with torch.inference_mode():
        for kind in ("class", "rollout"):
            feats, maps = vit.forward_with_attention(x, kind)
            again = vit.forward_with_attention(x, kind, "mean", 0.0)
            named = vit.forward_with_attention(x, kind, head_fusion="mean", discard_ratio=0)
            assert torch.equal(again[0], feats) and torch.equal(again[1], maps) and torch.equal(named[1], maps)
            assert torch.equal(feats, vit(x))
        small = vit.forward_with_attention(x, "rollout", "mean", 1.0 / 290.0)  # r S^2 < 1: k = 0, the same path
        assert torch.equal(small[1], vit.forward_with_attention(x, "rollout")[1])
        with vit.capturing_attention("rollout", "max", 0.9) as maps:
            feats = vit(x)
        assert torch.equal(feats, vit(x)) and torch.equal(maps[0], vit.forward_with_attention(x, "rollout", "max", 0.9)[1])
        assert not torch.equal(maps[0], vit.forward_with_attention(x, "rollout")[1])


BAD_RATIOS = (1.0, -0.1, 1.5, float("nan"), "0.5", None, True)


def test_model_refusals_name_the_option():
    vit = tiny_vit()
    x = _images(32)
    with pytest.raises(ValueError, match="attention_head_fusion is one of"):
        vit.forward_with_attention(x, "rollout", "sum")
    for bad in BAD_RATIOS:
        with pytest.raises(ValueError, match="attention_discard_ratio is a real number"):
            vit.forward_with_attention(x, "rollout", "mean", bad)
    with pytest.raises(ValueError, match=r"attention_head_fusion='max'.*rollout"):
        vit.forward_with_attention(x, "class", "max")
    with pytest.raises(ValueError, match=r"attention_discard_ratio=0.5.*rollout"):
        vit.forward_with_attention(x, "class", "mean", 0.5)
    assert len(vit.blocks[0].attn.qkv._forward_hooks) == 0  # noqa: SLF001


def _backbone(vit):
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    with torch.device("meta"):
        model = TimmBackbone("vit_small_patch16_224")  # (the named trunk's shapes only: it is replaced)
    model.feat_extract = vit
    model.preproc_func = timm_preproc_func("vit_small_patch16_224")
    return model.eval()


def _engines():
    from _vit_classifier_ref import timm_model

    from tiatoolbox_amd.models import DeepFeatureExtractor, PatchPredictor

    model = timm_model(tiny_vit())
    model.preproc_func = timm_preproc_func("vit_small_patch16_224")
    return {"features": DeepFeatureExtractor(_backbone(tiny_vit()), batch_size=2), "classifier": PatchPredictor(model, batch_size=2)}


def _cfg(side: int = 32):
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(side, side),
                                  stride_shape=(side, side))


@pytest.mark.parametrize("which", ["features", "classifier"])
def test_engine_refusals_name_the_option_and_leave_nothing_behind(which, tmp_path):
    eng = _engines()[which]
    patches = np.random.default_rng(3).integers(0, 256, (3, 32, 32, 3), dtype=np.uint8)
    kw = {"patch_mode": True, "ioconfig": _cfg()}
    plain = eng.run(patches, **kw)
    cases = [
        ({"attention_head_fusion": "max"}, "attention_head_fusion='max'"),                                   # no maps asked for
        ({"attention_discard_ratio": 0.9}, "attention_discard_ratio=0.9"),
        ({"attention_head_fusion": "min", "return_attention": "class"}, "attention_head_fusion='min'"),      # beside "class"
        ({"attention_discard_ratio": 0.5, "return_attention": "class"}, "attention_discard_ratio=0.5"),
        ({"attention_head_fusion": "sum", "return_attention": "rollout"}, "attention_head_fusion is one of"),
        *[({"attention_discard_ratio": bad, "return_attention": "rollout"}, "attention_discard_ratio is a real number") for bad in BAD_RATIOS],
    ]
    for extra, message in cases:
        with pytest.raises(ValueError, match=message):
            eng.run(patches, **kw, **extra)
        assert not hasattr(eng, "attention_head_fusion") and not hasattr(eng, "attention_discard_ratio")
    wsi = {"patch_mode": False, "ioconfig": _cfg(), "save_dir": tmp_path / "out"}
    with pytest.raises(ValueError, match="attention_head_fusion='max'"):
        eng.run([tmp_path / "slide.npy"], **wsi, attention_head_fusion="max")
    with pytest.raises(ValueError, match="attention_discard_ratio=0.9"):
        eng.run([tmp_path / "slide.npy"], **wsi, merge_attention="class", attention_discard_ratio=0.9)
    after = eng.run(patches, **kw)
    assert sorted(after) == sorted(plain) and "attention" not in after


@pytest.mark.parametrize("which", ["features", "classifier"])
def test_engine_runs_the_options_per_call(which):
    """Patch mode on the plain-torch route: the maps are those of ``forward_with_attention`` with the same options, everything else is
    that of the run without them, the defaults are today's rollout, and the next call has forgotten the options."""
    eng = _engines()[which]
    patches = np.random.default_rng(4).integers(0, 256, (5, 32, 32, 3), dtype=np.uint8)
    kw = {"patch_mode": True, "ioconfig": _cfg(), "return_probabilities": True}
    plain = eng.run(patches, **kw)
    today = eng.run(patches, return_attention="rollout", **kw)
    same = eng.run(patches, return_attention="rollout", attention_head_fusion="mean", attention_discard_ratio=0.0, **kw)
    assert np.array_equal(same["attention"], today["attention"])
    out = eng.run(patches, return_attention="rollout", attention_head_fusion="max", attention_discard_ratio=0.9, **kw)
    for key in plain:
        assert np.array_equal(out[key], plain[key]), key
    model = eng.model
    x = model.preproc_func.device_batch(torch.from_numpy(patches), torch.float32).permute(0, 3, 1, 2).contiguous()
    with torch.inference_mode():
        want = torch.cat([model.feat_extract.forward_with_attention(x[i:i + 2], "rollout", "max", 0.9)[1] for i in (0, 2, 4)])
    assert out["attention"].dtype == np.float32 and np.array_equal(out["attention"], want.numpy())
    assert not np.array_equal(out["attention"], today["attention"])
    assert np.array_equal(eng.run(patches, return_attention="rollout", **kw)["attention"], today["attention"])
    assert not hasattr(eng, "attention_head_fusion") and not hasattr(eng, "attention_discard_ratio")


def test_fused_graph_takes_the_new_wrappers_only_when_asked(monkeypatch):
    """The wiring of ``FusedViT`` on any device, the wrappers replaced by their contracts in torch / NumPy: the defaults (and
    ``r S^2 < 1`` with the mean) call today's two wrappers and none of the new three; another fusion or ``k >= 1`` calls the fused
    probabilities and the discard step once per block and the product once per block after the first."""
    from _vit_attention_ref import probs32
    from _vit_classifier_ref import torch_vit_wrappers

    from tiatoolbox_amd.models.architecture import vit_fused

    calls: dict = {}

    def count(name):
        calls[name] = calls.get(name, 0) + 1

    def probs(qkv, heads, scale, *, q_rows, head_mean):
        count("hip_mha_probs_h")
        return probs32(qkv, heads, scale, q_rows, head_mean=head_mean)

    def step(a, r_in):
        count("hip_rollout_step_f32")
        r = torch.eye(a.shape[-1]).expand_as(a) if r_in is None else r_in
        return 0.5 * (a @ r) + 0.5 * r

    def probs_fused(qkv, heads, scale, head_fusion):
        count("hip_mha_probs_fused_h")
        return torch.from_numpy(fuse(probs32(qkv, heads, scale).numpy(), head_fusion))

    def discard_normalize(f, k):
        count("hip_rollout_discard_normalize_f32")
        return torch.from_numpy(a_hat(f.numpy(), k))

    def product(a, r_in):
        count("hip_rollout_product_f32")
        return a @ r_in

    for name, fn in torch_vit_wrappers({}).items():
        monkeypatch.setattr(vit_fused, name, fn)
    for name, fn in {"hip_mha_probs_h": probs, "hip_rollout_step_f32": step, "hip_mha_probs_fused_h": probs_fused,
                     "hip_rollout_discard_normalize_f32": discard_normalize, "hip_rollout_product_f32": product}.items():
        monkeypatch.setattr(vit_fused, name, fn)
    vit = tiny_vit()
    fused = vit_fused.FusedViT(vit)
    fused.prepare(torch.bfloat16)
    x = _images(64)
    today = {"hip_mha_probs_h": 2, "hip_rollout_step_f32": 2}
    other = {"hip_mha_probs_fused_h": 2, "hip_rollout_discard_normalize_f32": 2, "hip_rollout_product_f32": 1}
    fused.return_attention = "rollout"
    with torch.inference_mode():
        plain = fused(x)
        base = fused.attention_maps
        assert calls == today
        for fusion, r, want in (("mean", 0.0, today), ("mean", 1.0 / 290.0, today), ("mean", 0.5, other), ("max", 0.0, other),
                                ("min", 0.9, other)):
            calls.clear()
            fused.attention_head_fusion, fused.attention_discard_ratio = fusion, r
            assert torch.equal(fused(x), plain) and calls == want, (fusion, r, calls)
            assert tuple(fused.attention_maps.shape) == (2, 4, 4) and torch.equal(fused.attention_maps, base) == (want is today)
        fused.attention_head_fusion = "sum"
        with pytest.raises(ValueError, match="attention_head_fusion is one of"):
            fused(x)


def test_library_lists_the_three_entry_points():
    import ctypes as C  # noqa: N812
    import re
    from pathlib import Path

    from tiatoolbox_amd import _lib

    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    sig = _lib._SIGNATURES  # noqa: SLF001
    assert sig["tia_mha_probs_fused_h"] == ([p, p, i64, i64, i64, i64, C.c_float, i32, i32, p], C.c_int)
    assert sig["tia_rollout_discard_normalize_f32"] == ([p, p, p, i64, i64, i64, p], C.c_int)
    assert sig["tia_rollout_product_f32"] == ([p, p, p, i64, i64, p], C.c_int)
    header = (Path(__file__).resolve().parent.parent / "include" / "tiatoolbox_amd.h").read_text()
    for name, args in (("tia_mha_probs_fused_h", 10), ("tia_rollout_discard_normalize_f32", 7), ("tia_rollout_product_f32", 6)):
        found = re.search(rf"^int {name}\(([^;]*)\);", header, flags=re.M | re.S)
        assert found and len(found.group(1).split(",")) == args == len(sig[name][0]), name
    assert "#define TIA_ABI_VERSION 6" in header
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define TIA_FUSE_(\w+) (\d)", header)}
    from tiatoolbox_amd.models.engine._rollout_options import FUSION_CODES

    assert codes == {k.upper(): v for k, v in FUSION_CODES.items()}

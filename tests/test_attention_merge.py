"""``merge_attention`` on the host: the package's NumPy loop (the specification of ``tia_merge_patch_grids_f32``) against the
independent restatement in ``_attention_merge_ref``, bit for bit; coverage against ``merge_patch_rects``; exactness properties; the
float32 arithmetic against a float64 evaluation of the same formulas; the static method and every refusal."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _attention_merge_ref as ref  # noqa: E402

MODES = ("nearest", "bilinear")
ALL = ("sum", "count", "raw")


class _Slide:
    """What ``merge_attention`` reads of a slide reader (an ``ArrayWSIReader`` itself lives on the device)."""

    def __init__(self, width: int, height: int, mpp: float = 0.5, power: float = 20.0) -> None:
        self.slide_dimensions, self.mpp, self.power = (width, height), mpp, power


def _geometry(case):
    ws, hs, _, _, _, gh, gw, w, h = case
    return (ws, hs), (h, w), (gh, gw)


def _host(coords, maps, space, canvas, mode, want=ALL, **kw):
    from tiatoolbox_amd.models.engine import _attention_merge as am

    return am.merge_patch_grids(coords, maps, space, canvas, interpolation=mode, want=want, device="cpu", **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_host_loop_equals_the_restatement(case, c, mode):
    space, canvas, _ = _geometry(case)
    coords, maps = ref.case_inputs(case, c)
    if ref.overlapping(case):  # the equality tests the ORDER only if the order matters: shown on the restatement alone
        share = ref.order_matters(coords, maps, space, canvas, mode)
        print(f"order matters on {100 * share:.1f} % of the covered pixels ({mode}, C = {c})")
        assert share >= 0.02  # noqa: PLR2004
    exp = ref.merge(coords, maps, space, canvas, mode)
    out = _host(coords, maps, space, canvas, mode)
    for key in ALL:
        assert out[key].dtype == exp[key].dtype and out[key].shape == exp[key].shape, key
        assert np.array_equal(out[key], exp[key]), (key, int((out[key] != exp[key]).sum()))
    assert exp["count"].max() >= (4 if ref.overlapping(case) else 1)


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_count_is_the_coverage_of_merge_patch_rects(case):
    from tiatoolbox_amd.models.engine import _patch_merge as pm

    space, canvas, _ = _geometry(case)
    coords, maps = ref.case_inputs(case, 1)
    rects = pm.patch_rects(coords, space, canvas)
    cover = pm.merge_patch_rects(rects, np.ones((len(rects), 1), np.float32), canvas, want=("count",), device="cpu")["count"]
    got = _host(coords, maps, space, canvas, "bilinear", want=("count",))["count"]
    assert got.dtype == cover.dtype == np.int32 and np.array_equal(got, cover)


def test_one_patch_integer_ratio_nearest_is_exact():
    """One 60 x 40 patch with a grid of 5 x 3 cells (20 x 8 slide pixels each) on a canvas at 1/4: a cell is 5 x 2 canvas pixels, and
    every pixel equals its cell's value exactly."""
    maps = ref.random_maps(1, 2, 5, 3, seed=5)
    out = _host(np.array([[0, 0, 60, 40]]), maps, (60, 40), (10, 15), "nearest", want=("sum", "raw", "count"))
    expect = np.repeat(np.repeat(maps[0], 2, axis=1), 5, axis=2)
    assert np.array_equal(out["sum"], expect) and (out["count"] == 1).all()
    # up-sampling by 3 as well
    out = _host(np.array([[0, 0, 60, 40]]), maps, (60, 40), (120, 180), "nearest", want=("sum",))
    assert np.array_equal(out["sum"], np.repeat(np.repeat(maps[0], 24, axis=1), 60, axis=2))


@pytest.mark.parametrize("mode", MODES)
def test_constant_maps_give_the_constant(mode):
    """Every lerp of equal values returns the value exactly (``v + w * 0``); the sum of ``k`` copies and the divisor ``k + 1e-8`` round:
    ``raw`` is the constant within a few ulps."""
    case = ref.CASES[4]
    space, canvas, (gh, gw) = _geometry(case)
    coords = ref.grid_coordinates(case)
    value = np.float32(0.3137)
    out = _host(coords, np.full((len(coords), 2, gh, gw), value, np.float32), space, canvas, mode, want=("raw", "count", "sum"))
    covered = out["count"] > 0
    assert covered.any() and out["count"].max() >= 4  # noqa: PLR2004
    # sum of k equal float32 values: at most k - 1 roundings, each <= u relative; the quotient adds 1e-8 / k and one rounding
    k = out["count"].max()
    assert np.abs(out["raw"][:, covered] - value).max() <= (k + 1) * ref.U * value
    assert not out["raw"][:, ~covered].any()


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_bilinear_against_float64(case):
    """Per patch: the float32 samples against the float64 evaluation of the same formulas (the four per-patch numbers unrounded),
    ``|v - v64| <= (3 (gw + 1) + 3 (gh + 1) + 6) u max(map_i)``.  Measured (in u max(map_i)): 17.6 at 16 x 16, 8.2 at 6 x 5, under 5 on the smaller grids."""
    space, canvas, (gh, gw) = _geometry(case)
    coords, maps = ref.case_inputs(case, 3)
    worst = 0.0
    for i in range(len(coords)):
        r = ref.rect_of(coords[i], *space, canvas[1], canvas[0])
        if r[2] <= r[0] or r[3] <= r[1]:
            continue
        got = _host(coords[i:i + 1], maps[i:i + 1], space, canvas, "bilinear", want=("sum",))["sum"][:, r[1]:r[3], r[0]:r[2]]
        v64 = ref.patch_samples(coords[i], r, maps[i], space, canvas, "bilinear", np.float64)
        err = float(np.abs(got.astype(np.float64) - v64).max())
        top = float(maps[i].max())
        worst = max(worst, err / (ref.U * top))
        assert err <= ref.bilinear_bound(gh, gw, top), (i, err / (ref.U * top))
    print(f"bilinear float32 against float64, grid {gh} x {gw}: at most {worst:.1f} u max(map); bound {3 * (gw + 1) + 3 * (gh + 1) + 6} u")
    assert worst > 0


@pytest.mark.parametrize("case", ref.CASES, ids=ref.CASE_IDS)
def test_nearest_against_float64(case):
    """Per patch, the cell every pixel takes (read off a grid that holds its own cell numbers) against the float64 coordinate's cell,
    wherever that coordinate is further than 1e-4 from a cell boundary in both axes.  That leaves out nothing on the first five
    cases and at most 2 % of the (patch, row) and (patch, column) coordinates on the sixth (measured: 10 of 1386)."""
    space, canvas, (gh, gw) = _geometry(case)
    coords = ref.grid_coordinates(case)
    cells = np.arange(gh * gw, dtype=np.float32).reshape(1, 1, gh, gw)
    total = left_out = 0
    for i in range(len(coords)):
        r = ref.rect_of(coords[i], *space, canvas[1], canvas[0])
        if r[2] <= r[0] or r[3] <= r[1]:
            continue
        got = _host(coords[i:i + 1], cells, space, canvas, "nearest", want=("sum",))["sum"][0, r[1]:r[3], r[0]:r[2]]
        gy, gx = ref.grid_coordinates_of_pixels(coords[i], r, space, canvas, (gh, gw), np.float64)
        clear_y, clear_x = (np.abs(g + 0.5 - np.rint(g + 0.5)) > 1e-4 for g in (gy, gx))  # noqa: PLR2004
        total += gy.shape[0] + gx.shape[1]
        left_out += int((~clear_y[:, 0]).sum() + (~clear_x[0, :]).sum())
        expect = np.minimum(np.floor(gy + 0.5), gh - 1) * gw + np.minimum(np.floor(gx + 0.5), gw - 1)
        keep = clear_y & clear_x
        assert np.array_equal(got[keep], expect[keep].astype(np.float32)), i
    print(f"nearest against float64: {left_out} of {total} coordinates within 1e-4 of a cell boundary")
    assert left_out <= (0.02 * total if case is ref.CASES[5] else 0)


def test_three_dimensional_maps_are_one_channel():
    case = ref.CASES[2]
    space, canvas, _ = _geometry(case)
    coords, maps = ref.case_inputs(case, 1)
    four, three = _host(coords, maps, space, canvas, "bilinear"), _host(coords, maps[:, 0], space, canvas, "bilinear")
    assert three["raw"].shape == canvas and three["sum"].shape == canvas and three["count"].shape == canvas
    assert np.array_equal(three["raw"], four["raw"][0]) and np.array_equal(three["sum"], four["sum"][0])
    only = _host(coords, maps, space, canvas, "bilinear", want=("raw",))
    assert list(only) == ["raw"]


def test_tensors_in_tensors_out_on_the_host():
    import torch

    case = ref.CASES[0]
    space, canvas, _ = _geometry(case)
    coords, maps = ref.case_inputs(case, 3)
    out = _host(torch.from_numpy(coords), torch.from_numpy(maps), space, canvas, "bilinear")
    exp = ref.merge(coords, maps, space, canvas, "bilinear")
    for key in ALL:
        assert isinstance(out[key], torch.Tensor) and np.array_equal(out[key].numpy(), exp[key]), key


def test_refusals_of_the_host_function():
    from tiatoolbox_amd.models.engine import _attention_merge as am

    coords, maps = np.array([[0, 0, 8, 8]]), np.ones((1, 1, 2, 2), np.float32)
    with pytest.raises(ValueError, match="want"):
        am.merge_patch_grids(coords, maps, (8, 8), (4, 4), want=("labels",))
    with pytest.raises(ValueError, match="want"):
        am.merge_patch_grids(coords, maps, (8, 8), (4, 4), want=())
    with pytest.raises(ValueError, match="interpolation"):
        am.merge_patch_grids(coords, maps, (8, 8), (4, 4), interpolation="bicubic")
    with pytest.raises(ValueError, match="empty canvas"):
        am.merge_patch_grids(coords, maps, (8, 8), (0, 4))
    with pytest.raises(ValueError, match="must agree"):
        am.merge_patch_grids(coords, maps[0, 0], (8, 8), (4, 4))
    with pytest.raises(ValueError, match="must agree"):
        am.merge_patch_grids(np.zeros((2, 4)), maps, (8, 8), (4, 4))
    with pytest.raises(ValueError, match="coarser `resolution`"):
        am.merge_patch_grids(coords, maps, (8, 8), (1 << 16, 1 << 15), device="cpu")
    wide = np.broadcast_to(np.float32(1.0), (1, 1, 1, (1 << 24) + 1))  # (a view without memory: refused before anything is copied)
    with pytest.raises(ValueError, match="2\\^24"):
        am.merge_patch_grids(coords, wide, (8, 8), (4, 4), device="cpu")


def test_static_method_on_a_dict_and_on_a_file(tmp_path):
    from tiatoolbox_amd.models import DeepFeatureExtractor, PatchPredictor

    case = ref.CASES[2]  # its patches on a 300 x 210 slide at 20x, read at 20x
    (ws, hs), _, _ = _geometry(case)
    reader = _Slide(ws, hs)
    coords, maps = ref.case_inputs(case, 3)
    resolution = 4.0  # power: ratio 5 -> np.round((300, 210) / 5) = (60, 42)
    h, w = 42, 60
    output = {"coordinates": coords, "attention": maps, "resolution": 20.0, "units": "power"}
    for mode in MODES:
        exp = ref.merge(coords, maps, (ws, hs), (h, w), mode)
        got = PatchPredictor.merge_attention(reader, output, resolution=resolution, units="power", interpolation=mode)
        assert got.dtype == np.float32 and got.shape == (3, h, w) and np.array_equal(got, exp["raw"])
    got, cover = DeepFeatureExtractor.merge_attention(reader, output, resolution=resolution, return_count=True)  # inherited
    assert np.array_equal(got, exp["raw"]) and cover.dtype == np.int32 and np.array_equal(cover, exp["count"])
    # a rollout-shaped [N, gh, gw] array through an .npz, the slide given as an array
    path = tmp_path / "slide.npz"
    np.savez(path, coordinates=coords, attention=maps[:, 1], resolution=1.0, units="baseline")
    got = PatchPredictor.merge_attention(reader, path, resolution=resolution)
    assert got.shape == (h, w) and np.array_equal(got, exp["raw"][1])
    # the default resolution: 1.25x, ratio 16 -> (19, 13)
    got = PatchPredictor.merge_attention(reader, str(path))
    assert got.shape == (13, 19) and np.array_equal(got, ref.merge(coords, maps[:, 1:2], (ws, hs), (13, 19))["raw"][0])

    with pytest.raises(ValueError, match="resolution"):
        PatchPredictor.merge_attention(reader, {"coordinates": coords, "attention": maps})
    with pytest.raises(ValueError, match="units"):
        PatchPredictor.merge_attention(reader, {"coordinates": coords, "attention": maps, "resolution": 20.0})
    with pytest.raises(ValueError, match="'attention'"):
        PatchPredictor.merge_attention(reader, {"coordinates": coords, "probabilities": maps, "resolution": 20.0, "units": "power"})
    with pytest.raises(ValueError, match="'coordinates'"):
        PatchPredictor.merge_attention(reader, {"attention": maps, "resolution": 20.0, "units": "power"})
    with pytest.raises(ValueError, match="interpolation"):
        PatchPredictor.merge_attention(reader, output, interpolation="cubic")
    with pytest.raises(ValueError, match="must agree"):
        PatchPredictor.merge_attention(reader, output | {"attention": maps[:-1]})


def _vit_engine(cls):
    import copy

    import torch
    from _vit_ref import tiny_vit

    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    with torch.device("meta"):
        model = TimmBackbone("vit_small_patch16_224")  # (the named trunk's shapes only: it is replaced)
    model.feat_extract = copy.deepcopy(tiny_vit())
    model.preproc_func = timm_preproc_func("vit_small_patch16_224")
    return cls(model.eval(), batch_size=4, device="cpu")


def test_run_kwarg_refusals(tmp_path):
    """Everything ``merge_attention`` does not cover is a ``ValueError`` before any launch (on a machine without a device: before the
    engine would fail for lack of one); the option never becomes an attribute that shadows the static method."""
    from tiatoolbox_amd.models import DeepFeatureExtractor, IOPatchPredictorConfig, PatchPredictor

    cfg = IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(64, 64), stride_shape=(32, 32))
    patches, slides = np.zeros((2, 64, 64, 3), np.uint8), [np.zeros((96, 128, 3), np.uint8)]
    eng = _vit_engine(DeepFeatureExtractor)
    with pytest.raises(ValueError, match="patch_mode=True"):
        eng.run(patches, patch_mode=True, ioconfig=cfg, merge_attention="rollout")
    with pytest.raises(ValueError, match="merge_attention='heads'"):
        eng.run(slides, patch_mode=False, ioconfig=cfg, merge_attention="heads", save_dir=tmp_path / "a")
    with pytest.raises(ValueError, match="attention_interpolation='cubic'"):
        eng.run(slides, patch_mode=False, ioconfig=cfg, merge_attention="class", attention_interpolation="cubic", save_dir=tmp_path / "b")
    with pytest.raises(ValueError, match="bfloat16x3"):
        eng.run(slides, patch_mode=False, ioconfig=cfg, merge_attention="class", compute_dtype="bfloat16x3", save_dir=tmp_path / "c")
    assert getattr(eng, "compute_dtype", "float32") != "bfloat16x3"  # refused before any kwarg of the call became an attribute
    with pytest.raises(ValueError, match="merge_predictions"):  # still refused for features
        eng.run(slides, patch_mode=False, ioconfig=cfg, merge_predictions=True, merge_attention="class", save_dir=tmp_path / "d")
    assert eng.merge_attention is PatchPredictor.merge_attention and not list(tmp_path.iterdir())
    cnn = PatchPredictor("resnet18-kather100k", batch_size=4, device="cpu")
    with pytest.raises(ValueError, match="no VisionTransformer"):
        cnn.run(slides, patch_mode=False, merge_attention="rollout", save_dir=tmp_path / "e")
    assert cnn.merge_attention is PatchPredictor.merge_attention

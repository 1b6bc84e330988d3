"""Slide reads below the baseline resolution: ``resolution_factor``, ``VirtualWSIReader`` / its resampled view and
``tia_gather_area_patches_u8`` against a NumPy restatement of the reference's read (``read_bounds(..., resolution, units,
pad_constant_values=255)`` -> ``imresize`` -> ``cv2.INTER_AREA`` at an integer scale), and the engines' WSI mode on a slide
whose baseline is finer than the model's input resolution."""

from __future__ import annotations

import types

import numpy as np
import pytest
import torch

from tiatoolbox_amd.wsicore import ResampledWSIView, VirtualWSIReader, resolution_factor


# ---------------------------------------------------------------------------------------------- NumPy restatement
def area_round(sums: np.ndarray, k: int) -> np.ndarray:
    """OpenCV's resizeAreaFast for uint8: k == 2 -> (sum + 2) >> 2 (half up); k >= 3 -> float32(sum) * (1.0f / k^2), rounded
    half to even and saturated."""
    sums = np.asarray(sums, dtype=np.int64)
    if k == 1:
        return sums.astype(np.uint8)
    if k == 2:  # noqa: PLR2004
        return ((sums + 2) >> 2).astype(np.uint8)
    v = np.rint(sums.astype(np.float32) * (np.float32(1.0) / np.float32(k * k)))
    return np.minimum(v, 255).astype(np.uint8)


def area_shrink(region: np.ndarray, k: int) -> np.ndarray:
    """``[..., H, W, C]`` uint8 (H, W multiples of k) -> ``[..., H / k, W / k, C]``: box sums, then :func:`area_round`."""
    *lead, h, w, c = region.shape
    sums = region.reshape(*lead, h // k, k, w // k, k, c).sum(axis=(-4, -2), dtype=np.int64)
    return area_round(sums, k)


def area_read(slide: np.ndarray, bounds, k: int, pad: int = 255) -> np.ndarray:
    """Baseline ``bounds`` ``[M, 4]`` (extents ``k * (pw, ph)``): pad with ``pad`` outside the slide, then shrink by k."""
    s3 = slide if slide.ndim == 3 else slide[..., None]  # noqa: PLR2004
    b = np.asarray(bounds, dtype=np.int64).reshape(-1, 4)
    w, h = int(b[0, 2] - b[0, 0]), int(b[0, 3] - b[0, 1])
    margin = int(max(0, -b[:, :2].min(), (b[:, 2] - s3.shape[1]).max(), (b[:, 3] - s3.shape[0]).max()))
    padded = np.pad(s3, ((margin, margin), (margin, margin), (0, 0)), constant_values=pad)
    ys = b[:, 1:2] + margin + np.arange(h)[None]
    xs = b[:, 0:1] + margin + np.arange(w)[None]
    out = area_shrink(padded[ys[:, :, None], xs[:, None, :]], k)
    return out if slide.ndim == 3 else out[..., 0]  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_resolution_factor_known_values():
    assert resolution_factor(0.5, "mpp", mpp=0.25, power=40) == 2
    assert resolution_factor(0.5, "mpp", mpp=(0.25, 0.25), power=40) == 2
    assert resolution_factor(1.0, "mpp", mpp=0.25) == 4
    assert resolution_factor(20, "power", power=40) == 2
    assert resolution_factor(10, "power", power=40.0) == 4
    assert resolution_factor(0.25, "baseline") == 4
    assert resolution_factor(1.0, "baseline") == 1
    assert resolution_factor(0, "level") == 1
    assert resolution_factor(0.25, "mpp", mpp=0.25) == 1
    assert resolution_factor(0.5, "mpp", mpp=0.2500000001) == 2  # within the relative tolerance


@pytest.mark.parametrize(("args", "match"), [
    ((0.125, "mpp"), "up-samples"),
    ((80, "power"), "up-samples"),
    ((2.0, "baseline"), "up-samples"),
    ((0.6, "mpp"), "not an integer"),
    ((15, "power"), "not an integer"),
    ((0.4, "baseline"), "not an integer"),
    ((1, "level"), "one level"),
    ((0.5, "furlong"), "Invalid resolution units"),
    ((0.0, "mpp"), "positive"),
])
def test_resolution_factor_errors(args, match):
    with pytest.raises(ValueError, match=match):
        resolution_factor(*args, mpp=0.25, power=40)


def test_resolution_factor_missing_or_anisotropic_native():
    with pytest.raises(ValueError, match="native mpp is None"):
        resolution_factor(0.5, "mpp", mpp=None, power=40)
    with pytest.raises(ValueError, match="native power is None"):
        resolution_factor(20, "power", mpp=0.25, power=None)
    with pytest.raises(ValueError, match="differs between x and y"):
        resolution_factor(0.5, "mpp", mpp=(0.25, 0.26))


def test_restatement_rounding_known_answers():
    # k = 2: half up ((s + 2) >> 2): sums 2 and 10 (0.5, 2.5) round up, where half-to-even would round down
    assert area_round([0, 1, 2, 3, 6, 10, 1020], 2).tolist() == [0, 0, 1, 1, 2, 3, 255]
    box = np.array([[0, 0], [0, 2]], np.uint8)[..., None]
    assert area_shrink(box, 2)[0, 0, 0] == 1
    # k = 4 and k = 8: exact ties go to the even neighbour
    assert area_round([8, 24, 40, 7, 9, 4080], 4).tolist() == [0, 2, 2, 0, 1, 255]
    assert area_round([32, 96, 160, 31, 33, 16320], 8).tolist() == [0, 2, 2, 0, 1, 255]
    tie = np.zeros((4, 4, 1), np.uint8)
    tie[0, :2] = 4  # sum 8 -> 0.5 -> 0
    assert area_shrink(tie, 4)[0, 0, 0] == 0
    tie[0, :2] = 12  # sum 24 -> 1.5 -> 2
    assert area_shrink(tie, 4)[0, 0, 0] == 2
    # k = 3: float32(sum) * float32(1 / 9) then rint
    assert area_round([4, 5, 13, 14, 2295], 3).tolist() == [0, 1, 1, 2, 255]


def test_restatement_pads_before_averaging():
    slide = np.zeros((4, 4, 1), np.uint8)
    out = area_read(slide, [[-1, 0, 1, 2]], 2)  # half the box outside the slide: (255 + 0 + 255 + 0 + 2) >> 2
    assert out.shape == (1, 1, 1, 1) and out[0, 0, 0, 0] == 128
    assert area_read(slide, [[10, 10, 12, 12]], 2)[0, 0, 0, 0] == 255


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("c", [1, 3])
def test_restatement_matches_cv2_inter_area(k, c):
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(k * 10 + c)
    ph, pw = 13, 11
    region = rng.integers(0, 256, (ph * k, pw * k, c), dtype=np.uint8)
    region[: k * 3] = rng.integers(0, 4, (k * 3, pw * k, c), dtype=np.uint8)  # small values: many exact ties
    got = cv2.resize(region, (pw, ph), interpolation=cv2.INTER_AREA)
    exp = area_shrink(region, k)
    np.testing.assert_array_equal(got.reshape(exp.shape), exp)


def test_view_dimensions_follow_numpy_round():
    """``np.round(W / k)`` (halves to even), the reference's ``_find_read_bounds_params`` rule."""
    base = types.SimpleNamespace(slide_dimensions=(1003, 1001), mode="rgb", mpp=0.25, power=40.0)
    view = ResampledWSIView(base, 2)
    assert view.slide_dimensions == (502, 500)  # 501.5 -> 502, 500.5 -> 500
    assert view.mpp == 0.5 and view.power == 20.0
    assert ResampledWSIView(base, 4).slide_dimensions == (251, 250)  # 250.75, 250.25
    aniso = types.SimpleNamespace(slide_dimensions=(8, 8), mode="rgb", mpp=(0.25, 0.25), power=None)
    v = ResampledWSIView(aniso, 2)
    assert v.mpp == (0.5, 0.5) and v.power is None


def test_engine_helper_checks_output_resolutions():
    from tiatoolbox_amd.models.engine.io_config import IOSegmentorConfig
    from tiatoolbox_amd.models.engine.semantic_segmentor import SemanticSegmentor

    reader = VirtualWSIReader.__new__(VirtualWSIReader)  # resolution metadata only: no device image needed here
    reader.mpp, reader.power, reader.mode = 0.25, 40.0, "rgb"
    eng = SemanticSegmentor.__new__(SemanticSegmentor)
    same = {"units": "mpp", "resolution": 0.5}
    eng._ioconfig = IOSegmentorConfig(input_resolutions=[same], output_resolutions=[same], patch_input_shape=[64, 64],  # noqa: SLF001
                                      patch_output_shape=[32, 32], save_resolution=same)
    view = eng._reader_at_input_resolution(reader)  # noqa: SLF001
    assert isinstance(view, ResampledWSIView) and view.factor == 2 and view.base is reader
    eng._ioconfig = IOSegmentorConfig(input_resolutions=[same], output_resolutions=[{"units": "mpp", "resolution": 1.0}],  # noqa: SLF001
                                      patch_input_shape=[64, 64], patch_output_shape=[32, 32], save_resolution=same)
    with pytest.raises(ValueError, match="equal to the input resolution"):
        eng._reader_at_input_resolution(reader)  # noqa: SLF001
    native = {"units": "mpp", "resolution": 0.25}
    eng._ioconfig = IOSegmentorConfig(input_resolutions=[native], output_resolutions=[{"units": "mpp", "resolution": 1.0}],  # noqa: SLF001
                                      patch_input_shape=[64, 64], patch_output_shape=[32, 32])
    assert eng._reader_at_input_resolution(reader) is reader  # native resolution: the reader itself  # noqa: SLF001
    assert eng._reader_at_input_resolution("not a virtual reader") == "not a virtual reader"  # noqa: SLF001


# ------------------------------------------------------------------------------------------------------ GPU tests
def _edge_bounds(sw: int, sh: int, w: int, h: int, rng) -> np.ndarray:
    """Regions of w x h baseline pixels over every edge and corner, fully outside, inside, at byte-unaligned x offsets."""
    xs = [-w - 3, -w + 1, -5, 0, 1, 3, 7, sw // 2 - w // 2, sw - w, sw - w + 5, sw - 1, sw + 2]
    ys = [-h - 1, -h + 2, -3, 0, 2, sh // 2 - h // 2, sh - h, sh - h + 3, sh - 1, sh + 4]
    pts = [(x, y) for x in xs for y in ys]
    pick = rng.choice(len(pts), size=14, replace=False)
    corners = [(-5, -3), (sw - w + 5, -3), (-5, sh - h + 3), (sw - w + 5, sh - h + 3), (-w - 3, -h - 1), (sw + 2, sh + 4), (1, 2)]
    sel = corners + [pts[i] for i in pick]
    return np.array([[x, y, x + w, y + h] for x, y in sel], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
def test_hip_area_gather_matches_restatement(k, c):
    from tiatoolbox_amd.wsicore import ArrayWSIReader, _area_read

    rng = np.random.default_rng(100 * k + c)
    sh, sw = 301, 517
    slide = rng.integers(0, 256, (sh, sw, c), dtype=np.uint8)
    slide[:40] = rng.integers(0, 3, (40, sw, c), dtype=np.uint8)  # low values: many rounding ties
    if c == 1:
        slide = slide[..., 0].copy()
    reader = VirtualWSIReader(slide, mpp=0.25, power=40.0)
    for ph, pw in [(224, 224), (64, 48), (20, 7), (5, 5)]:
        b = _edge_bounds(sw, sh, pw * k, ph * k, rng)
        exp = area_read(slide, b, k)
        dev = torch.from_numpy(b).cuda()
        got = _area_read(reader, dev, (pw, ph), k, 255).cpu().numpy()
        assert got.shape == exp.shape, (got.shape, exp.shape)
        np.testing.assert_array_equal(got, exp, err_msg=f"k={k} c={c} {ph}x{pw}")
        # the view: bounds in its own pixels, host and device (size=) forms
        view = ResampledWSIView(reader, k)
        vb = np.array([[x, y, x + pw, y + ph] for x, y in rng.integers(-pw, 300 // k + 2, (6, 2)).tolist()], np.int32)
        vexp = area_read(slide, vb * k, k)
        np.testing.assert_array_equal(view.read_bounds_batch(vb).cpu().numpy(), vexp)
        np.testing.assert_array_equal(view.read_bounds_batch(torch.from_numpy(vb).cuda(), size=(pw, ph)).cpu().numpy(), vexp)
        if k == 1:  # factor 1 == the plain gather, byte for byte
            np.testing.assert_array_equal(got, ArrayWSIReader(slide).read_bounds_batch(b).cpu().numpy())


@pytest.mark.gpu
def test_hip_area_gather_many_patches():
    """More patches than one launch's grid-y limit (65,535): the launcher chunks them."""
    from tiatoolbox_amd.wsicore import _area_read

    rng = np.random.default_rng(11)
    slide = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    reader = VirtualWSIReader(slide)
    m, k, pw, ph = 70001, 2, 5, 5
    xy = rng.integers(-12, 135, (m, 2))
    b = np.concatenate([xy, xy + [pw * k, ph * k]], axis=1).astype(np.int32)
    got = _area_read(reader, torch.from_numpy(b).cuda(), (pw, ph), k, 255).cpu().numpy()
    np.testing.assert_array_equal(got, area_read(slide, b, k))


@pytest.mark.gpu
def test_virtual_reader_read_bounds_resolution():
    rng = np.random.default_rng(3)
    slide = rng.integers(0, 256, (203, 317, 3), dtype=np.uint8)
    reader = VirtualWSIReader(slide, mpp=0.25, power=40.0)
    # coord_space="resolution": bounds at 0.5 mpp
    got = reader.read_bounds([150, 90, 170, 112], resolution=0.5, units="mpp", coord_space="resolution")
    np.testing.assert_array_equal(got, area_read(slide, [[300, 180, 340, 224]], 2)[0])
    got = reader.read_bounds([-3, -2, 9, 6], resolution=10, units="power", coord_space="resolution")
    np.testing.assert_array_equal(got, area_read(slide, [[-12, -8, 36, 24]], 4)[0])
    # coord_space="baseline": baseline bounds at any offset, extents multiples of the factor
    got = reader.read_bounds([301, 195, 325, 213], resolution=0.75, units="mpp")
    np.testing.assert_array_equal(got, area_read(slide, [[301, 195, 325, 213]], 3)[0])
    with pytest.raises(ValueError, match="integer factor"):
        reader.read_bounds([0, 0, 25, 24], resolution=0.5, units="mpp")
    # no resolution: the ArrayWSIReader read; pad value honoured
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    np.testing.assert_array_equal(reader.read_bounds([-4, 200, 16, 208]), ArrayWSIReader(slide).read_bounds([-4, 200, 16, 208]))
    assert (reader.read_bounds([-4, -4, 0, 0], pad_constant_values=7) == 7).all()
    with pytest.raises(ValueError, match="up-samples"):
        reader.read_bounds([0, 0, 8, 8], resolution=0.125, units="mpp", coord_space="resolution")
    view = reader.at_resolution(0.5, "mpp")
    assert view.slide_dimensions == (158, 102) and view.mpp == 0.5 and view.power == 20.0  # 158.5 -> 158, 101.5 -> 102
    assert not hasattr(view, "device_image")
    mask = view.tissue_mask(resolution=1.25, units="power")
    np.testing.assert_array_equal(np.asarray(mask.img), np.asarray(reader.tissue_mask(resolution=1.25, units="power").img))


def _tissue_slide(h: int, w: int, seed: int) -> np.ndarray:
    from tiatoolbox_amd.utils import synth

    slide = np.full((h, w, 3), 245, np.uint8)
    slide[h // 7:h - h // 7, w // 10:w - w // 10] = synth.g_he(1, h - 2 * (h // 7), w - 2 * (w // 10), seed=seed)[0]
    return slide


@pytest.mark.gpu
def test_patch_predictor_wsi_mode_on_resampled_slide(tmp_path):
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.tools.patchextraction import PatchExtractor
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    slide = _tissue_slide(2000, 2360, seed=9)  # 0.25 mpp / 40x
    down = area_shrink(slide, 2)                # the same slide at 0.5 mpp / 20x
    eng = PatchPredictor("resnet18-kather100k", batch_size=8, device="cuda")
    virt = VirtualWSIReader(slide, mpp=0.25, power=40.0)
    arr = ArrayWSIReader(down, mpp=0.5, power=20.0)

    def run(reader, name, **kw):
        path = eng.run([reader], patch_mode=False, save_dir=tmp_path / name, return_probabilities=True, **kw)[0]
        with np.load(path) as res:
            return {k: res[k] for k in res.files}

    # automatic tissue mask: computed from the baseline slide, applied to the 0.5-mpp grid
    auto = run(virt, "auto")
    grid = PatchExtractor.get_coordinates(image_shape=(1180, 1000), patch_input_shape=(224, 224), stride_shape=(224, 224))
    base_mask = virt.tissue_mask(resolution=1.25, units="power")
    keep = PatchExtractor.filter_coordinates(base_mask, grid, wsi_shape=(1180, 1000), min_mask_ratio=0)
    assert np.array_equal(auto["coordinates"], grid[keep]) and 4 < len(auto["coordinates"]) <= len(grid)
    ref = run(arr, "auto_ref", masks=[np.asarray(base_mask.img)])
    assert np.array_equal(auto["coordinates"], ref["coordinates"])
    assert np.array_equal(auto["predictions"], ref["predictions"])
    np.testing.assert_allclose(auto["probabilities"], ref["probabilities"], rtol=0, atol=1e-6)
    # objective power units
    power = [{"units": "power", "resolution": 20.0}]
    mask = np.zeros((1000, 1180), np.uint8)
    mask[150:800, 200:1000] = 1
    got = run(virt, "power", masks=[mask], input_resolutions=power)
    exp = run(arr, "power_ref", masks=[mask], input_resolutions=power)
    assert np.array_equal(got["coordinates"], exp["coordinates"]) and np.array_equal(got["predictions"], exp["predictions"])
    np.testing.assert_allclose(got["probabilities"], exp["probabilities"], rtol=0, atol=1e-6)
    # a 0.5-mpp slide read at 0.25 mpp would be up-sampled
    with pytest.raises(ValueError, match="up-samples"):
        eng.run([VirtualWSIReader(down, mpp=0.5, power=20.0)], patch_mode=False, save_dir=tmp_path / "up",
                input_resolutions=[{"units": "mpp", "resolution": 0.25}])


@pytest.mark.gpu
def test_patch_predictor_odd_slide_edges(tmp_path):
    """Odd baseline dimensions: the grid follows ``np.round(W / k)`` and the right / bottom patches average slide bytes
    with the 255 padding."""
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor
    from tiatoolbox_amd.tools.patchextraction import PatchExtractor

    slide = _tissue_slide(1001, 1003, seed=4)
    virt = VirtualWSIReader(slide, mpp=0.25, power=40.0)
    view = virt.at_resolution(0.5, "mpp")
    assert view.slide_dimensions == (502, 500)
    mask = np.ones((1001, 1003), np.uint8)
    eng = PatchPredictor("resnet18-kather100k", batch_size=4, device="cuda")
    path = eng.run([virt], masks=[mask], patch_mode=False, save_dir=tmp_path / "odd", return_probabilities=True)[0]
    with np.load(path) as res:
        coords, probs = res["coordinates"], res["probabilities"]
    grid = PatchExtractor.get_coordinates(image_shape=(502, 500), patch_input_shape=(224, 224), stride_shape=(224, 224))
    assert np.array_equal(coords, grid) and coords[:, 2].max() > 502 and coords[:, 3].max() > 500
    patches = area_read(slide, coords * 2, 2)
    np.testing.assert_array_equal(view.read_bounds_batch(coords).cpu().numpy(), patches)
    edge = patches[np.argmax(coords[:, 2] + coords[:, 3])]
    assert (edge[-1, -1] == 255).all()  # beyond the slide: pad only
    y0, x0 = int(coords[np.argmax(coords[:, 2] + coords[:, 3]), 1]), int(coords[np.argmax(coords[:, 2] + coords[:, 3]), 0])
    # view row 500 = baseline rows 1000 (the slide's last) and 1001 (pad): slide bytes averaged with 255, half up
    box = slide[1000, 2 * x0:2 * x0 + 2].astype(int).sum(0) + 2 * 255
    np.testing.assert_array_equal(edge[500 - y0, 0], (box + 2) >> 2)
    exp = PatchPredictor("resnet18-kather100k", batch_size=4, device="cuda").run(patches, patch_mode=True, return_probabilities=True)
    np.testing.assert_allclose(probs, exp["probabilities"], atol=1e-5)


@pytest.mark.gpu
def test_semantic_segmentor_wsi_mode_on_resampled_slide(tmp_path):
    from tiatoolbox_amd.models.architecture.unet import UNetModel
    from tiatoolbox_amd.models.engine.io_config import IOSegmentorConfig
    from tiatoolbox_amd.models.engine.semantic_segmentor import SemanticSegmentor
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    torch.manual_seed(0)
    model = UNetModel(3, 3, "resnet50").eval()
    res = {"units": "mpp", "resolution": 0.5}
    cfg = IOSegmentorConfig(input_resolutions=[res], output_resolutions=[res], patch_input_shape=[128, 128],
                            patch_output_shape=[64, 64], stride_shape=[50, 50], save_resolution=res)
    slide = _tissue_slide(1200, 1400, seed=3)
    down = area_shrink(slide, 2)
    mask = np.zeros((600, 700), np.uint8)
    mask[100:480, 120:600] = 1
    eng = SemanticSegmentor(model, batch_size=8, device="cuda")
    out = {}
    for name, reader in [("virt", VirtualWSIReader(slide, mpp=0.25, power=40)), ("ref", ArrayWSIReader(down, mpp=0.5, power=20))]:
        path = eng.run([reader], masks=[mask], patch_mode=False, ioconfig=cfg, return_probabilities=True, save_dir=tmp_path / name)[0]
        with np.load(path) as r:
            out[name] = {k: r[k] for k in r.files}
    got, exp = out["virt"], out["ref"]
    assert got["predictions"].shape == (600, 700) and got["probabilities"].shape == (600, 700, 3)
    assert np.array_equal(got["coordinates"], exp["coordinates"])
    assert np.array_equal(got["predictions"], exp["predictions"])
    np.testing.assert_allclose(got["probabilities"], exp["probabilities"], rtol=0, atol=1e-6)


def _stub_hovernet():
    """HoVer-Net whose heads are a deterministic function of the input pixels (random weights give no nuclei)."""
    from tiatoolbox_amd.models.architecture.hovernet import HoVerNet

    class _Stub(HoVerNet):
        @staticmethod
        def infer_batch(model, batch_data, *, device):  # noqa: ARG004
            x = torch.as_tensor(batch_data).to(device).float()
            dark = (1.0 - x.mean(-1) / 255.0)[:, 46:210, 46:210]
            ramp = torch.linspace(-1, 1, 164, device=dark.device)
            hv = torch.stack([ramp[None, None, :] * dark, ramp[None, :, None] * dark], dim=-1)
            return dark[..., None].contiguous(), hv.contiguous(), (1.0 + (dark > 0.8).float())[..., None].contiguous()

    torch.manual_seed(0)
    return _Stub(num_types=6, mode="fast")


@pytest.mark.gpu
def test_multitask_segmentor_process_wsi_on_resampled_slide(tmp_path):
    from tiatoolbox_amd.models.architecture import get_pretrained_model
    from tiatoolbox_amd.models.engine.multi_task_segmentor import MultiTaskSegmentor
    from tiatoolbox_amd.utils import synth
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    rng = np.random.default_rng(5)
    slide = np.full((900, 1300, 3), 244, np.uint8)
    tissue = synth.g_he(8, 256, 256, seed=23)
    yy, xx = np.mgrid[0:900, 0:1300]
    for k, (y, x) in enumerate([(100, 30), (100, 286), (356, 30), (356, 286), (356, 542), (560, 1000), (300, 1000)]):
        slide[y:y + 256, x:x + 256] = tissue[k]
        for _ in range(14):
            cy, cx, r = rng.integers(y + 8, y + 248), rng.integers(x + 8, x + 248), rng.integers(5, 10)
            slide[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 25
    slide2x = np.repeat(np.repeat(slide, 2, axis=0), 2, axis=1)  # 0.125 mpp
    slide2x[1::2, 1::2] = np.clip(slide2x[1::2, 1::2].astype(int) + 1, 0, 255)  # not a plain repeat: rounding matters
    down = area_shrink(slide2x, 2)
    cfg = get_pretrained_model("hovernet_fast-pannuke")[1]
    mask = np.zeros((900, 1300), np.uint8)
    mask[80:880, 0:1300] = 1
    eng = MultiTaskSegmentor(_stub_hovernet(), batch_size=4, device="cuda")
    virt = VirtualWSIReader(slide2x, mpp=0.125, power=80.0)
    arr = ArrayWSIReader(down, mpp=0.25, power=40.0)
    eng.run([arr], masks=[mask], patch_mode=False, ioconfig=cfg, save_dir=tmp_path / "ref")  # sets the engine's ioconfig
    got = eng.process_wsi(virt, mask, return_predictions=(True,))
    exp = eng.process_wsi(arr, mask, return_predictions=(True,))
    assert np.array_equal(got["coordinates"], exp["coordinates"])
    assert got["predictions"].shape == (900, 1300) and np.array_equal(got["predictions"], exp["predictions"])
    assert len(exp["box"]) > 30
    for key in ("box", "centroid", "prob", "type"):
        a = np.array(list(got[key]), dtype=np.float64)
        b = np.array(list(exp[key]), dtype=np.float64)
        assert np.array_equal(a, b), key
    assert all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(got["contours"], exp["contours"], strict=True))

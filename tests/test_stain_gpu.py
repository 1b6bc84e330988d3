"""GPU parity: HIP stain path (through the C ABI) vs the CPU oracle and the reference goldens.

Tolerances (BASELINE.json north_star): integer/index work bit-exact (tissue masks, counts,
contrast-enhancer percentiles); float stain-normalised pixels within 1e-4 *before* the
``astype(uint8)`` truncation; the uint8 output may therefore differ by at most 1 LSB on a
vanishing fraction of bytes (a value sitting within 1e-4 of an integer boundary).
"""

from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oracle import stain as ostain
from tiatoolbox_amd.utils import synth

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).parent / "golden"
FLOAT_TOL = 1e-4          # on the pre-cast float in [0, 255]
STAT_TOL = 1e-9           # per-patch f64 statistics


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "stain_golden.npz")


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


def _u8_close(a: np.ndarray, b: np.ndarray, max_rate: float = 2e-4) -> float:
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    assert d.max() <= 1, f"max byte difference {d.max()}"
    rate = float((d != 0).mean())
    assert rate <= max_rate, f"byte mismatch rate {rate}"
    return rate


def _stats(batch_np, torch_mod, **kw):
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import _stain_device as dev

    t = torch_mod.from_numpy(batch_np).cuda()
    params = dev.make_params(mode=_lib.MODE_MACENKO, **kw)
    return dev.stain_stats(t, params).cpu().numpy(), params


def _large_image(h, w, seed):
    """H&E-like image of any size: G-he blocks of 250 x 250 tiled, a white margin on two sides, a black corner (zeros: rgb2od's
    0 -> 1 rule), cropped to (h, w)."""
    bh, bw = -(-h // 250), -(-w // 250)
    blocks = synth.g_he(bh * bw, 250, 250, seed=seed).reshape(bh, bw, 250, 250, 3)
    img = blocks.transpose(0, 2, 1, 3, 4).reshape(bh * 250, bw * 250, 3)[:h, :w].copy()
    img[: h // 16] = 250
    img[:, : w // 20] = 252
    img[-8:, -8:] = 0
    return img


@pytest.mark.parametrize("shape", [(1000, 1000), (3000, 2500), (777, 1203)])
def test_large_single_images_take_the_multi_workgroup_path(torch_mod, shape):
    """One image above 4 x 256 x 256 pixels: every sweep of the statistics runs over many workgroups (stain_stats_big.hip) instead of
    one per image.  Against the oracle on the whole image (1e-9 like the per-patch kernels), against the streaming kernel's record
    (select_mode 2 keeps it: agreement to rounding of the moment sums), and for a batch of two such images at once; fixed
    matrices (Ruifrok) and the zero -> one rule take the same path."""
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import _stain_device as dev

    h, w = shape
    imgs = np.stack([_large_image(h, w, seed=h + k) for k in range(2)])
    stats, _ = _stats(imgs, torch_mod)
    ref, _ = _stats(imgs, torch_mod, select_mode=2)
    for i, img in enumerate(imgs):
        s, r = stats[i], ref[i]
        assert int(s[_lib.ST_FLAGS]) == 0 and s[_lib.ST_NTISSUE] == r[_lib.ST_NTISSUE]
        assert s[_lib.ST_PLOW] == r[_lib.ST_PLOW] and s[_lib.ST_PHIGH] == r[_lib.ST_PHIGH]
        for lo, n in ((_lib.ST_STAIN, 6), (_lib.ST_MAXC, 2), (_lib.ST_MINPHI, 2), (_lib.ST_COV, 6), (_lib.ST_EVEC, 6), (_lib.ST_PINV, 6)):
            np.testing.assert_allclose(s[lo:lo + n], r[lo:lo + n], rtol=1e-9, atol=1e-10)  # (moment sums of millions of pixels in another order)
    img = imgs[0]
    dbg: dict = {}
    sm = ostain.MacenkoExtractor().get_stain_matrix(img.copy(), debug=dbg)
    s = stats[0]
    assert int(s[_lib.ST_NTISSUE]) == dbg["n_tissue"]
    pl, ph = np.percentile(img, (2, 98))
    assert s[_lib.ST_PLOW] == pl and s[_lib.ST_PHIGH] == ph
    np.testing.assert_allclose(s[_lib.ST_MINPHI], dbg["min_phi"], atol=STAT_TOL)
    np.testing.assert_allclose(s[_lib.ST_MAXPHI], dbg["max_phi"], atol=STAT_TOL)
    np.testing.assert_allclose(s[_lib.ST_STAIN:_lib.ST_STAIN + 6].reshape(2, 3), sm, atol=STAT_TOL)
    conc = ostain.StainNormalizer.get_concentrations(img.copy(), sm)
    np.testing.assert_allclose(s[_lib.ST_MAXC:_lib.ST_MAXC + 2], np.percentile(conc, 99, axis=0), atol=STAT_TOL)
    # fixed stain matrix (Ruifrok) with a target: PINV, MAXC and the fused matrix
    t = torch_mod.from_numpy(imgs[:1]).cuda()
    ruifrok = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])
    ruifrok /= np.linalg.norm(ruifrok, axis=1, keepdims=True)
    kw = {"mode": _lib.MODE_FIXED, "stain_fixed": ruifrok, "target_stain": ruifrok, "target_maxc": np.array([[1.5, 0.9]]), "zero_to_one": True}
    big = dev.stain_stats(t, dev.make_params(**kw)).cpu().numpy()[0]
    small = dev.stain_stats(t, dev.make_params(select_mode=2, **kw)).cpu().numpy()[0]
    np.testing.assert_allclose(big[:48], small[:48], rtol=1e-12, atol=1e-13)
    conc = ostain.StainNormalizer.get_concentrations(img.copy(), ruifrok)
    np.testing.assert_allclose(big[_lib.ST_MAXC:_lib.ST_MAXC + 2], np.percentile(conc, 99, axis=0), atol=STAT_TOL)


def test_large_images_with_massive_ties_take_the_radix_fall_back(torch_mod):
    """A posterised large image (eight levels per channel: a few hundred distinct colours over 2.4 M pixels) puts far more than 16 Ki
    equal keys into the bins of the percentile ranks: the candidate lists overflow and the selection goes to the radix passes over
    the image -- ONE launch whose workgroups meet at a grid barrier between the digit passes (`big_select_sweep_kernel`).  The record
    says so (the diagnostics slots), and the results equal the streaming kernel's and the oracle's; a batch of two exercises two
    independent barriers in one launch."""
    from tiatoolbox_amd import _lib

    imgs = np.stack([_large_image(1536, 1600, seed=70 + k) for k in range(2)])
    imgs = (np.clip(imgs.astype(int) // 32 * 32 + 16, 0, 255)).astype(np.uint8)
    stats, _ = _stats(imgs, torch_mod)
    ref, _ = _stats(imgs, torch_mod, select_mode=2)
    for i in range(2):
        s, r = stats[i], ref[i]
        assert int(s[_lib.ST_FLAGS]) == 0
        assert s[_lib.ST_CYCLES] == 1.0 or s[_lib.ST_CYCLES + 5] == 1.0, "no selection fell back: the image does not test what it says"
        for lo, n in ((_lib.ST_STAIN, 6), (_lib.ST_MAXC, 2), (_lib.ST_MINPHI, 2), (_lib.ST_COV, 6), (_lib.ST_EVEC, 6), (_lib.ST_PINV, 6)):
            np.testing.assert_allclose(s[lo:lo + n], r[lo:lo + n], rtol=1e-9, atol=1e-10)
    img = imgs[1]
    dbg: dict = {}
    sm = ostain.MacenkoExtractor().get_stain_matrix(img.copy(), debug=dbg)
    s = stats[1]
    np.testing.assert_allclose(s[_lib.ST_MINPHI], dbg["min_phi"], atol=STAT_TOL)
    np.testing.assert_allclose(s[_lib.ST_MAXPHI], dbg["max_phi"], atol=STAT_TOL)
    np.testing.assert_allclose(s[_lib.ST_STAIN:_lib.ST_STAIN + 6].reshape(2, 3), sm, atol=STAT_TOL)
    conc = ostain.StainNormalizer.get_concentrations(img.copy(), sm)
    np.testing.assert_allclose(s[_lib.ST_MAXC:_lib.ST_MAXC + 2], np.percentile(conc, 99, axis=0), atol=STAT_TOL)


@pytest.mark.parametrize("shape", [(64, 64), (96, 96), (37, 41), (256, 256), (224, 224)])
def test_macenko_stats_match_oracle(torch_mod, shape):
    from tiatoolbox_amd import _lib

    imgs = synth.g_he(3, *shape, seed=5)
    stats, _ = _stats(imgs, torch_mod)
    for i, img in enumerate(imgs):
        dbg: dict = {}
        sm = ostain.MacenkoExtractor().get_stain_matrix(img.copy(), debug=dbg)
        s = stats[i]
        assert int(s[_lib.ST_FLAGS]) == 0
        assert int(s[_lib.ST_NTISSUE]) == dbg["n_tissue"]          # integer mask work: exact
        pl, ph = np.percentile(img, (2, 98))
        assert s[_lib.ST_PLOW] == pl and s[_lib.ST_PHIGH] == ph      # exact f64 equality
        cov = dbg["cov"]
        got = np.array([s[_lib.ST_COV + k] for k in range(6)])
        exp = np.array([cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]])
        np.testing.assert_allclose(got, exp, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(s[_lib.ST_EVEC:_lib.ST_EVEC + 6].reshape(2, 3).T, dbg["eigen_vectors"], atol=STAT_TOL)
        np.testing.assert_allclose(s[_lib.ST_MINPHI], dbg["min_phi"], atol=STAT_TOL)
        np.testing.assert_allclose(s[_lib.ST_MAXPHI], dbg["max_phi"], atol=STAT_TOL)
        np.testing.assert_allclose(s[_lib.ST_STAIN:_lib.ST_STAIN + 6].reshape(2, 3), sm, atol=STAT_TOL)
        conc = ostain.StainNormalizer.get_concentrations(img.copy(), sm)
        np.testing.assert_allclose(s[_lib.ST_MAXC:_lib.ST_MAXC + 2], np.percentile(conc, 99, axis=0), atol=STAT_TOL)


def test_mask_and_contrast_enhancer_bit_exact(torch_mod, gold):
    from tiatoolbox_amd.utils import misc

    crops = gold["real_crops"]
    assert np.array_equal(misc.contrast_enhancer(crops), gold["ce_real"])
    assert np.array_equal(misc.get_luminosity_tissue_mask(crops, 0.8), gold["mask08_real"])
    he = synth.g_he(3, 96, 96, seed=int(gold["he_seed"]))
    assert np.array_equal(misc.get_luminosity_tissue_mask(he, 0.85), gold["mask085_he"])
    # the reference's own 27-value golden (tests/test_utils.py:882-911)
    inp = np.array([[[37, 244, 193], [106, 235, 128], [71, 140, 47]],
                    [[103, 184, 72], [20, 188, 238], [126, 7, 0]],
                    [[137, 195, 204], [32, 203, 170], [101, 77, 133]]], dtype=np.uint8)
    exp = np.array([[[35, 255, 203], [110, 248, 133], [72, 146, 46]],
                    [[106, 193, 73], [17, 198, 251], [131, 3, 0]],
                    [[143, 205, 215], [30, 214, 178], [104, 78, 139]]], dtype=np.uint8)
    assert np.array_equal(misc.contrast_enhancer(inp, low_p=2, high_p=98), exp)
    with pytest.raises(AssertionError):
        misc.contrast_enhancer(np.float32(inp), low_p=2, high_p=98)
    with pytest.raises(ValueError, match="Empty tissue mask"):
        misc.get_luminosity_tissue_mask(np.zeros((100, 100, 3)), threshold=0)


@pytest.mark.parametrize("method", ["macenko", "ruifrok", "custom"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_normalizer_matches_reference_goldens(gold, target_image, method, precision):
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    sm = np.array([[0.60, 0.72, 0.34], [0.10, 0.95, 0.29]]) if method == "custom" else None
    norm = get_normalizer(method, stain_matrix=sm)
    norm.precision = precision
    norm.fit(target_image)
    np.testing.assert_allclose(norm.stain_matrix_target, gold[f"{method}_stain_matrix_target"], atol=STAT_TOL)
    np.testing.assert_allclose(norm.maxC_target, gold[f"{method}_maxC_target"], atol=STAT_TOL)
    assert norm.maxC_target.shape == (1, 2)
    assert np.array_equal(norm.stain_matrix_target_RGB, gold[f"{method}_stain_matrix_target_RGB"])
    np.testing.assert_allclose(norm.target_concentrations[:64], gold[f"{method}_target_conc_head"], atol=STAT_TOL)
    he = synth.g_he(3, 96, 96, seed=int(gold["he_seed"]))
    # batch call and per-image calls give the same bytes
    out_real = norm.transform(gold["real_crops"])
    _u8_close(out_real, gold[f"{method}_real"], max_rate=2e-4 if precision == "f64" else 2e-3)
    out_he = np.stack([norm.transform(p) for p in he])
    _u8_close(out_he, gold[f"{method}_he"], max_rate=2e-4 if precision == "f64" else 2e-3)
    assert out_real.dtype == np.uint8 and out_real.shape == gold["real_crops"].shape


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_transform_float_within_1e4(he_patches, precision):
    """The north-star float bar: |HIP - oracle| <= 1e-4 on the pre-cast float pixels."""
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    norm = get_normalizer("macenko")
    norm.precision = precision
    norm.fit(he_patches[0])
    ref = ostain.get_normalizer("macenko")
    ref.fit(he_patches[0].copy())
    got = norm.transform(he_patches[1:5], out="float64" if precision == "f64" else "float32")
    exp = np.stack([ref.transform_float(p.copy()) for p in he_patches[1:5]])
    err = np.abs(got.astype(np.float64) - exp).max()
    assert err <= FLOAT_TOL, err
    u8 = norm.transform(he_patches[1:5])
    rate = _u8_close(u8, exp.astype(np.uint8), max_rate=2e-4 if precision == "f64" else 2e-3)
    print(f"[{precision}] max float err {err:.3e}, uint8 mismatch rate {rate:.2e}")


def test_unit_outputs_equal_totensor(he_patches, torch_mod):
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    norm = get_normalizer("macenko")
    norm.fit(he_patches[0])
    u8 = norm.transform(he_patches[1:3])
    for kind, dt in (("unit_float32", torch_mod.float32), ("unit_float16", torch_mod.float16),
                     ("unit_bfloat16", torch_mod.bfloat16)):
        t = norm.transform(torch_mod.from_numpy(he_patches[1:3]).cuda(), out=kind)
        exp = (torch_mod.from_numpy(u8).to(torch_mod.float32) / 255).to(dt)
        assert t.dtype == dt and torch_mod.equal(t.cpu(), exp)


def test_uniform_random_bytes(uniform_patches):
    """Stress input (G-uniform): every byte value, zeros included (rgb2od's 0 -> 1 rule)."""
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    norm = get_normalizer("ruifrok")
    norm.fit(uniform_patches[0])
    ref = ostain.get_normalizer("ruifrok")
    ref.fit(uniform_patches[0].copy())
    got = norm.transform(uniform_patches[1:], out="float64")
    exp = np.stack([ref.transform_float(p.copy()) for p in uniform_patches[1:]])
    assert np.abs(got - exp).max() <= FLOAT_TOL
    before = uniform_patches.copy()
    norm.transform(uniform_patches[1:])
    assert np.array_equal(before, uniform_patches), "input must not be modified"


def test_empty_mask_raises(he_patches):
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    norm = get_normalizer("macenko")
    norm.fit(he_patches[0])
    white = np.full((2, 32, 32, 3), 255, np.uint8)
    with pytest.raises(ValueError, match="Empty tissue mask"):
        norm.transform(white)
    with pytest.raises(ValueError, match="Empty tissue mask"):
        ostain.get_normalizer("macenko").fit(white[0].copy())


def test_constant_image_and_degenerate_selection():
    """All pixels identical: every order statistic collapses to one value (no LDS overflow)."""
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    img = np.full((1, 128, 128, 3), 120, np.uint8)
    img[0, :, :, 1] = 60
    norm = get_normalizer("ruifrok")
    norm.fit(img[0])
    ref = ostain.get_normalizer("ruifrok")
    ref.fit(img[0].copy())
    np.testing.assert_allclose(norm.maxC_target, ref.maxC_target, atol=STAT_TOL)
    _u8_close(norm.transform(img), np.stack([ref.transform(img[0].copy())]))


def test_large_batch_properties(torch_mod):
    """Full-size (BASELINE configs[1] shape) size-independent properties on 1024 x 224x224 patches:
    batch == per-chunk results, permutation equivariance, determinism."""
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    patches = torch_mod.from_numpy(synth.g_he(64, 224, 224, seed=9)).cuda().repeat(16, 1, 1, 1)
    perm = torch_mod.randperm(patches.shape[0], generator=torch_mod.Generator().manual_seed(0)).cuda()
    norm = get_normalizer("macenko")
    norm.precision = "f32"
    norm.fit(patches[0])
    full = norm.transform(patches)
    again = norm.transform(patches)
    assert torch_mod.equal(full, again)
    chunks = torch_mod.cat([norm.transform(patches[i:i + 100]) for i in range(0, patches.shape[0], 100)])
    assert torch_mod.equal(full, chunks)
    assert torch_mod.equal(norm.transform(patches[perm]), full[perm])
    assert torch_mod.equal(full[:64], full[64:128])  # repeated content, repeated output


def test_big_single_image_matches_oracle(target_image):
    """One workgroup walking a large image (the fit() target case, 1000x1000 in the reference)."""
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    big = np.tile(target_image, (3, 3, 1))[:700, :650]
    norm = get_normalizer("macenko")
    norm.fit(big)
    ref = ostain.get_normalizer("macenko")
    ref.fit(big.copy())
    np.testing.assert_allclose(norm.stain_matrix_target, ref.stain_matrix_target, atol=STAT_TOL)
    np.testing.assert_allclose(norm.maxC_target, ref.maxC_target, atol=STAT_TOL)


def test_stain_augmentor_matches_reference_golden(gold):
    """StainAugmentor.fit/augment with injected (alpha, beta) vs the real reference's output."""
    from tiatoolbox_amd.tools.stainaugment import StainAugmentor

    crops = gold["real_crops"]
    for k, ab in enumerate(gold["augment_ab"]):
        aug = StainAugmentor(method="macenko", augment_background=bool(k))
        aug.fit(crops[k], threshold=0.85)
        out = aug.augment(alpha_beta=ab)
        _u8_close(out, gold["augment_real"][k])
        assert out.shape == crops[k].shape and out.dtype == np.uint8
    with pytest.raises(ValueError, match="Unsupported stain extractor method"):
        StainAugmentor(method="reinhard")
    # sigma = 0 => alpha = 1, beta = 0: equals recomposition of the source concentrations
    aug = StainAugmentor(method="macenko", sigma1=0.0, sigma2=0.0, always_apply=True)
    res = aug(image=crops[0])["image"]
    exp = ostain.stain_augment(crops[0], ostain.MacenkoExtractor().get_stain_matrix(crops[0].copy()),
                               np.ones(2), np.zeros(2))
    _u8_close(res, exp)
    assert aug.source_concentrations.shape == (128 * 128, 2) and aug.tissue_mask.shape == (128 * 128,)


def test_stain_augmentor_table_form_and_its_fallback(gold):
    """The float64 augmentation as a product of per-patch tables (whole 3072-byte chunks) agrees with the oracle for ordinary and for
    extreme (alpha, beta); exponents beyond the tables' safe range run the reference's per-pixel arithmetic inside the same kernel."""
    from tiatoolbox_amd.tools.stainaugment import StainAugmentor

    crop = gold["real_crops"][0]            # 128 x 128: 16 chunks
    sm = ostain.MacenkoExtractor().get_stain_matrix(crop.copy())
    for ab, bg in (((1.3, 0.7, 0.05, -0.02), False), ((0.6, 1.4, -0.03, 0.04), True), ((40.0, 0.02, 2.0, -1.5), False),
                   ((900.0, 700.0, 0.0, 0.0), True)):   # the last one: |m| >> 18 -> the libm fall-back
        aug = StainAugmentor(method="macenko", augment_background=bg)
        aug.fit(crop, threshold=0.85)
        out = aug.augment(alpha_beta=np.array(ab))
        exp = ostain.stain_augment(crop, sm, np.array(ab[:2]), np.array(ab[2:]), augment_background=bg)
        _u8_close(out, exp, max_rate=5e-4)


def test_stain_augmentor_f32_fast_path(gold, he_patches):
    """precision='f32' (16-byte-access kernel): within one grey level of the float64 path on < 1e-3 of the
    bytes, for tissue-only and background-included augmentation, batched device input."""
    import torch

    from tiatoolbox_amd.tools.stainaugment import StainAugmentor

    crops = gold["real_crops"]              # 128x128: 128*128*3 % 3072 == 0
    for k, ab in enumerate(gold["augment_ab"]):
        aug = StainAugmentor(method="macenko", augment_background=bool(k), precision="f32")
        aug.fit(crops[k], threshold=0.85)
        assert aug._fast_path_ok()  # noqa: SLF001
        _u8_close(aug.augment(alpha_beta=ab), gold["augment_real"][k], max_rate=1e-3)
    odd = StainAugmentor(method="macenko", precision="f32")
    odd.fit(he_patches[0][:50, :50], threshold=0.85)      # 50*50*3 is not a chunk multiple: f64 kernel
    assert not odd._fast_path_ok()  # noqa: SLF001
    res = odd.augment(alpha_beta=np.array([1.1, 0.9, 0.01, -0.01]))
    assert res.shape == (50, 50, 3) and res.dtype == np.uint8
    sm = ostain.MacenkoExtractor().get_stain_matrix(he_patches[0][:50, :50].copy())
    _u8_close(res, ostain.stain_augment(he_patches[0][:50, :50], sm, np.array([1.1, 0.9]), np.array([0.01, -0.01])))
    with pytest.raises(ValueError, match="precision"):
        StainAugmentor(precision="f16")
    del torch


@pytest.mark.gpu
def test_vahadane_dictionary_learning_on_device_matches_sklearn(he_patches, target_image):
    """``TIA_MODE_VAHADANE`` (dictionary learning restated in the HIP kernel) against scikit-learn's
    ``DictionaryLearning`` driven exactly as the reference drives it (stainextract.py:305-316; the oracle's
    ``VahadaneExtractor`` -- ``random_state`` only matters for never-used atoms, which these inputs do not have):
    stain matrices to 1e-6 (measured ~1e-12), whole batches in one launch, then fit/transform to <= 1 LSB."""
    from tiatoolbox_amd.tools.stainextract import VahadaneExtractor
    from tiatoolbox_amd.tools.stainnorm import get_normalizer
    from tiatoolbox_amd.utils import synth

    ref_ex = ostain.VahadaneExtractor(random_state=0)
    ex = VahadaneExtractor()
    worst = 0.0
    for batch in (he_patches[:4], synth.g_he(3, 64, 64, seed=21), synth.g_he(2, 224, 224, seed=22),
                  synth.g_he(2, 37, 41, seed=23), target_image[None]):
        got = ex.get_stain_matrix(batch)
        assert got.shape == (len(batch), 2, 3)
        for i, img in enumerate(batch):
            exp = ref_ex.get_stain_matrix(img.copy())
            worst = max(worst, float(np.abs(got[i] - exp).max()))
    assert worst <= 1e-6, worst
    single = ex.get_stain_matrix(he_patches[0])
    assert single.shape == (2, 3) and np.array_equal(single, ex.get_stain_matrix(he_patches[:1])[0])
    # deterministic, and independent of how the batch is split
    a = ex.get_stain_matrix(he_patches[:6])
    b = np.concatenate([ex.get_stain_matrix(he_patches[:2]), ex.get_stain_matrix(he_patches[2:6])])
    assert np.array_equal(a, b)

    norm = get_normalizer("vahadane")
    norm.fit(target_image)
    ref = ostain.get_normalizer("vahadane")
    ref.fit(target_image.copy())
    np.testing.assert_allclose(norm.stain_matrix_target, ref.stain_matrix_target, atol=1e-6)
    np.testing.assert_allclose(norm.maxC_target, ref.maxC_target, rtol=1e-6)
    out = norm.transform(he_patches[:3])
    for i in range(3):
        exp = ref.transform(he_patches[i].copy())
        diff = np.abs(out[i].astype(int) - exp.astype(int))
        assert diff.max() <= 1 and (diff != 0).mean() < 2e-3, (i, diff.max(), (diff != 0).mean())
    white = np.full((1, 32, 32, 3), 255, np.uint8)
    with pytest.raises(ValueError, match="Empty tissue mask"):
        ex.get_stain_matrix(white)


@pytest.mark.gpu
def test_window_selection_equals_histogram_selection(he_patches, target_image):
    """The order statistics (angular percentiles, 99th-percentile concentrations) come from sample-placed windows swept
    in float32 with exact float64 candidates; the multi-level histogram selection is the fall-back.  Both are exact
    selections of the same float64 keys, so every statistic must be BIT-identical between ``select_mode`` 0 and 1 --
    on realistic patches, uniform noise (flat key distributions), tiny / odd-sized patches (sample too small, per-pixel
    path), saturated patches (massive ties), a large image (no mask-bit cache) and every extractor mode."""
    import torch

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import _stain_device as dev
    from tiatoolbox_amd.utils import synth

    rng = np.random.default_rng(8)
    flat = np.full((2, 64, 64, 3), 120, np.uint8)
    flat[:, ::2, ::3] = 60
    flat[1, :32] = rng.integers(0, 256, (32, 64, 3))
    steps = (np.clip(synth.g_he(3, 128, 128, seed=31).astype(int) // 32 * 32 + 16, 0, 255)).astype(np.uint8)  # heavy ties
    big = np.ascontiguousarray(np.tile(target_image, (3, 3, 1))[:700, :650])
    batches = [he_patches, synth.g_he(48, 224, 224, seed=30), synth.g_uniform(8, 256, 256, seed=2), steps, flat,
               synth.g_he(3, 37, 41, seed=32), synth.g_he(2, 16, 16, seed=33), big[None],
               np.ascontiguousarray(synth.g_he(1, 1000, 1000, seed=34))]
    target = np.array([[0.55, 0.76, 0.35], [0.1, 0.96, 0.27]])
    modes = {"macenko": {"mode": _lib.MODE_MACENKO}, "fixed": {"mode": _lib.MODE_FIXED, "stain_fixed": target},
             "vahadane": {"mode": _lib.MODE_VAHADANE}}
    checked = 0
    for batch in batches:
        x = torch.from_numpy(batch).cuda()
        for name, kw in modes.items():
            if name == "vahadane" and batch.shape[1] > 300:
                continue
            a = dev.stain_stats(x, dev.make_params(select_mode=0, target_stain=target, target_maxc=np.array([[1.9, 1.0]]), **kw))
            a = a.cpu().numpy()[:, :_lib.ST_CYCLES]
            for other in (1, 2):  # histogram selection; window selection on the streaming kernel
                b = dev.stain_stats(x, dev.make_params(select_mode=other, target_stain=target, target_maxc=np.array([[1.9, 1.0]]), **kw))
                b = b.cpu().numpy()[:, :_lib.ST_CYCLES]
                if batch.shape[1] * batch.shape[2] > 4 * 256 * 256 and name != "vahadane":
                    # large images: select_mode 0 is the multi-workgroup path (stain_stats_big.hip), whose float64 moment sums are
                    # merged in another order than the one-workgroup kernels' -- agreement to rounding, not bit for bit (the exact
                    # order statistics themselves are selected on keys that differ in the last ulp)
                    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-10, err_msg=f"{name} {other} {batch.shape}")
                    continue
                same = (a == b) | (np.isnan(a) & np.isnan(b))
                assert same.all(), (name, other, batch.shape, np.argwhere(~same)[:5], a[~same][:5], b[~same][:5])
            checked += a.shape[0]
    assert checked > 150


@pytest.mark.gpu
def test_headline_size_batch_against_oracle(target_image):
    """BASELINE configs[1] size (4096 x 224 x 224 in ONE launch sequence) checked against the oracle itself, not only
    for self-consistency: 32 of the 4096 patches (spread over the batch, every one with different content) -- stain
    matrices / maxC to 1e-9, normalised pixels within 1 LSB, float64 pre-cast values to 1e-4 (north-star tolerance)."""
    import torch

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools.stainnorm import get_normalizer
    from tiatoolbox_amd.utils import synth

    uniq = synth.g_he(512, 224, 224, seed=77)
    batch = torch.from_numpy(uniq).cuda().repeat(8, 1, 1, 1)
    pick = np.linspace(0, 4095, 32).astype(int)
    # make the picked patches unique in content and position: roll each one by its index
    for i in pick:
        batch[i] = torch.roll(batch[i], shifts=int(i) % 224, dims=1)
    norm = get_normalizer("macenko")
    norm.fit(target_image)
    out, stats = norm.transform(batch, return_stats=True)
    pre = norm.transform(batch, out="float64")
    ref = ostain.get_normalizer("macenko")
    ref.fit(target_image.copy())
    host = batch[torch.from_numpy(pick).cuda()].cpu().numpy()
    stats_h = stats.cpu().numpy()
    out_h, pre_h = out[torch.from_numpy(pick).cuda()].cpu().numpy(), pre[torch.from_numpy(pick).cuda()].cpu().numpy()
    for j, i in enumerate(pick):
        exp_sm = ref.extractor.get_stain_matrix(host[j].copy())
        np.testing.assert_allclose(stats_h[i, _lib.ST_STAIN:_lib.ST_STAIN + 6].reshape(2, 3), exp_sm, atol=1e-9)
        exp_pre = ref.transform_float(host[j].copy())
        assert np.abs(pre_h[j] - exp_pre).max() <= FLOAT_TOL, (i, np.abs(pre_h[j] - exp_pre).max())
        diff = np.abs(out_h[j].astype(int) - exp_pre.astype(np.uint8).astype(int))
        assert diff.max() <= 1 and (diff != 0).mean() < 2e-4, (i, diff.max(), (diff != 0).mean())


@pytest.mark.gpu
def test_metric_size_batch_against_oracle(target_image):
    """J1 -- BASELINE.json's metric configuration: 4096 x 256 x 256 patches in ONE launch sequence (the shape ``bench.py`` times;
    restates ``tools/stainnorm.py:89-113`` + ``tools/stainextract.py:177-227`` per patch), checked against the oracle on 32
    patches spread over the batch, each with content no other patch has.  At 256^2 the statistics come from the
    REGISTER-RESIDENT kernel (one HBM read of the patch; since round 4 for every patch of at most 256^2), with at most 1 % of
    the patches handed back, and the streaming kernel is run on the same batch for bit-identity.  Stain
    matrix / maxC to 1e-9, float64 pre-cast pixels to 1e-4 (north-star tolerance), uint8 within 1 LSB on < 2e-4 of the bytes."""
    import ctypes

    import torch

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import _stain_device as dev
    from tiatoolbox_amd.tools.stainnorm import get_normalizer
    from tiatoolbox_amd.utils import synth

    n, side = 4096, 256
    uniq = synth.g_he(256, side, side, seed=91)
    batch = torch.from_numpy(uniq).cuda().repeat(n // 256, 1, 1, 1)
    pick = np.unique(np.concatenate([np.linspace(0, n - 1, 30).astype(int), [1023, 1024]]))   # micro-batch seams included
    for i in pick:   # unique content and position: roll rows by the index, columns by a second stride
        batch[i] = torch.roll(batch[i], shifts=(int(i) % side, (7 * int(i)) % side), dims=(0, 1))
    norm = get_normalizer("macenko")
    norm.fit(target_image)
    out, stats = norm.transform(batch, return_stats=True)
    prm = norm.extractor.stats_params(target_stain=norm.stain_matrix_target, target_maxc=norm.maxC_target)
    lib = _lib.load()
    assert lib.tia_stain_stats_path(side, side, ctypes.byref(prm)) == 1, "256^2 patches: the register-resident kernel"
    assert lib.tia_stain_stats_path(257, 256, ctypes.byref(prm)) == 0    # (does not fit 16 groups per thread: streaming)
    handed_back = dev.redo_count(batch.device, n, side, side)
    assert 0 <= handed_back <= n // 100, f"hand-backs to the streaming kernel: {handed_back} of {n}"
    # the same batch through the streaming kernel (window selection, select_mode 2): bit-identical statistics
    prm.select_mode = 2
    assert lib.tia_stain_stats_path(side, side, ctypes.byref(prm)) == 0
    stats_stream = dev.stain_stats(batch, prm)
    assert torch.equal(stats[:, :_lib.ST_CYCLES], stats_stream[:, :_lib.ST_CYCLES])
    pre = norm.transform(batch, out="float64")
    ref = ostain.get_normalizer("macenko")
    ref.fit(target_image.copy())
    idx = torch.from_numpy(pick).cuda()
    host, stats_h = batch[idx].cpu().numpy(), stats.cpu().numpy()
    out_h, pre_h = out[idx].cpu().numpy(), pre[idx].cpu().numpy()
    assert not stats_h[:, _lib.ST_FLAGS].any()
    worst = 0.0
    for j, i in enumerate(pick):
        exp_sm = ref.extractor.get_stain_matrix(host[j].copy())
        np.testing.assert_allclose(stats_h[i, _lib.ST_STAIN:_lib.ST_STAIN + 6].reshape(2, 3), exp_sm, atol=STAT_TOL)
        conc = ostain.StainNormalizer.get_concentrations(host[j].copy(), exp_sm)
        np.testing.assert_allclose(stats_h[i, _lib.ST_MAXC:_lib.ST_MAXC + 2], np.percentile(conc, 99, axis=0), atol=STAT_TOL)
        exp_pre = ref.transform_float(host[j].copy())
        err = float(np.abs(pre_h[j] - exp_pre).max())
        worst = max(worst, err)
        assert err <= FLOAT_TOL, (i, err)
        diff = np.abs(out_h[j].astype(int) - exp_pre.astype(np.uint8).astype(int))
        assert diff.max() <= 1 and (diff != 0).mean() < 2e-4, (i, diff.max(), (diff != 0).mean())
    # the repeated (un-rolled) patches must reproduce their first occurrence bit for bit, wherever they sit in the batch
    rest = np.setdiff1d(np.arange(n), pick)
    first = {int(i) % 256: int(i) for i in rest[::-1]}
    sample = rest[:: max(1, len(rest) // 64)]
    for i in sample:
        assert torch.equal(out[int(i)], out[first[int(i) % 256]])
    print(f"[metric size] worst pre-cast error {worst:.3e} over {len(pick)} patches")


@pytest.mark.gpu
def test_rgb2od_standalone_kernel_and_side_effect(uniform_patches):
    """a1 -- ``utils/transforms.py:209-231`` through ``tia_rgb2od_u8``: values equal the oracle's float64 (same NumPy log on the
    256 possible bytes => bit-identical), and the reference's side effect ``img[img == 0] = 1`` happens in the caller's array
    (NumPy) / tensor (CUDA), for HWC images, NHWC batches, flat (N, 3) arrays and odd byte counts."""
    import torch

    from tiatoolbox_amd.utils.transforms import rgb2od

    rng = np.random.default_rng(3)
    cases = [uniform_patches[0].copy(), uniform_patches.copy(), rng.integers(0, 4, (1001, 3), dtype=np.uint8),
             rng.integers(0, 3, (7,), dtype=np.uint8), np.zeros((5, 5, 3), np.uint8)]
    for arr in cases:
        arr.flat[arr.size // 2] = 0
        mine, theirs = arr.copy(), arr.copy()
        assert (mine == 0).any()
        exp = ostain.rgb2od(theirs)                      # mutates ``theirs``
        got = rgb2od(mine)                               # must mutate ``mine`` identically
        assert got.dtype == np.float64 and got.shape == arr.shape
        assert np.array_equal(got, exp)
        assert np.array_equal(mine, theirs) and not (mine == 0).any()
        keep = arr.copy()
        assert np.array_equal(rgb2od(keep, mutate=False), exp) and np.array_equal(keep, arr)
    t = torch.from_numpy(uniform_patches.copy()).cuda()
    theirs = uniform_patches.copy()
    exp = ostain.rgb2od(theirs)
    got = rgb2od(t)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), exp) and np.array_equal(t.cpu().numpy(), theirs)
    view = torch.from_numpy(uniform_patches.copy()).cuda()[:, ::2]          # non-contiguous view: the edit is handed back
    theirs = uniform_patches.copy()[:, ::2]
    exp = ostain.rgb2od(theirs)
    assert np.array_equal(rgb2od(view).cpu().numpy(), exp) and np.array_equal(view.cpu().numpy(), theirs)
    ro = uniform_patches[0].copy()
    ro.setflags(write=False)                                                   # read-only input: values only
    assert np.array_equal(rgb2od(ro), ostain.rgb2od(uniform_patches[0].copy()))
    # other dtypes keep the reference's semantics (log of the values as they are, 0 -> 1 in place): float RGB, integer arrays, lists
    f32 = uniform_patches[0].astype(np.float32)
    theirs = f32.copy()
    exp = ostain.rgb2od(theirs)
    got = rgb2od(f32)
    # (NumPy's float32 log of x / 255 near 1 carries the cancellation's error: compare absolutely)
    assert got.dtype == exp.dtype and np.allclose(got, exp, rtol=1e-6, atol=4e-7) and np.array_equal(f32, theirs)
    i64 = uniform_patches[0][:8, :8].astype(np.int64)
    assert np.allclose(rgb2od(i64.copy()), ostain.rgb2od(i64.copy()), rtol=1e-14, atol=0)
    assert np.allclose(rgb2od(i64.tolist()), ostain.rgb2od(i64.copy()), rtol=1e-14, atol=0)
    tf = torch.from_numpy(uniform_patches[0].copy()).cuda().float()
    assert np.allclose(rgb2od(tf).cpu().numpy(), exp, rtol=1e-6, atol=4e-7) and int((tf == 0).sum()) == 0
    with pytest.raises(TypeError, match="numeric"):
        rgb2od(np.array([["a"]]))


@pytest.mark.gpu
def test_f64_table_exp_against_libm_exp(he_patches, uniform_patches, target_image):
    """``TIA_MATH_F64`` evaluates ``255 exp(-t)`` with the kernel's own table + cubic; ``TIA_MATH_F64_REF`` keeps the reference's
    order of operations and the device library's ``exp``.  Float64 outputs must agree to 1e-10 on the 0..255 scale (bound:
    4e-15 relative), uint8 outputs may differ only where the float sits within that distance of an integer -- i.e. essentially
    never -- on H&E-like and on uniform-noise input (every byte value), through the 12-byte AND the 16-byte-access kernels.
    A patch whose fused matrix is far outside the safe exponent range takes the in-kernel libm fall-back: identical to REF."""
    import torch

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import _stain_device as dev
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    norm = get_normalizer("macenko")
    norm.fit(target_image)
    for batch_np in (he_patches, np.ascontiguousarray(uniform_patches), he_patches[:, :50, :50].copy()):
        x = torch.from_numpy(batch_np).cuda()
        p = norm.extractor.stats_params(target_stain=norm.stain_matrix_target, target_maxc=norm.maxC_target)
        stats = dev.stain_stats(x, p)
        a = dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=_lib.OUT_F64, math=_lib.MATH_F64)
        b = dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=_lib.OUT_F64, math=_lib.MATH_F64_REF)
        assert float((a - b).abs().max()) <= 1e-10, float((a - b).abs().max())
        for kind in (_lib.OUT_U8, _lib.OUT_UNIT_F16):
            ua = dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=kind, math=_lib.MATH_F64)
            ub = dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=kind, math=_lib.MATH_F64_REF)
            assert float((ua != ub).float().mean()) <= 1e-6
        assert torch.equal(b.clamp(0, 255).to(torch.uint8),
                           dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=_lib.OUT_U8, math=_lib.MATH_F64_REF))
    # unsafe exponent range -> in-kernel fall-back (the statistics record is edited on purpose)
    x = torch.from_numpy(he_patches[:2]).cuda()
    p = norm.extractor.stats_params(target_stain=norm.stain_matrix_target, target_maxc=norm.maxC_target)
    stats = dev.stain_stats(x, p)
    stats[1, _lib.ST_M:_lib.ST_M + 9] *= 1e6
    stats[1, _lib.ST_SCALE:_lib.ST_SCALE + 2] *= 1e6
    for kind in (_lib.OUT_U8, _lib.OUT_F64):
        ua = dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=kind, math=_lib.MATH_F64)
        ub = dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=kind, math=_lib.MATH_F64_REF)
        assert torch.equal(ua[1], ub[1])
        assert float((ua[0].double() - ub[0].double()).abs().max()) <= 1e-10
    # non-finite entries take the fall-back too (same bits as REF, NaN for NaN); entries just inside the table form's range
    # (|m| < 126: factors down to exp(-700)) still agree to 1e-10
    for val, exact in ((float("nan"), True), (float("inf"), True), (-float("inf"), True), (125.0, False), (-125.0, False)):
        stats = dev.stain_stats(x, p)
        stats[1, _lib.ST_M + 4] = val
        ua = dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=_lib.OUT_F64, math=_lib.MATH_F64)
        ub = dev.stain_apply(x, stats, norm.stain_matrix_target, out_kind=_lib.OUT_F64, math=_lib.MATH_F64_REF)
        if exact:
            assert bool(((ua[1] == ub[1]) | (ua[1].isnan() & ub[1].isnan())).all()), val
        else:
            assert float((ua[1] - ub[1]).abs().max()) <= 1e-10, val
        assert float((ua[0] - ub[0]).abs().max()) <= 1e-10


@pytest.mark.gpu
def test_refused_host_register_does_not_poison_the_next_launch(he_patches):
    """A host-side HIP call that is refused (``hipHostRegister`` of mmap'd / foreign memory in ``_HostFeed``; here:
    ``hipHostUnregister`` of memory that was never registered) leaves the runtime's sticky last-error set; every ``tia_*`` entry point reports ``hipGetLastError() != hipSuccess`` as ``TIA_ELAUNCH``.
    ``tia_clear_last_error`` (same runtime instance as the kernels' checks) is what ``_HostFeed`` calls after a refusal."""
    import torch

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.engine import engine_abc
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    lib = _lib.load()
    lib.tia_clear_last_error()
    arr = np.ascontiguousarray(he_patches[:2])
    rt = torch.cuda.cudart()
    # a refusal that every ROCm release reports: un-registering memory that was never registered (registering the same range
    # twice is accepted by ROCm 7's runtime, so that cannot serve as the refusal here)
    rc = int(rt.cudaHostUnregister(arr.ctypes.data))
    assert rc != 0
    try:
        assert engine_abc._clear_last_hip_error() != 0, "the refusal must be pending in the library's runtime instance"  # noqa: SLF001
        assert lib.tia_clear_last_error() == 0, "... and consumed by the helper"
        rc = int(rt.cudaHostUnregister(arr.ctypes.data))      # pending again
        assert rc != 0
        engine_abc._clear_last_hip_error()  # noqa: SLF001
        norm = get_normalizer("ruifrok")
        norm.fit(he_patches[0])
        assert norm.transform(arr).shape == arr.shape                     # would raise HipLibraryError(TIA_ELAUNCH) otherwise
    finally:
        lib.tia_clear_last_error()


@pytest.mark.gpu
def test_vahadane_kernel_pair_equals_one_kernel_form(he_patches, target_image):
    """Default Vahadane statistics = two kernels: dictionary learning that REPLAYS a pixel's atom updates from per-iteration
    scalars (no 2 x N dictionary in memory; divisions by those scalars through Markstein's reciprocal sequence), then the common
    tail.  ``dl_one_kernel=True`` keeps the dictionary in the workspace (plain divisions).  Same arithmetic on the same values in
    the same order: every statistic must be BIT-identical -- H&E-like patches, uniform noise (an atom can become unused: the
    hand-back path), odd sizes, a large image, several regularisers, a white patch (empty mask), and more iterations than the
    replay records (handed back as a whole)."""
    import torch

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import _stain_device as dev

    target = np.array([[0.55, 0.76, 0.35], [0.1, 0.96, 0.27]])
    mixed = he_patches.copy()
    mixed[3] = 255
    batches = [mixed, synth.g_he(6, 224, 224, seed=40), synth.g_uniform(4, 128, 128, seed=6), synth.g_he(3, 37, 41, seed=41),
               np.ascontiguousarray(np.tile(target_image, (2, 2, 1))[None, :500, :470])]
    checked = 0
    for batch in batches:
        x = torch.from_numpy(batch).cuda()
        for alpha in (0.1, 0.02, 0.6, 5.0):
            for iters in (3, 2, 1, 6):
                kw = {"mode": _lib.MODE_VAHADANE, "dl_alpha": alpha, "dl_max_iter": iters, "target_stain": target,
                      "target_maxc": np.array([[1.9, 1.0]])}
                a = dev.stain_stats(x, dev.make_params(**kw)).cpu().numpy()[:, :_lib.ST_CYCLES]
                b = dev.stain_stats(x, dev.make_params(dl_one_kernel=True, **kw)).cpu().numpy()[:, :_lib.ST_CYCLES]
                same = (a == b) | (np.isnan(a) & np.isnan(b))
                assert same.all(), (batch.shape, alpha, iters, np.argwhere(~same)[:5], a[~same][:5], b[~same][:5])
                checked += a.shape[0]
    assert checked >= 300

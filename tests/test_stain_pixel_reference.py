"""Every route of the per-pixel stain kernels of ``csrc/stain_apply.hip`` -- normalisation, concentrations, augmentation, luminosity
mask -- against the mathematical per-pixel function in ``np.longdouble`` (``tests/_stain_pixel_ref.py``).  The statistics records are
built on the host, so that a kernel's value is checked on its own: not through fit + statistics kernel + apply.

Comparison rule: with the per-pixel tolerance ``tol`` a float output lies in [clip(T - tol), clip(T + tol)], a byte in
[floor(clip(T - tol)), floor(clip(T + tol))]; every byte is within 1 of floor(clip(T)) and the rate of those that differ stays within
2e-4 (float64 maths) / 2e-3 (float32 maths).  ``tol`` is 1e-10 max(1, A) for the float64 modes (A: the absolute sum of the exponent's
terms) and twice a first-order bound for ``TIA_MATH_F32``.  A byte whose window holds two values is ambiguous; the host tests cap the
ambiguous share of every input the GPU tests use (2e-4 / 5e-3), from the truth alone.

The tests without the ``gpu`` mark check the helper on the host: the truth against the oracle on fitted inputs, the conditions on the
inputs, the float32 bounds against a NumPy float32 emulation, and that the case lists reach every route (restated launch conditions).
Each GPU test prints its largest error / tol (float outputs) and byte mismatch rates; ``profiles/stain_pixel_reference.txt`` holds them."""

from __future__ import annotations

import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _stain_pixel_ref as R  # noqa: E402, N812

from oracle import stain as ostain  # noqa: E402
from tiatoolbox_amd.utils import cvtables  # noqa: E402

MATHS = {"f64": R.MATH_F64, "f32": R.MATH_F32, "f64ref": R.MATH_F64_REF}
OUTS = {"u8": R.OUT_U8, "f32": R.OUT_F32, "f64": R.OUT_F64, "unit_f16": R.OUT_UNIT_F16, "unit_bf16": R.OUT_UNIT_BF16,
        "unit_f32": R.OUT_UNIT_F32}
ITEMSIZE = {R.OUT_U8: 1, R.OUT_F32: 4, R.OUT_F64: 8, R.OUT_UNIT_F16: 2, R.OUT_UNIT_BF16: 2, R.OUT_UNIT_F32: 4}
Y085, Y080 = cvtables.y_threshold(0.85), cvtables.y_threshold(0.8)
# (input byte offset, output byte offset) of the views of test 2; the odd ones need the alignment test of sweep12 / store12
OFFSETS_U8 = [(4, 4), (8, 8), (4, 0), (1, 1), (3, 3), (0, 3), (1, 0)]
OFFSETS_WIDE_OUT = {R.OUT_F32: [(4, 4), (8, 8)], R.OUT_F64: [(4, 8)], R.OUT_UNIT_F16: [(4, 4), (8, 8), (1, 2)], R.OUT_UNIT_BF16: [(8, 8)],
                    R.OUT_UNIT_F32: [(4, 4), (3, 8)]}
ALIGN_SHAPES = [(64, 80), (50, 50)]
AUG_F64 = [((64, 80), 0), ((50, 50), 0), ((37, 41), 0), ((64, 80), 4), ((64, 80), 1)]     # (shape, input byte offset)
AUG_F32 = [((32, 32), 0), ((64, 80), 0)]
MASK_CASES = [((64, 80), 0), ((32, 32), 0), ((50, 50), 0), ((37, 41), 0), ((64, 80), 4), ((64, 80), 1), ((1, 1), 0), ((1, 4), 0), ((3, 1), 0)]

_TRUTH: dict = {}


def _apply_truth(shape):
    """(images, T, A, float32 bound B) of one shape: computed once, shared, read only."""
    key = ("apply", shape)
    if key not in _TRUTH:
        d = R.inputs()
        img = R.crop(d["imgs"], shape)
        t, a = R.apply_truth(img, d["recs"], d["target"])
        _TRUTH[key] = (img, t, a, R.bound_f32_apply(img, d["recs"], t))
    return _TRUTH[key]


def _augment_truth(shape, extreme, bg, z1):
    key = ("augment", shape, extreme, bg, z1)
    if key not in _TRUTH:
        img, recs, ab = R.crop(R.inputs()["imgs"], shape), R.augment_records(), R.augment_ab(extreme)
        t, a, sel = R.augment_truth(img, recs, ab, Y085, augment_background=bg, zero_to_one=z1)
        _TRUTH[key] = (img, ab, t, a, sel, R.bound_f32_augment(img, recs, ab, sel, t))
    return _TRUTH[key]


def _apply_tol(math, out_kind, t, a, b):
    return 2 * b if math == R.MATH_F32 else R.tol_f64(t, a, out_kind)


def _not_f():
    """The patches that are compared through a window: the M = 0 record is compared exactly."""
    return [k != "f" for k in R.inputs()["kinds"]]


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
def test_helper_constants_and_precision():
    from tiatoolbox_amd import _lib

    R.require_longdouble()
    for name in ("ST_STAIN", "ST_PLOW", "ST_PHIGH", "ST_PINV", "ST_M", "ST_SCALE", "MATH_F64", "MATH_F32", "MATH_F64_REF", "OUT_U8", "OUT_F32",
                 "OUT_F64", "OUT_UNIT_F16", "OUT_UNIT_BF16", "OUT_UNIT_F32"):
        assert getattr(R, name) == getattr(_lib, name), name
    assert _lib.TIA_STATS_STRIDE == R.STRIDE
    assert "torch" not in R.__dict__


def test_truth_matches_the_oracle_on_fitted_inputs():
    """Records fitted on the image they normalise: the clipped truth is ``transform_float`` (lstsq against pinv, np.dot against the
    longdouble sum: 1e-9 is generous), and the augment truth gives ``stain_augment``'s bytes."""
    d = R.inputs()
    ref = ostain.get_normalizer("macenko")
    ref.fit(d["target_img"].copy())
    np.testing.assert_array_equal(ref.stain_matrix_target, d["target"])
    he = d["he"]
    recs = np.stack([R.make_record(s, d["maxc_t"] / maxc, d["target"], *R.percentiles(p)) for (s, maxc), p in zip(d["fits"], he)])
    t, a = R.apply_truth(he, recs, d["target"])
    exp = np.stack([ref.transform_float(p.copy()) for p in he])
    err = np.abs(np.clip(t, 0, 255) - exp).max()
    assert err <= 1e-9, err  # noqa: PLR2004
    assert a.max() < 100 and a.min() > 0  # noqa: PLR2004
    for (al0, al1, be0, be1), bg in itertools.product(R.AB_ORDINARY + R.AB_EXTREME, (False, True)):
        ab = np.tile([al0, al1, be0, be1], (4, 1))
        t, a, _ = R.augment_truth(he, recs, ab, Y085, augment_background=bg, zero_to_one=True)
        exp = np.stack([ostain.stain_augment(p, s, np.array([al0, al1]), np.array([be0, be1]), augment_background=bg)
                        for p, (s, _) in zip(he, d["fits"])])
        R.check_u8(exp, t, R.tol_f64(t, a), R.MATH_F64, f"oracle augment {al0, al1, be0, be1} bg={bg}")


def test_records_take_the_forms_they_are_meant_for():
    d = R.inputs()
    forms = {k: R.apply_form(r) for k, r in zip(d["kinds"], d["recs"])}
    assert forms["a"] == forms["b"] == forms["e"] == forms["f"] == {"trick": True, "table": True}
    assert forms["c"] == {"trick": False, "table": True} and forms["d"] == {"trick": False, "table": False}
    assert d["kinds"][:4] == ["a", "c", "d", "f"]                       # neighbours in one batch take different forms
    m = {k: np.abs(r[R.ST_M:R.ST_M + 9]).reshape(3, 3) for k, r in zip(d["kinds"], d["recs"])}
    assert m["b"].max() == pytest.approx(20.0) and m["d"].min() > 126 and m["c"].max() < 126  # noqa: PLR2004
    assert (m["c"].sum(0) > 64.04).sum() >= 2 and m["c"].sum(0).max() < 126 and not m["f"].any()  # noqa: PLR2004
    me = d["recs"][d["kinds"].index("e")][R.ST_M:R.ST_M + 9]
    assert (me > 0).any() and (me < 0).any()
    recs = R.augment_records()
    assert [R.augment_tables_ok(r, ab) for r, ab in zip(recs, R.augment_ab(True))] == [True, False] * 4   # table and libm patches alternate
    assert all(R.augment_tables_ok(r, ab) for r, ab in zip(recs, R.augment_ab(False)))
    imgs = d["imgs"]
    assert (imgs[6] == 255).all() and not imgs[7].any() and len(np.unique(imgs[1])) == 256 and (imgs[1] == 0).any()  # noqa: PLR2004


def test_case_lists_reach_every_route():
    """The launch conditions restated: which kernel each (shape, type, offset) of the GPU tests reaches."""
    hw = {s: s[0] * s[1] for s in R.SHAPES}
    reach = {(m, R.apply_route(m, o, hw[s])) for m in MATHS.values() for o in OUTS.values() for s in R.SHAPES}
    assert reach == {(R.MATH_F64, "wide"), (R.MATH_F32, "wide")} | {(m, r) for m in MATHS.values() for r in ("groups12", "scalar")}
    for m in (R.MATH_F64, R.MATH_F32):
        assert {o for o in OUTS.values() if R.apply_route(m, o, 5120) == "wide"} == {R.OUT_U8, R.OUT_UNIT_F16, R.OUT_UNIT_BF16}
        # the float and float64 outputs and OUT_UNIT_F32 take 12-byte groups and the scalar loop outside the 16-byte route
        assert {R.apply_route(m, o, hw[s]) for o in (R.OUT_F32, R.OUT_F64, R.OUT_UNIT_F32) for s in R.SHAPES} == {"groups12", "scalar"}
    assert [R.apply_route(R.MATH_F64, R.OUT_U8, hw[s]) for s in R.SHAPES] == ["wide", "wide", "groups12", "scalar", "scalar", "groups12", "scalar"]
    # test 2: a 4- or 8-byte offset leaves the 16-byte route for the 12-byte groups; an odd one, or an output that is not aligned
    # for store12's 8- and 16-byte forms, takes the scalar loop
    u8 = [R.apply_route(R.MATH_F32, R.OUT_U8, 5120, img_off=i, out_off=o) for i, o in OFFSETS_U8]
    assert u8 == ["groups12", "groups12", "groups12", "scalar", "scalar", "scalar", "scalar"]
    wide = {k: [R.apply_route(R.MATH_F32, k, 2500, img_off=i, out_off=o) for i, o in v] for k, v in OFFSETS_WIDE_OUT.items()}
    assert wide == {R.OUT_F32: ["scalar", "scalar"], R.OUT_F64: ["scalar"], R.OUT_UNIT_F16: ["scalar", "groups12", "scalar"],
                    R.OUT_UNIT_BF16: ["groups12"], R.OUT_UNIT_F32: ["scalar", "scalar"]}
    assert [R.augment_route(R.MATH_F64, s[0] * s[1], off=o) for s, o in AUG_F64] == ["f64_wide_pair", "per_pixel", "per_pixel", "per_pixel", "per_pixel"]
    assert [R.augment_route(R.MATH_F32, s[0] * s[1], off=o) for s, o in AUG_F32] == ["f32_wide"] * 2
    assert R.augment_route(R.MATH_F32, 2500) == R.augment_route(R.MATH_F32, 5120, off=4) == "ESIZE"
    assert [R.mask_route(s[0] * s[1], off=o) for s, o in MASK_CASES] == ["wide", "wide", "dword", "scalar", "dword", "scalar", "scalar", "dword", "scalar"]


def test_inputs_meet_the_ambiguity_and_clip_conditions():
    """Conditions on the inputs, from the truth alone: the share of bytes whose window holds two values is capped for every
    (image, record, alpha/beta) of the GPU tests, and the ordinary records clip under 15 % of the values of a patch."""
    d = R.inputs()
    worst = {"apply f64": 0.0, "apply f32": 0.0, "augment f64": 0.0, "augment f32": 0.0}
    for shape in R.SHAPES:
        img, t, a, b = _apply_truth(shape)
        for k in range(R.N):
            if d["kinds"][k] == "f":
                assert (t[k] == 255).all()  # noqa: PLR2004
                continue
            for name, tol in (("f64", R.tol_f64(t[k], a[k])), ("f32", 2 * b[k])):
                share = R.ambiguous_share(t[k], tol)
                assert share <= R.AMBIGUOUS_CAP[MATHS[name]], (shape, k, name, share)
                worst["apply " + name] = max(worst["apply " + name], share)
            if d["kinds"][k] in "ab":
                assert R.clipped_share(t[k]) < 0.15, (shape, k)  # noqa: PLR2004
    for (shape, _), extreme, bg, z1 in itertools.product(AUG_F64 + AUG_F32, (False, True), (False, True), (False, True)):
        img, ab, t, a, sel, b = _augment_truth(shape, extreme, bg, z1)
        for k in range(R.N):
            for name, tol in (("f64", R.tol_f64(t[k], a[k])), ("f32", 2 * b[k])):
                share = R.ambiguous_share(t[k], tol)
                assert share <= R.AMBIGUOUS_CAP[MATHS[name]], (shape, extreme, bg, z1, k, name, share)
                worst["augment " + name] = max(worst["augment " + name], share)
    print("largest ambiguous share:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert worst["apply f64"] == worst["augment f64"] == 0.0


def test_float32_bounds_hold_for_a_numpy_emulation():
    """A NumPy float32 emulation of ApplyCtx<F32>::pixel and AugCtx::pixel (exact exp2, correctly rounded) stays inside tol = 2 B."""
    worst = {"apply": 0.0, "augment": 0.0}
    for shape in R.SHAPES:
        img, t, _, b = _apply_truth(shape)
        em = np.clip(R.emulate_f32_apply(img, R.inputs()["recs"]), 0, 255)
        worst["apply"] = max(worst["apply"], R.check_float(em, t, 2 * b, f"emulated apply {shape}"))
    for (shape, _), extreme, bg in itertools.product(AUG_F32, (False, True), (False, True)):
        img, ab, t, _, sel, b = _augment_truth(shape, extreme, bg, True)
        em = np.clip(R.emulate_f32_augment(img, R.augment_records(), ab, sel), 0, 255)
        worst["augment"] = max(worst["augment"], R.check_float(em, t, 2 * b, f"emulated augment {shape}"))
    print("emulation: largest error / tol", worst)
    assert worst["apply"] <= 0.5 and worst["augment"] <= 0.5  # noqa: PLR2004  (below B itself)


def _edge_case(shape):
    """Inputs of the rounding-boundary tests: image, records without a contrast stretch, alpha/beta, y_thr, expected selection."""
    img, first, k = R.rounding_edge_image(shape)
    recs = R.augment_records()[:4].copy()
    recs[:, R.ST_PLOW:R.ST_PHIGH + 1] = 0.0                                  # PHIGH == PLOW: the bytes go to the tables as they are
    return img, recs, R.augment_ab(False)[:4], k + 1, first


EDGE_SHAPES = [(64, 80), (50, 50), (37, 41)]


def test_rounding_boundary_pixels():
    """The two triples sit where the search says, the restated tissue test parts them, and their windows are unambiguous enough."""
    lo, hi, k = R.rounding_edge_pixels()
    ty = cvtables.ty_tables().astype(np.int64)
    t_lo, t_hi = (int(sum(ty[c][p[c]] for c in range(3))) for p in (lo, hi))
    assert t_lo == 4096 * k + 2047 and t_hi == t_lo + 1 and lo.min() > 0 and hi.min() > 0  # noqa: PLR2004
    for shape in EDGE_SHAPES:
        img, recs, ab, y, first = _edge_case(shape)
        assert np.array_equal(R.tissue(img, recs, y, zero_to_one=False), first)
        assert R.tissue(img, recs, y + 1, zero_to_one=True).all() and not R.tissue(img, recs, y - 1, zero_to_one=False).any()
        t, a, sel = R.augment_truth(img, recs, ab, y, augment_background=False, zero_to_one=True)
        assert np.array_equal(sel, first)
        b = R.bound_f32_augment(img, recs, ab, sel, t)
        assert R.ambiguous_share(t, R.tol_f64(t, a)) == 0 and R.ambiguous_share(t, 2 * b) <= R.AMBIGUOUS_CAP[R.MATH_F32]
        other = R.augment_truth(img, recs, ab, y + 1, augment_background=False, zero_to_one=True)[0]
        assert (np.floor(np.clip(other, 0, 255)) != np.floor(np.clip(t, 0, 255))).any()   # a moved boundary changes bytes


def test_comparison_rejects_a_wrong_value():
    """The rule would catch what a kernel can get wrong: a swapped matrix row, a byte rounded instead of truncated."""
    img, t, a, b = _apply_truth((37, 41))
    d = R.inputs()
    good = np.floor(np.clip(t, 0, 255)).astype(np.uint8)
    R.check_u8(good, t, R.tol_f64(t, a), R.MATH_F64, "truth")
    recs = d["recs"].copy()
    recs[:, R.ST_M + 6:R.ST_M + 9] = recs[:, R.ST_M + 3:R.ST_M + 6]                 # m[6 + c] <- m[3 + c]
    with pytest.raises(AssertionError):
        R.check_float(np.clip(R.emulate_f32_apply(img, recs), 0, 255), t, 2 * b, "wrong row")
    with pytest.raises(AssertionError):
        R.check_u8(np.rint(np.clip(t, 0, 255)).astype(np.uint8), t, R.tol_f64(t, a), R.MATH_F64, "rounded")
    with pytest.raises(AssertionError):
        R.check_float(np.clip(t, 0, 255).astype(np.float64) * (1 + 1e-9), t, R.tol_f64(t, a), "1e-9 relative")


# ------------------------------------------------------------------------------------------------------------------------------------
# device runners
# ------------------------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch

    return torch


def _dev():
    from tiatoolbox_amd.tools import _stain_device as dev

    return dev


def _out_dtype(out_kind):
    torch = _torch()
    return {R.OUT_U8: torch.uint8, R.OUT_F32: torch.float32, R.OUT_F64: torch.float64, R.OUT_UNIT_F16: torch.float16,
            R.OUT_UNIT_BF16: torch.bfloat16, R.OUT_UNIT_F32: torch.float32}[out_kind]


def _view_at(nbytes: int, off: int):
    """``nbytes`` contiguous bytes that start ``off`` bytes past a 256-byte aligned address, and their buffer."""
    torch = _torch()
    buf = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0  # noqa: PLR2004
    return buf[off:off + nbytes]


def _img_at(img: np.ndarray, off: int = 0):
    torch = _torch()
    v = _view_at(img.size, off).view(img.shape)
    v.copy_(torch.from_numpy(np.array(img)))
    assert v.is_contiguous() and v.data_ptr() % 16 == off % 16  # noqa: PLR2004
    return v


def _run_apply(img, recs, math, out_kind, *, img_off=0, out_off=0):
    """One ``stain_apply`` call (torch tensor on the device); the views sit ``*_off`` bytes past an aligned address."""
    torch = _torch()
    n, h, w, _ = img.shape
    out = _view_at(img.size * ITEMSIZE[out_kind], out_off).view(_out_dtype(out_kind)).view(n, h, w, 3)
    assert out.data_ptr() % 16 == out_off % 16  # noqa: PLR2004
    res = _dev().stain_apply(_img_at(img, img_off), torch.from_numpy(np.array(recs)).cuda(), R.inputs()["target"], out_kind=out_kind,
                             math=math, out=out)
    torch.cuda.synchronize()
    return res


def _np(t):
    torch = _torch()
    return t.to(torch.float32).cpu().numpy() if t.dtype in (torch.float16, torch.bfloat16) else t.cpu().numpy()


def _check_apply(res, u8, math, out_kind, truth, what) -> str:
    """One output of any type by the comparison rule; ``u8``: the same call with OUT_U8 (the unit types are compared exactly: where
    OUT_U8 takes another route or float64 form than the unit type, the bytes still agree because no window of a float64 mode holds
    two values, which test_inputs_meet_the_ambiguity_and_clip_conditions asserts)."""
    torch = _torch()
    _, t, a, b = truth
    tol = _apply_tol(math, out_kind, t, a, b)
    f = R.inputs()["kinds"].index("f")
    if out_kind in (R.OUT_UNIT_F16, R.OUT_UNIT_BF16, R.OUT_UNIT_F32):
        exp = (u8.cpu().to(torch.float32) / 255).to(res.dtype)     # on the host: a correctly rounded float32 division
        assert torch.equal(res.cpu(), exp), f"{what}: not float32(u8) / 255"
        assert bool((res[f] == 1).all())
        return "exact"
    got = _np(res)
    assert (got[f] == 255).all(), f"{what}: M = 0 must give exactly 255"  # noqa: PLR2004
    keep = _not_f()
    if out_kind == R.OUT_U8:
        return f"rate {R.check_u8(got[keep], t[keep], tol[keep], math, what):.1e}"
    ratio = R.check_float(got[keep], t[keep], tol[keep], what)
    err, ratio_normal = R.error_figures(got[keep], t[keep], tol[keep])
    return f"err/tol {ratio:.3f} (err {err:.1e})" if math != R.MATH_F32 else f"err/tol {ratio:.3f} (T >= 255 * 2^-126: {ratio_normal:.3f})"


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU tests
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("math", list(MATHS))
def test_apply_every_mode_type_and_shape(math, shape):
    """Test 1: {F64, F32, F64_REF} x six output types x seven shapes; records a, c, d, f, a, e, a, b in one batch."""
    truth = _apply_truth(shape)
    recs, m = R.inputs()["recs"], MATHS[math]
    u8 = _run_apply(truth[0], recs, m, R.OUT_U8)
    line = []
    for name, kind in OUTS.items():
        res = u8 if kind == R.OUT_U8 else _run_apply(truth[0], recs, m, kind)
        line.append(f"{name}: {_check_apply(res, u8, m, kind, truth, f'{math} {name} {shape}')}")
    print(f"apply {math} {shape[0]}x{shape[1]} [{R.apply_route(m, R.OUT_U8, shape[0] * shape[1])}/{R.apply_route(m, R.OUT_F64, shape[0] * shape[1])}]:",
          "; ".join(line))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALIGN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("math", list(MATHS))
def test_apply_views_that_are_not_16_byte_aligned(math, shape):
    """Test 2: the same pixels through input and ``out=`` views at byte offsets 4, 8, 1 and 3 of a larger buffer (contiguous, so
    ``as_batch`` accepts them).  F32 and F64_REF have one arithmetic on every route: bit-identical to the aligned call.  The float64
    modes are compared with the truth (TIA_MATH_F64 is the table form when aligned and the exponent-trick form otherwise)."""
    torch = _torch()
    truth = _apply_truth(shape)
    recs, m = R.inputs()["recs"], MATHS[math]
    line = []
    for kind, offsets in [(R.OUT_U8, OFFSETS_U8), *OFFSETS_WIDE_OUT.items()]:
        aligned = _run_apply(truth[0], recs, m, kind).clone()
        u8 = aligned if kind == R.OUT_U8 else None
        for io, oo in offsets:
            res = _run_apply(truth[0], recs, m, kind, img_off=io, out_off=oo)
            what = f"{math} out_kind {kind} {shape} offsets {io}, {oo}"
            if m != R.MATH_F64:
                assert torch.equal(res, aligned), f"{what}: differs from the aligned call"
            if m != R.MATH_F32 and kind in (R.OUT_U8, R.OUT_F32, R.OUT_F64):
                line.append(f"{kind}@{io},{oo}: {_check_apply(res, u8, m, kind, truth, what)}")
            elif m == R.MATH_F64:   # unit types: no float64 window holds two values (host test), so floor(clip(T)) is THE byte
                byte = torch.from_numpy(np.floor(np.clip(truth[1], 0, 255)).astype(np.uint8))
                assert torch.equal(res.cpu(), (byte.to(torch.float32) / 255).to(res.dtype)), f"{what}: not float32(floor(T)) / 255"
                line.append(f"{kind}@{io},{oo}: exact")
    print(f"apply {math} {shape[0]}x{shape[1]} misaligned:", "; ".join(line) if line else "bit-identical to the aligned call")


@pytest.mark.gpu
@pytest.mark.parametrize("out", ["u8", "unit_f16"])
@pytest.mark.parametrize("math", ["f64", "f32"])
def test_apply_multi_step_loops(math, out):
    """Test 3: n = 4096 caps the grid at one workgroup per patch: four waves share the five chunks of a 64 x 80 patch, so one wave
    takes two steps.  Bit-identical to the n = 8 call that test 1 checks against the truth."""
    torch = _torch()
    img, m, kind = _apply_truth((64, 80))[0], MATHS[math], OUTS[out]
    recs = R.inputs()["recs"]
    base = _run_apply(img, recs, m, kind)
    big = _run_apply(np.tile(img, (512, 1, 1, 1)), np.tile(recs, (512, 1)), m, kind)
    assert torch.equal(big.view(512, *base.shape), base[None].expand(512, *base.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["augment_f64", "augment_f32", "mask"])
def test_augment_and_mask_multi_step_loops(what):
    """Test 3 for the augment kernels (float64 pair: the grid is capped from n = 1024) and the 16-byte mask kernel."""
    torch = _torch()
    dev = _dev()
    img, ab = R.crop(R.inputs()["imgs"], (64, 80)), R.augment_ab(True)
    recs = R.augment_records()
    reps = 128 if what == "augment_f64" else 512

    def run(k):
        i, r = torch.from_numpy(np.tile(img, (k, 1, 1, 1))).cuda(), torch.from_numpy(np.tile(recs, (k, 1))).cuda()
        if what == "mask":
            return dev.luminosity_mask(i, r, Y085, zero_to_one=True)
        return dev.augment(i, r, torch.from_numpy(np.tile(ab, (k, 1))).cuda(), Y085, augment_background=False, zero_to_one=True,
                           math=R.MATH_F32 if what == "augment_f32" else R.MATH_F64)

    base, big = run(1), run(reps)
    assert torch.equal(big.view(reps, *base.shape), base[None].expand(reps, *base.shape))


@pytest.mark.gpu
def test_wrappers_split_batches_beyond_the_grid_limit():
    """Test 4: 65537 patches of 2 x 2 through the four wrappers (two launches: 65535 + 2); equal to the first eight computed alone."""
    torch = _torch()
    dev = _dev()
    n, reps = 65537, 8193
    img8, ab8 = R.crop(R.inputs()["imgs"], (2, 2)), R.augment_ab(True)
    assert dev._MAX_GRID_Y < n  # noqa: SLF001
    for recs8 in (R.inputs()["recs"], R.augment_records()):
        def tiled(a):
            return torch.from_numpy(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n].copy()).cuda()

        img, recs, ab = tiled(img8), tiled(recs8), tiled(ab8)
        i8, r8, a8 = img[:8].clone(), recs[:8].clone(), ab[:8].clone()
        calls = {
            "apply f64": lambda i, r, a: dev.stain_apply(i, r, R.inputs()["target"]),  # noqa: ARG005
            "apply f32 f32": lambda i, r, a: dev.stain_apply(i, r, R.inputs()["target"], math=R.MATH_F32, out_kind=R.OUT_F32),  # noqa: ARG005
            "concentrations": lambda i, r, a: dev.concentrations(i, r),  # noqa: ARG005
            "mask": lambda i, r, a: dev.luminosity_mask(i, r, Y085, zero_to_one=True),  # noqa: ARG005
            "augment": lambda i, r, a: dev.augment(i, r, a, Y085, augment_background=False, zero_to_one=True),
        }
        for name, fn in calls.items():
            first, full = fn(i8, r8, a8), fn(img, recs, ab)
            assert full.shape[0] == n
            exp = first.repeat(reps, *([1] * (first.dim() - 1)))[:n]
            assert torch.equal(full, exp), name


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_concentrations_equal_numpy_and_longdouble(shape):
    """Test 5: equal to elementwise NumPy in the kernel's order (contraction is off), and within 4 * 2^-53 * sum |terms| of the truth."""
    torch = _torch()
    d = R.inputs()
    img = R.crop(d["imgs"], shape)
    same, truth, mag = R.conc_truth(img, d["recs"])
    got = _dev().concentrations(torch.from_numpy(np.array(img)).cuda(), torch.from_numpy(np.array(d["recs"])).cuda()).cpu().numpy()
    assert got.shape == same.shape
    assert np.array_equal(got, same), f"{int((got != same).sum())} values differ from NumPy; largest {np.abs(got - same).max()}"
    err = np.abs(got.astype(R.LD) - truth)
    bound = 4 * R.LD(2.0) ** -53 * mag
    assert (err <= bound).all()
    print(f"concentrations {shape}: largest error / bound {float((err[mag > 0] / bound[mag > 0]).max()):.3f}")


def _oracle_mask(img, thr):
    try:
        return ostain.get_luminosity_tissue_mask(img.copy(), thr)
    except ValueError:      # "Empty tissue mask computed.": the all-white patch
        return np.zeros(img.shape[:2], bool)


@pytest.mark.gpu
@pytest.mark.parametrize(("shape", "off"), MASK_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"off{v}")
def test_luminosity_mask_every_route(shape, off):
    """Test 6: the 16-byte kernel, the dword route and the byte route, bit-exact against ``oracle.stain.get_luminosity_tissue_mask``
    (which stretches the contrast with ``contrast_enhancer`` first) with PLOW / PHIGH from ``np.percentile(img, (2, 98))``; then
    hand-set records and thresholds against the integer-table restatement."""
    torch = _torch()
    dev = _dev()
    img = R.crop(R.inputs()["imgs"], shape)
    recs = np.zeros((R.N, R.STRIDE))
    for k in range(R.N):
        recs[k, R.ST_PLOW], recs[k, R.ST_PHIGH] = R.percentiles(img[k])
    timg = _img_at(img, off)
    for thr, y in ((0.8, Y080), (0.85, Y085)):
        got = dev.luminosity_mask(timg, torch.from_numpy(recs).cuda(), y).cpu().numpy()
        exp = np.stack([_oracle_mask(p, thr) for p in img])
        assert got.dtype == bool and np.array_equal(got, exp), (thr, int((got != exp).sum()))
        assert np.array_equal(got, R.tissue(img, recs, y, zero_to_one=False))
    # hand-set edges: PHIGH == PLOW (no stretch), PHIGH < PLOW, a narrow and a one-sided window, fractional percentiles
    edge = recs.copy()
    edge[0, R.ST_PLOW:R.ST_PHIGH + 1] = (100.0, 100.0)
    edge[1, R.ST_PLOW:R.ST_PHIGH + 1] = (200.0, 100.0)
    edge[2, R.ST_PLOW:R.ST_PHIGH + 1] = (127.0, 128.0)
    edge[3, R.ST_PLOW:R.ST_PHIGH + 1] = (0.0, 254.0)
    edge[4, R.ST_PLOW:R.ST_PHIGH + 1] = (3.5, 250.25)
    ty = cvtables.ty_tables().astype(np.int64)
    y_all = int((ty[:, 255].sum() + (1 << 11)) >> 12) + 1                # 1 + the largest table sum's index: everything is tissue
    tedge = torch.from_numpy(edge).cuda()
    seen = set()
    for y, z1 in itertools.product((0, Y080, Y085, y_all), (False, True)):
        got = dev.luminosity_mask(timg, tedge, y, zero_to_one=z1).cpu().numpy()
        assert np.array_equal(got, R.tissue(img, edge, y, zero_to_one=z1)), (y, z1)
        seen.add((y, bool(got.all()), bool(got.any())))
    assert (0, False, False) in seen and (y_all, True, True) in seen      # nothing, everything
    if shape == R.FULL:     # zero_to_one decides: with the window (0, 8) the stretch sends 0 to 0 and 1 to 31, and y_thr = 1 parts them
        one = edge.copy()
        one[:, R.ST_PLOW:R.ST_PHIGH + 1] = (0.0, 8.0)
        a, b = (R.tissue(img, one, 1, zero_to_one=z) for z in (False, True))
        assert a[7].all() and not b[7].any()                                # the black patch
        for z in (False, True):
            got = dev.luminosity_mask(timg, torch.from_numpy(one).cuda(), 1, zero_to_one=z).cpu().numpy()
            assert np.array_equal(got, R.tissue(img, one, 1, zero_to_one=z))


def _run_augment(img, recs, ab, math, bg, z1, off=0, y_thr=Y085):
    torch = _torch()
    res = _dev().augment(_img_at(img, off), torch.from_numpy(np.array(recs)).cuda(), torch.from_numpy(ab).cuda(), y_thr,
                         augment_background=bg, zero_to_one=z1, math=math)
    torch.cuda.synchronize()
    return res.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("z1", [False, True], ids=["keep0", "zero_to_one"])
@pytest.mark.parametrize("bg", [False, True], ids=["tissue", "background"])
@pytest.mark.parametrize(("math", "shape", "off"), [("f64", s, o) for s, o in AUG_F64] + [("f32", s, o) for s, o in AUG_F32],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_augment_every_route(math, shape, off, bg, z1):
    """Test 7: the float64 table kernel and its libm partner (64 x 80: table and fall-back patches alternate in the batch), the
    per-pixel float64 kernel (50 x 50, 37 x 41, a view that is not 16-byte aligned) and the float32 kernel, against the truth."""
    m = MATHS[math]
    recs = R.augment_records()
    rates = []
    for extreme in (False, True):
        img, ab, t, a, _, b = _augment_truth(shape, extreme, bg, z1)
        got = _run_augment(img, recs, ab, m, bg, z1, off)
        tol = 2 * b if m == R.MATH_F32 else R.tol_f64(t, a)
        rates.append(R.check_u8(got, t, tol, m, f"augment {math} {shape} off {off} extreme={extreme}"))
    print(f"augment {math} {shape[0]}x{shape[1]} off {off} bg={bg} z1={z1} [{R.augment_route(m, shape[0] * shape[1], off=off)}]: mismatch rates {rates}")


@pytest.mark.gpu
def test_augment_f32_refuses_what_it_has_no_kernel_for():
    from tiatoolbox_amd import _lib

    recs, ab = R.augment_records(), R.augment_ab(False)
    for shape, off in (((50, 50), 0), ((64, 80), 4)):
        with pytest.raises(_lib.HipLibraryError, match="TIA_ESIZE"):
            _run_augment(R.crop(R.inputs()["imgs"], shape), recs, ab, R.MATH_F32, False, True, off)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tissue_test_at_its_rounding_boundary(shape):
    """Pixels whose table sums are 4096 k + 2047 and 4096 k + 2048, with y_thr = k + 1: the descale rounds the first down (tissue) and
    the second up (not tissue).  The mask routes (16-byte, dword, byte) and every augment kernel must part them; a rounding term or a
    comparison that is off by one moves one of the two."""
    torch = _torch()
    dev = _dev()
    img, recs, ab, y, first = _edge_case(shape)
    timg, trecs = torch.from_numpy(img).cuda(), torch.from_numpy(recs).cuda()
    for yy, exp in ((y, first), (y + 1, np.ones_like(first)), (y - 1, np.zeros_like(first))):
        for z1 in (False, True):
            assert np.array_equal(dev.luminosity_mask(timg, trecs, yy, zero_to_one=z1).cpu().numpy(), exp), (yy, z1)
    t, a, sel = R.augment_truth(img, recs, ab, y, augment_background=False, zero_to_one=True)
    assert np.array_equal(sel, first)
    R.check_u8(_run_augment(img, recs, ab, R.MATH_F64, False, True, y_thr=y), t, R.tol_f64(t, a), R.MATH_F64, f"augment f64 {shape} at the boundary")
    if shape == R.FULL:
        R.check_u8(_run_augment(img, recs, ab, R.MATH_F64, False, True, off=4, y_thr=y), t, R.tol_f64(t, a), R.MATH_F64, "augment f64 per pixel at the boundary")
        b = R.bound_f32_augment(img, recs, ab, sel, t)
        R.check_u8(_run_augment(img, recs, ab, R.MATH_F32, False, True, y_thr=y), t, 2 * b, R.MATH_F32, "augment f32 at the boundary")

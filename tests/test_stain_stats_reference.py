"""The per-patch stain statistics (``tia_stain_stats_u8``: the register-resident, streaming and large-image kernels, the window and the
histogram selection and every fall-back between them) against the CPU oracle on inputs chosen to be hard: sparse tissue, massive
ties, angles beyond a right angle, nearly isotropic covariance, contrast-enhancer fall-backs, zero bytes, every size at which the
dispatch changes.  The forms share their arithmetic (stain_stats_common.hpp), so agreement between them proves nothing about it:
here every record is compared with ``oracle/stain.py`` and NumPy, never with another form.

Gates (the project's own): NTISSUE, PLOW, PHIGH, FLAGS exact; COV rtol 1e-9 / atol 1e-12; EVEC, MINPHI, MAXPHI, STAIN, MAXC, PINV
atol 1e-9; M and SCALE 1e-9 of the largest magnitude of the reference block.  The host-only tests prove that the case list reaches the
routes and has the properties it is named for, that the oracle is stable to a hundredth of the gates on every case that is not
rank-deficient by construction, and that the comparison rejects records that are wrong in the ways this code can be wrong."""

from __future__ import annotations

import ctypes

import _stain_stats_ref as R
import numpy as np
import pytest

SELECT_MODES = (0, 1, 2)
PER_PATCH_SHAPES = [s for r in ("small", "register", "above") for s in R.SHAPES[r]]
BIG_SHAPES = R.SHAPES["big"]


def _cases_at(shape, z1=None):
    return [c for c in R.CASES if c.shape == shape and (z1 is None or c.z1 == z1)]


def _fixed_cases() -> list:
    """MODE_FIXED / MODE_GIVEN: one case per class and route, and the three shapes that pin ``np_index`` at n = 1, 2 and 5."""
    seen, out = set(), []
    for c in R.CASES:
        key = (c.cls, R.ROUTE_OF_SHAPE[c.shape], c.z1)
        if key not in seen or (c.cls == "he" and c.shape in [(1, 1), (1, 2), (1, 5)]):
            seen.add(key)
            out.append(c)
    return out


FIXED_CASES = _fixed_cases()


def _hands_back(case: R.Case) -> bool:
    """A Macenko patch the register-resident kernel must return: too few tissue pixels in the window-placing sample."""
    exp = R.expected(case)
    return R.route(*case.shape) == "register" and exp.n_tissue >= 2 and R.sample_members(R.image(case), case.z1) < R.MIN_SAMPLE  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
def test_helper_constants_match_the_library():
    from tiatoolbox_amd import _lib

    for name in ("ST_STAIN", "ST_MAXC", "ST_NTISSUE", "ST_PLOW", "ST_PHIGH", "ST_MINPHI", "ST_MAXPHI", "ST_COV", "ST_EVEC", "ST_FLAGS",
                 "ST_PINV", "ST_M", "ST_SCALE", "FLAG_EMPTY_MASK", "FLAG_DEGENERATE", "MODE_MACENKO", "MODE_FIXED", "MODE_GIVEN"):
        assert getattr(R, name) == getattr(_lib, name), name
    assert R.STRIDE == _lib.TIA_STATS_STRIDE
    used = sorted((lo, lo + n) for lo, n, _ in R.FIELDS.values())
    assert all(a[1] <= b[0] for a, b in zip(used, used[1:])), "the fields overlap"


def test_every_shape_reaches_its_route():
    """``tia_stain_stats_path`` (host query) says which shapes the register-resident kernel takes; the two thresholds of
    stain_stats.hip separate the rest."""
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import _stain_device as dev

    lib = _lib.load()
    for mode in (R.MODE_MACENKO, R.MODE_FIXED, R.MODE_GIVEN):
        for sel in SELECT_MODES:
            prm = dev.make_params(mode=mode, select_mode=sel)
            for shape, name in R.ROUTE_OF_SHAPE.items():
                path = lib.tia_stain_stats_path(*shape, ctypes.byref(prm))
                assert path == int(name == "register" and sel == 0), (shape, mode, sel, path)
                assert R.route(*shape, sel) == (name if sel == 0 and name in ("register", "big") else "streaming")
            # the limits themselves, and their neighbours
            for (h, w), reg in (((64, 64), 1), ((1023, 4), 0), ((4097, 1), 0), ((256, 256), 1), ((16385, 4), 0)):
                assert lib.tia_stain_stats_path(h, w, ctypes.byref(prm)) == (reg if sel == 0 else 0), (h, w, sel)
    hw = {s: s[0] * s[1] for s in R.ROUTE_OF_SHAPE}
    assert all(hw[s] < R.REG_MIN or hw[s] % 4 for s in R.SHAPES["small"]) and hw[(63, 65)] == R.REG_MIN - 1
    assert all(R.REG_MIN <= hw[s] <= R.REG_LIMIT and hw[s] % 4 == 0 for s in R.SHAPES["register"])
    assert hw[(64, 64)] == R.REG_MIN and hw[(256, 256)] == R.REG_LIMIT
    assert all(R.REG_LIMIT - 1 <= hw[s] <= R.BIG_ABOVE for s in R.SHAPES["above"]) and hw[(512, 512)] == R.BIG_ABOVE
    assert hw[(255, 257)] == R.REG_LIMIT - 1 and hw[(255, 257)] % 4 and hw[(116, 565)] == R.REG_LIMIT + 4
    assert all(hw[s] > R.BIG_ABOVE for s in R.SHAPES["big"]) and hw[(4, 65537)] == R.BIG_ABOVE + 4


def test_case_list_and_the_cap_on_skipped_fields():
    """About 150 cases; every class in front of every route; only rank-deficient cases skip fields, at most one case in ten; the
    flagged records are the ones built to be flagged."""
    assert 120 <= len(R.CASES) <= 170  # noqa: PLR2004
    for name, shapes in R.SHAPES.items():
        for shape in shapes:
            assert R.Case("he", shape, 5) in R.CASES, (name, shape)
    for cls in ("sparse", "few_colours", "posterised", "anticorrelated", "uniform", "zeros", "white"):
        routes = {R.ROUTE_OF_SHAPE[c.shape] for c in R.CASES if c.cls == cls}
        assert routes == set(R.SHAPES), (cls, routes)
    assert {R.ROUTE_OF_SHAPE[c.shape] for c in R.CASES if c.cls == "few_colours_band"} == {"small", "register", "above"}
    assert {R.ROUTE_OF_SHAPE[c.shape] for c in R.CASES if c.cls == "enhancer_fallback"} == set(R.SHAPES)
    status = {c: R.expected(c).status for c in R.CASES}
    deficient = [c for c, s in status.items() if s == "rank_deficient"]
    assert 1 <= len(deficient) <= R.RANK_DEFICIENT_SHARE * len(R.CASES), [c.name for c in deficient]
    for c, s in status.items():
        exp = R.expected(c)
        if s == "ok":
            assert exp.fields == R.ALL_MACENKO and exp.rec[R.ST_FLAGS] == 0, c.name
            assert np.isfinite(exp.rec[[lo + i for lo, n, _ in R.FIELDS.values() for i in range(n)]]).all(), c.name
        elif s == "rank_deficient":
            assert set(R.ALL_MACENKO) - set(exp.fields) == set(R.EIGEN_FIELDS), c.name
        elif s == "degenerate":
            assert exp.n_tissue == 1 and exp.rec[R.ST_FLAGS] == R.FLAG_DEGENERATE, c.name
            assert (c.cls == "sparse" and c.arg == 1) or c.shape in [(1, 1), (1, 2)], c.name
        else:
            assert c.cls == "white" and exp.n_tissue == 0 and exp.rec[R.ST_FLAGS] == R.FLAG_EMPTY_MASK, c.name
    assert all(status[c] == "degenerate" for c in R.CASES if c.cls == "sparse" and c.arg == 1)
    assert all(status[c] == "empty" for c in R.CASES if c.cls == "white")
    # fixed and given mode: one case per class and route, and n = 1, 2, 5
    assert {(c.cls, R.ROUTE_OF_SHAPE[c.shape]) for c in FIXED_CASES} == {(c.cls, R.ROUTE_OF_SHAPE[c.shape]) for c in R.CASES}
    assert {(1, 1), (1, 2), (1, 5)} <= {c.shape for c in FIXED_CASES}


def test_contents_have_the_properties_they_are_named_for():  # noqa: C901, PLR0912, PLR0915
    ulp_ranks, fallbacks, handed_back, around_cap = 0, 0, 0, set()
    for c in R.CASES:
        img, exp = R.image(c), R.expected(c)
        hw = c.shape[0] * c.shape[1]
        lo, hi = np.percentile(R._edit(img, c.z1), (2, 98))  # noqa: SLF001
        if c.cls == "sparse":
            assert exp.n_tissue == c.arg, c.name                   # the oracle's mask is the k pixels
            if c.arg * 50 < hw * 3 // 4:                             # well below 2 % of the bytes: both percentiles are the background
                assert lo >= hi, c.name
                assert (exp.rec[R.ST_PLOW], exp.rec[R.ST_PHIGH]) == (img.min(), img.max()), c.name
                fallbacks += 1
            if c.arg in (101, 201):                                # (n - 1) * 0.99 within an ulp of an integer
                vi = (c.arg - 1) * float(np.true_divide(99, 100))
                assert abs(vi - round(vi)) <= np.spacing(vi), c.name
                ulp_ranks += 1
            if c.arg in (R.CAP - 1, R.CAP, R.CAP + 1):
                around_cap.add((R.ROUTE_OF_SHAPE[c.shape], c.arg - R.CAP))
            handed_back += _hands_back(c)
        elif c.cls == "sparse_noise":
            assert 236 <= lo < hi <= 255, c.name                   # noqa: PLR2004  (no fall-back: the enhancer stretches the noise itself)
            assert exp.n_tissue >= c.arg, c.name
        elif c.cls in ("few_colours", "few_colours_band") and exp.status == "ok":
            phi = R.angles(img)
            assert len(np.unique(np.round(phi, 9))) <= 4, c.name    # noqa: PLR2004
            srt = np.sort(phi)
            for q in (0.01, 0.99):                                 # massive exact ties at both percentile ranks
                k = int((len(phi) - 1) * q)
                assert (np.abs(phi - srt[k]) < 1e-9).sum() > len(phi) // 8 or len(phi) < 64, c.name  # noqa: PLR2004
        elif c.cls == "posterised" and hw >= 1000:                  # noqa: PLR2004
            phi = R.angles(img)
            distinct = len(np.unique(np.round(phi, 9)))
            assert 4 < distinct < len(phi) // 4, (c.name, distinct)  # noqa: PLR2004
        elif c.cls == "anticorrelated":
            assert exp.rec[R.ST_MAXPHI] > np.pi / 2, c.name
        elif c.cls == "uniform" and hw >= 1000:                     # noqa: PLR2004
            cov = np.cov(R.tissue_od(img, c.z1), rowvar=False)
            w = np.linalg.eigvalsh(cov)
            assert ((w[1:] - w[:-1]) / w[1:] < 0.2).all(), (c.name, w)  # noqa: PLR2004
            assert exp.rec[R.ST_MINPHI] < -3.0 and exp.rec[R.ST_MAXPHI] > 3.0, c.name  # noqa: PLR2004
            assert (img == 0).any(), c.name
        elif c.cls == "enhancer_fallback":
            assert (lo, hi) == (200.0, 200.0) and exp.rec[R.ST_PLOW] < 200.0 <= exp.rec[R.ST_PHIGH], c.name  # noqa: PLR2004
            fallbacks += 1
            handed_back += _hands_back(c)
        elif c.cls == "zeros":
            assert (img == 0).mean() > 0.03, c.name                 # noqa: PLR2004
            assert exp.rec[R.ST_PLOW] == (1.0 if c.z1 else 0.0), c.name   # the edit is visible in the record
    assert ulp_ranks >= 4 and fallbacks >= 30 and handed_back >= 10, (ulp_ranks, fallbacks, handed_back)  # noqa: PLR2004
    assert around_cap >= {(r, d) for r in ("small", "register") for d in (-1, 0, 1)}, around_cap
    # hand-backs at both ends of the register range, and a window sample below 64 members at a streaming size too
    assert any(_hands_back(c) for c in _cases_at((64, 64))) and any(_hands_back(c) for c in _cases_at((256, 256)))
    assert any(R.sample_members(R.image(c)) < R.MIN_SAMPLE <= R.expected(c).n_tissue for c in _cases_at((512, 512)))


@pytest.mark.parametrize(("name", "cls"), sorted({(R.ROUTE_OF_SHAPE[c.shape], c.cls) for c in R.CASES}))
def test_reference_is_stable_under_pixel_permutations(name, cls):
    """The 1e-9 gates only mean something where the oracle itself is stable: on the reversed image and two shuffles of the pixel
    positions every compared field agrees to a hundredth of its gate (1e-11).  Only cases that are rank-deficient by construction
    skip fields -- there the remaining fields still have to be stable."""
    worst = {"macenko": (0.0, ""), "ruifrok": (0.0, "")}
    for c in R.CASES:
        if R.ROUTE_OF_SHAPE[c.shape] != name or c.cls != cls:
            continue
        for mode in ("macenko", "ruifrok") if c in FIXED_CASES else ("macenko",):
            st = R.stability(c, mode)
            assert st <= R.STABILITY, f"{c.name} [{mode}, {R.expected(c, mode).status}]: the oracle disagrees with itself by {st:.3g} of a gate"
            worst[mode] = max(worst[mode], (st, c.name))
    print(f"reference stability, {name}, {cls}: largest permutation disagreement / gate: " +
          ", ".join(f"{m} {v:.2g}" + (f" ({n})" if v else "") for m, (v, n) in worst.items()))


def test_comparison_accepts_the_oracle_and_rejects_wrong_records():
    """The checks must be able to fail: records that are wrong in the ways this code can be wrong are rejected, the field named."""
    case = None
    for seed in range(40):                                          # a patch on which the eigenvector sign fix changes something
        c = R.Case("he", (64, 64), seed)
        if not np.array_equal(R.macenko_variant(R.image(c), sign_fix=False)[:48], R.macenko_variant(R.image(c))[:48], equal_nan=True):
            case = c
            break
    assert case is not None
    img, exp = R.image(case), R.oracle_macenko(R.image(case))
    assert exp.status == "ok"
    own = R.macenko_variant(img)
    assert np.array_equal(own[:48], exp.rec[:48], equal_nan=True), "the restatement with every switch off is the oracle's record"
    assert max(R.compare(own, exp, "the oracle's own record").values()) == 0.0
    wrong = {
        "ST_MINPHI": {"pct": "next"},                               # rank k + 1 instead of the lerp of k and k + 1
        "ST_MAXPHI": {"pct": "n"},                                  # n q instead of (n - 1) q
        "ST_EVEC": {"sign_fix": False},
        "ST_STAIN": {"swap": True},                                 # H and E rows swapped
        "ST_COV": {"ddof": 0},
        "ST_MAXC": {"maxc_tissue_only": True},
    }
    for field, kw in wrong.items():
        rec = R.macenko_variant(img, **kw)
        with pytest.raises(AssertionError, match=rf"(?s)wrong record.*\n  {field}: got .* expected "):
            R.compare(rec, exp, "wrong record")
    # the mask computed on the un-enhanced image: where the enhancer stretches a bright background into the tissue range
    noise = R.Case("sparse_noise", (256, 256), 500)
    with pytest.raises(AssertionError, match=r"(?s)wrong record.*\n  ST_NTISSUE: got .* expected "):
        R.compare(R.macenko_variant(R.image(noise), mask_unenhanced=True), R.expected(noise), "wrong record")
    # ... and a sparse case: a handful of tissue pixels, where n q and (n - 1) q are furthest apart
    sparse = R.Case("sparse", (64, 64), 5)
    exp5 = R.expected(sparse)
    for kw in ({"pct": "next"}, {"pct": "n"}, {"ddof": 0}):
        with pytest.raises(AssertionError, match="outside the gate"):
            R.compare(R.macenko_variant(R.image(sparse), **kw), exp5, "sparse")
    # a flag that is missing or extra, a count that is off by one, a percentile before its fall-back
    for off, value in ((R.ST_FLAGS, R.FLAG_DEGENERATE), (R.ST_NTISSUE, exp5.n_tissue + 1), (R.ST_PLOW, 255.0)):
        rec = exp5.rec.copy()
        rec[off] = value
        with pytest.raises(AssertionError, match="outside the gate"):
            R.compare(rec, exp5, "edited")
    rec = exp5.rec.copy()
    rec[R.ST_M] += 2e-9 * np.abs(rec[R.ST_M:R.ST_M + 9]).max()
    with pytest.raises(AssertionError, match="ST_M: got"):
        R.compare(rec, exp5, "edited")


# ------------------------------------------------------------------------------------------------------------------------------------
# device
# ------------------------------------------------------------------------------------------------------------------------------------
def _launch(imgs: np.ndarray, mode: str, sel: int, z1: bool, given: np.ndarray | None = None) -> np.ndarray:
    import torch

    from tiatoolbox_amd.tools import _stain_device as dev

    s_t, maxc_t = R.target()
    kw = {"select_mode": sel, "zero_to_one": z1, "target_stain": s_t, "target_maxc": maxc_t}
    if mode == "macenko":
        prm = dev.make_params(mode=R.MODE_MACENKO, **kw)
    elif mode == "given":
        prm = dev.make_params(mode=R.MODE_GIVEN, **kw)
    else:
        prm = dev.make_params(mode=R.MODE_FIXED, stain_fixed=R.fixed_matrix(mode), **kw)
    t = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    stats = dev.stain_stats(t, prm, None if given is None else torch.from_numpy(given))
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def _redo(n: int, shape) -> int:
    import torch

    from tiatoolbox_amd.tools import _stain_device as dev

    return dev.redo_count(torch.device("cuda", torch.cuda.current_device()), n, *shape)


def _run_macenko(cases: list, sel: int, worst: dict) -> int:
    """One launch of the cases (same shape, same ``zero_to_one``), every patch against the oracle; returns the hand-back count."""
    shape, z1 = cases[0].shape, cases[0].z1
    name = R.route(*shape, sel)
    got = _launch(np.stack([R.image(c) for c in cases]), "macenko", sel, z1)
    handed = _redo(len(cases), shape) if name == "register" else 0
    for i, c in enumerate(cases):
        ratios = R.compare(got[i], R.expected(c), f"{c.name}, route {name}, select_mode {sel}, patch {i}")
        R.merge_worst(worst, ratios)
    return handed


@pytest.mark.gpu
@pytest.mark.parametrize("sel", SELECT_MODES)
@pytest.mark.parametrize("shape", PER_PATCH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_macenko_per_patch_kernels_against_the_oracle(shape, sel):
    worst: dict = {}
    handed = 0
    for z1 in (False, True):
        cases = _cases_at(shape, z1)
        if cases:
            handed += _run_macenko(cases, sel, worst)
    name = R.route(*shape, sel)
    expect = sum(_hands_back(c) for c in _cases_at(shape)) if name == "register" else 0
    if expect:
        assert handed >= 1, f"{shape}: {expect} patches have fewer than {R.MIN_SAMPLE} sampled tissue pixels, none was handed back"
    print(f"stats macenko {shape[0]}x{shape[1]} [{name}] select_mode {sel}: {len(_cases_at(shape))} cases, handed back {handed} "
          f"(expected at least {min(expect, 1)}); worst error / gate: {R.show(worst)}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BIG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_macenko_large_image_kernels_against_the_oracle(shape):
    worst: dict = {}
    for z1 in (False, True):
        cases = _cases_at(shape, z1)
        for i in range(0, len(cases), 2):                           # batches of two: two images' workgroups in one launch
            _run_macenko(cases[i:i + 2], 0, worst)
    print(f"stats macenko {shape[0]}x{shape[1]} [big] select_mode 0: {len(_cases_at(shape))} cases; worst error / gate: {R.show(worst)}")


@pytest.mark.gpu
@pytest.mark.parametrize("sel", SELECT_MODES)
@pytest.mark.parametrize("mode", ["ruifrok", "skew", "given"])
def test_fixed_and_given_matrices_against_the_oracle(mode, sel):
    """``ST_MAXC`` ranks all ``h w`` pixels here (1 x 1, 1 x 2, 1 x 5: ``np_index`` at n = 1, 2, 5); ``ST_PINV``, ``ST_M`` and
    ``ST_SCALE`` against NumPy.  MODE_GIVEN: every batch position has its own matrix, so a wrong patch index into ``d_stats`` shows."""
    worst: dict = {}
    for shape in R.ROUTE_OF_SHAPE:
        name = R.route(*shape, sel)
        if sel and R.ROUTE_OF_SHAPE[shape] == "big":
            continue                                                # (the audit modes are per-patch forms)
        for z1 in (False, True):
            cases = [c for c in FIXED_CASES if c.shape == shape and c.z1 == z1]
            if not cases:
                continue
            first = len(cases)
            if mode == "given":
                cases = cases + cases[::-1]                         # at least two positions, the same image under two matrices
            chunk = 2 if R.ROUTE_OF_SHAPE[shape] == "big" else len(cases)
            for lo in range(0, len(cases), chunk):
                part = cases[lo:lo + chunk]
                index = [2 * FIXED_CASES.index(c) + int(lo + i >= first) for i, c in enumerate(part)]
                given = np.stack([R.given_matrix(k) for k in index]) if mode == "given" else None
                got = _launch(np.stack([R.image(c) for c in part]), mode, sel, z1, given)
                for i, c in enumerate(part):
                    exp = R.expected(c, mode, index[i] if mode == "given" else 0)
                    R.merge_worst(worst, R.compare(got[i], exp, f"{c.name}, {mode}, route {name}, select_mode {sel}, patch {i}"))
    print(f"stats {mode} select_mode {sel}: {len(FIXED_CASES)} cases; worst error / gate: {R.show(worst)}")


@pytest.mark.gpu
@pytest.mark.parametrize("side", [64, 256])
def test_mixed_batches_do_not_depend_on_their_neighbours(side):
    """Dense, sparse (handed back), empty, few colours, one tissue pixel, dense: each patch against the oracle at its own index,
    forwards and in reversed order, and bit-identical between the two launches."""
    shape = (side, side)
    cases = [R.Case("he", shape, 5), R.Case("sparse", shape, 5), R.Case("white", shape), R.Case("few_colours", shape, 3),
             R.Case("sparse", shape, 1), R.Case("posterised", shape, 3), R.Case("sparse", shape, 63), R.Case("he", shape, 5)]
    assert all(c in R.CASES for c in cases) and _hands_back(cases[1]) and _hands_back(cases[6])
    assert [R.expected(c).status for c in cases] == ["ok", "ok", "empty", "ok", "degenerate", "ok", "ok", "ok"]
    for sel in SELECT_MODES:
        worst: dict = {}
        got = _launch(np.stack([R.image(c) for c in cases]), "macenko", sel, False)
        handed = _redo(len(cases), shape) if sel == 0 else 0
        back = _launch(np.stack([R.image(c) for c in cases[::-1]]), "macenko", sel, False)[::-1]
        for i, c in enumerate(cases):
            exp = R.expected(c)
            R.merge_worst(worst, R.compare(got[i], exp, f"{c.name}, mixed batch, select_mode {sel}, patch {i}"))
            R.compare(back[i], exp, f"{c.name}, reversed mixed batch, select_mode {sel}, patch {len(cases) - 1 - i}")
            assert got[i, :48].tobytes() == back[i, :48].tobytes(), f"{c.name}, select_mode {sel}: patch {i} depends on its position"
        assert got[0, :48].tobytes() == got[-1, :48].tobytes()     # the same image twice in one batch
        flags = got[:, R.ST_FLAGS].astype(int).tolist()
        assert flags == [0, 0, R.FLAG_EMPTY_MASK, 0, R.FLAG_DEGENERATE, 0, 0, 0], flags
        if sel == 0:
            assert handed >= 1, "no patch of the mixed batch was handed back to the streaming kernel"
        print(f"stats mixed batch {side}x{side} select_mode {sel}: handed back {handed}; worst error / gate: {R.show(worst)}")

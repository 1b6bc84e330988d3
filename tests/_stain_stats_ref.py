"""Helpers of ``tests/test_stain_stats_reference.py``: the case list of the per-patch stain statistics (``tia_stain_stats_u8``), the
record the CPU oracle (``oracle/stain.py``) gives for a case, the conditioning of that record, the comparison rule and which kernel a
shape reaches.  NumPy and the oracle only: no torch, no device.

The reference is never another form of the kernel: every expected value comes from ``MacenkoExtractor.get_stain_matrix``,
``StainNormalizer.get_concentrations``, ``np.percentile``, ``np.linalg.pinv`` and the expressions of ``_stain_pixel_ref.make_record``.
``ST_PLOW`` / ``ST_PHIGH`` hold what ``contrast_enhancer`` actually uses (``ce_percentiles`` of stain_stats_common.hpp applies the
min / max fall-back before it returns), i.e. ``_stain_pixel_ref.percentiles``."""

from __future__ import annotations

import functools
import warnings
from typing import NamedTuple

import numpy as np
from _stain_pixel_ref import make_record, percentiles

from oracle import stain as ostain
from tiatoolbox_amd.utils import synth

# include/tiatoolbox_amd.h (checked against tiatoolbox_amd._lib by the test module)
ST_STAIN, ST_MAXC, ST_NTISSUE, ST_PLOW, ST_PHIGH, ST_MINPHI, ST_MAXPHI = 0, 6, 8, 9, 10, 11, 12
ST_COV, ST_EVEC, ST_FLAGS, ST_PINV, ST_M, ST_SCALE, STRIDE = 13, 19, 25, 26, 32, 41, 64
FLAG_EMPTY_MASK, FLAG_DEGENERATE = 1, 2
MODE_MACENKO, MODE_FIXED, MODE_GIVEN = 0, 1, 3
# name -> (offset, length, gate kind); the order is the order of the report
FIELDS = {
    "ST_NTISSUE": (ST_NTISSUE, 1, "exact"), "ST_PLOW": (ST_PLOW, 1, "exact"), "ST_PHIGH": (ST_PHIGH, 1, "exact"),
    "ST_FLAGS": (ST_FLAGS, 1, "exact"), "ST_COV": (ST_COV, 6, "cov"), "ST_EVEC": (ST_EVEC, 6, "abs"),
    "ST_MINPHI": (ST_MINPHI, 1, "abs"), "ST_MAXPHI": (ST_MAXPHI, 1, "abs"), "ST_STAIN": (ST_STAIN, 6, "abs"),
    "ST_MAXC": (ST_MAXC, 2, "abs"), "ST_PINV": (ST_PINV, 6, "abs"), "ST_M": (ST_M, 9, "block"), "ST_SCALE": (ST_SCALE, 2, "block"),
}
STAT_TOL = 1e-9                    # test_stain_gpu.py: per-patch float64 statistics
COV_RTOL, COV_ATOL = 1e-9, 1e-12   # test_macenko_stats_match_oracle
STABILITY = 0.01                   # the reference must agree with itself on permuted pixels to a hundredth of every gate (1e-11)
EIGEN_FIELDS = ("ST_EVEC", "ST_MINPHI", "ST_MAXPHI", "ST_STAIN", "ST_MAXC", "ST_PINV", "ST_M", "ST_SCALE")
ALL_MACENKO = tuple(FIELDS)
ALL_FIXED = ("ST_PLOW", "ST_PHIGH", "ST_FLAGS", "ST_STAIN", "ST_MAXC", "ST_PINV", "ST_M", "ST_SCALE")   # what a fixed / given launch writes
RANK_DEFICIENT_SHARE = 0.1

# stain_stats_common.hpp / stain_stats.hip
CAP, SAMPLE_TARGET, MIN_SAMPLE = 1024, 4096, 64
REG_MIN, REG_LIMIT, BIG_ABOVE = 4096, 65536, 4 * 256 * 256
LUMINOSITY_THRESHOLD = 0.8

# the smallest shapes at which each route and boundary exists ("above": the streaming kernel around and above the register limit)
SHAPES = {
    "small": [(1, 1), (1, 2), (1, 5), (7, 1), (3, 5), (8, 8), (37, 41), (63, 65)],
    "register": [(64, 64), (41, 100), (100, 102), (256, 256)],
    "above": [(255, 257), (116, 565), (512, 512)],
    "big": [(513, 512), (4, 65537)],
}
ROUTE_OF_SHAPE = {s: r for r, ss in SHAPES.items() for s in ss}
RUIFROK = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])
SKEW = np.array([[0.55, 0.76, 0.35], [0.31, 0.84, 0.45]])        # rows 17 degrees apart, not unit length
TARGET_SEED = 77


def route(h: int, w: int, select_mode: int = 0) -> str:
    """The kernel a Macenko / fixed / given launch of ``h x w`` patches reaches (stain_stats.hip, restated): "big" (many workgroups
    per image), "register" (what it hands back goes through the streaming kernel) or "streaming" (the rows "small" and "above" of
    ``SHAPES``, and every size under ``select_mode`` 1 and 2)."""
    hw = h * w
    if select_mode == 0 and hw > BIG_ABOVE:
        return "big"
    if select_mode == 0 and REG_MIN <= hw <= REG_LIMIT and hw % 4 == 0:
        return "register"
    return "streaming"


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    cls: str
    shape: tuple
    arg: int = 0                   # k of the sparse class, else the seed
    z1: bool = False               # zero_to_one

    @property
    def name(self) -> str:
        return f"{self.cls}-{self.shape[0]}x{self.shape[1]}-{self.arg}" + ("-z1" if self.z1 else "")


SPARSE_K = (1, 2, 3, 5, 63, 64, 65, 101, 201, 1023, 1024, 1025, 4097)
FEW_COLOURS = np.array([[200, 60, 150], [120, 40, 160], [230, 150, 200], [90, 90, 170], [255, 255, 255]], np.uint8)


def _cases() -> list:
    out = []
    for shape in ROUTE_OF_SHAPE:                                   # the control, one per shape
        out.append(Case("he", shape, 5))
    for shape in [(37, 41), (64, 64), (256, 256)]:                 # every k the shape holds, in front of each per-patch kernel
        out += [Case("sparse", shape, k) for k in SPARSE_K if k <= shape[0] * shape[1] * 3 // 4]
    out += [Case("sparse", (100, 102), k) for k in (3, 64, 201, 1025)]
    out += [Case("sparse", (255, 257), k) for k in (5, 65, 1024, 4097)]
    out += [Case("sparse", (512, 512), k) for k in (3, 101, 1025)]
    out += [Case("sparse", (513, 512), k) for k in (5, 1023, 4097)]
    out += [Case("sparse", (4, 65537), 201)]
    out += [Case("sparse_noise", (256, 256), 500)]
    out += [Case("white", s) for s in [(1, 1), (8, 8), (64, 64), (256, 256), (116, 565), (513, 512)]]
    for cls in ("few_colours", "few_colours_band", "posterised", "anticorrelated", "uniform"):
        out += [Case(cls, s, 3) for s in [(3, 5), (37, 41), (63, 65), (64, 64), (41, 100), (256, 256), (116, 565), (513, 512)]
                if cls != "few_colours_band" or s != (513, 512)]
    out += [Case("few_colours", (512, 512), 4), Case("uniform", (255, 257), 4), Case("anticorrelated", (4, 65537), 4),
            Case("posterised", (512, 512), 4), Case("uniform", (8, 8), 4), Case("few_colours", (7, 1), 4)]
    out += [Case("enhancer_fallback", s, 3) for s in [(63, 65), (64, 64), (100, 102), (256, 256), (255, 257), (513, 512)]]
    for s in [(37, 41), (64, 64), (256, 256), (116, 565), (513, 512)]:
        out += [Case("zeros", s, 3, z1=False), Case("zeros", s, 3, z1=True)]
    assert len(set(out)) == len(out)
    return out


def _donor(seed: int) -> np.ndarray:
    """Tissue-coloured pixels of a ``g_he`` patch (the dark ones: the bright fifth is its background)."""
    px = synth.g_he(1, 96, 96, seed=100 + seed)[0].reshape(-1, 3)
    return px[px.mean(1) < 150.0]                                  # noqa: PLR2004


@functools.lru_cache(maxsize=None)
def image(case: Case) -> np.ndarray:
    """The image of a case, a seeded function of its class, shape and argument (read only)."""
    h, w = case.shape
    hw = h * w
    rng = np.random.default_rng([case.arg, h, w, sum(map(ord, case.cls))])
    if case.cls == "he":
        img = synth.g_he(1, h, w, seed=case.arg)[0]
    elif case.cls in ("sparse", "sparse_noise", "enhancer_fallback"):
        k = {"sparse": case.arg, "sparse_noise": case.arg, "enhancer_fallback": 40}[case.cls]
        flat = np.full((hw, 3), 255, np.uint8)
        if case.cls == "sparse_noise":
            flat = rng.integers(236, 256, (hw, 3), dtype=np.uint8)
        elif case.cls == "enhancer_fallback":
            flat[:] = 200
        donor = _donor(case.arg % 7)
        flat[rng.choice(hw, k, replace=False)] = donor[rng.choice(len(donor), k, replace=k > len(donor))]
        img = flat.reshape(h, w, 3)
    elif case.cls == "white":
        img = np.full((h, w, 3), 255, np.uint8)
    elif case.cls in ("few_colours", "few_colours_band"):
        img = FEW_COLOURS[rng.integers(0, 5, (h, w))]
        if case.cls == "few_colours_band":
            img[: max(1, h // 4)] = 255
    elif case.cls == "posterised":
        img = (synth.g_he(1, h, w, seed=case.arg)[0] // 32 * 32 + 16).astype(np.uint8)
    elif case.cls == "anticorrelated":
        t, u = rng.random((h, w)), rng.random((h, w))
        img = np.stack([40 + 200 * t, 240 - 200 * t, 128 + 20 * u], -1).astype(np.uint8)
    elif case.cls == "uniform":
        img = synth.g_uniform(1, h, w, seed=case.arg)[0]
    elif case.cls == "zeros":
        img = synth.g_he(1, h, w, seed=case.arg)[0]
        img[h // 3: h // 3 + max(1, h // 5), w // 4: w // 4 + max(2, w // 3)] = 0
    else:
        raise KeyError(case.cls)
    img = np.ascontiguousarray(img, np.uint8)
    assert img.shape == (h, w, 3)
    img.setflags(write=False)
    return img


def permuted(img: np.ndarray, which: int) -> np.ndarray:
    """Pixel positions reversed (0) or shuffled with seed ``which`` (1, 2): every statistic is invariant."""
    flat = img.reshape(-1, 3)
    order = np.arange(len(flat))[::-1] if which == 0 else np.random.default_rng(1000 + which).permutation(len(flat))
    return np.ascontiguousarray(flat[order].reshape(img.shape))


# ------------------------------------------------------------------------------------------------------------------------------------
# the oracle's record
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def target() -> tuple:
    """Target stain matrix and maxC of every launch (``has_target = 1``): an oracle fit of one ``g_he`` image."""
    img = synth.g_he(1, 96, 96, seed=TARGET_SEED)[0]
    s = ostain.MacenkoExtractor().get_stain_matrix(img.copy())
    maxc = np.percentile(ostain.StainNormalizer.get_concentrations(img.copy(), s), 99, axis=0)
    return s, maxc


def given_matrix(index: int) -> np.ndarray:
    """MODE_GIVEN: patch ``index`` brings its own matrix (Ruifrok's rows, perturbed by a function of the index, unit length)."""
    s = np.abs(RUIFROK + np.random.default_rng(500 + index).normal(0.0, 0.04, (2, 3)))
    return s / np.linalg.norm(s, axis=1, keepdims=True)


class Expected(NamedTuple):
    rec: np.ndarray                # [64], NaN where the oracle has no value
    fields: tuple                  # the fields to compare
    status: str                    # "ok", "rank_deficient", "degenerate" (one tissue pixel), "empty" (no tissue pixel)
    n_tissue: int


def _edit(img: np.ndarray, z1: bool) -> np.ndarray:
    out = img.copy()
    if z1:
        out[out == 0] = 1                                          # rgb2od's in-place edit, seen by the mask path
    return out


def _finish(rec: np.ndarray, stain: np.ndarray, img: np.ndarray) -> None:
    """MAXC, PINV, SCALE, M and the degenerate flag from a stain matrix, by the oracle's arithmetic."""
    s_t, maxc_t = target()
    conc = ostain.StainNormalizer.get_concentrations(img.copy(), stain)
    maxc = np.percentile(conc, 99, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = maxc_t / maxc
    full = make_record(stain, scale, s_t)
    for lo, n in ((ST_STAIN, 6), (ST_PINV, 6), (ST_M, 9), (ST_SCALE, 2)):
        rec[lo:lo + n] = full[lo:lo + n]
    rec[ST_MAXC:ST_MAXC + 2] = maxc
    finite = np.isfinite(rec[ST_STAIN:ST_STAIN + 6]).all() and np.isfinite(rec[ST_PINV:ST_PINV + 6]).all() and np.isfinite(maxc).all()
    rec[ST_FLAGS] = 0.0 if finite and np.isfinite(scale).all() else float(FLAG_DEGENERATE)


def tissue_od(img: np.ndarray, z1: bool) -> np.ndarray:
    """Optical densities of the oracle's tissue pixels, [n_tissue, 3] (empty when the mask is)."""
    try:
        mask = ostain.get_luminosity_tissue_mask(_edit(img, z1), threshold=LUMINOSITY_THRESHOLD).ravel()
    except ValueError:
        return np.zeros((0, 3))
    return ostain.rgb2od(img.copy()).reshape(-1, 3)[mask]


def rank_deficient(od: np.ndarray) -> bool:
    """``matrix_rank`` of the centred tissue OD matrix below 2: its second singular value is rounding noise (below 1e-10 of the
    first, a tenth of the gate), so the second eigenvector, and with it every angle, is LAPACK's choice."""
    if len(od) < 2:  # noqa: PLR2004
        return False
    centred = od - od.mean(0)
    return int(np.linalg.matrix_rank(centred, tol=1e-10 * np.linalg.norm(centred, 2))) < 2  # noqa: PLR2004


def oracle_macenko(img: np.ndarray, z1: bool = False) -> Expected:
    rec = np.full(STRIDE, np.nan)
    edited = _edit(img, z1)
    rec[ST_PLOW], rec[ST_PHIGH] = percentiles(edited)
    od = tissue_od(img, z1)
    n = len(od)
    rec[ST_NTISSUE] = n
    if n == 0:
        rec[ST_FLAGS] = FLAG_EMPTY_MASK
        return Expected(rec, ("ST_NTISSUE", "ST_PLOW", "ST_PHIGH", "ST_FLAGS"), "empty", n)
    if n == 1:                     # np.cov with ddof = 1 is NaN and eigh does not converge in the reference
        rec[ST_FLAGS] = FLAG_DEGENERATE
        return Expected(rec, ("ST_NTISSUE", "ST_FLAGS"), "degenerate", n)
    dbg: dict = {}
    stain = ostain.MacenkoExtractor().get_stain_matrix(edited, debug=dbg)
    assert dbg["n_tissue"] == n
    cov = dbg["cov"]
    rec[ST_COV:ST_COV + 6] = [cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]]
    rec[ST_EVEC:ST_EVEC + 6] = dbg["eigen_vectors"].T.ravel()
    rec[ST_MINPHI], rec[ST_MAXPHI] = dbg["min_phi"], dbg["max_phi"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _finish(rec, stain, img)
    if rank_deficient(od):
        return Expected(rec, tuple(f for f in ALL_MACENKO if f not in EIGEN_FIELDS), "rank_deficient", n)
    return Expected(rec, ALL_MACENKO, "ok", n)


def oracle_fixed(img: np.ndarray, stain: np.ndarray, z1: bool = False) -> Expected:
    """MODE_FIXED / MODE_GIVEN: the stain matrix is an input; ``ST_MAXC`` ranks all ``h w`` pixels."""
    rec = np.full(STRIDE, np.nan)
    rec[ST_PLOW], rec[ST_PHIGH] = percentiles(_edit(img, z1))
    _finish(rec, np.asarray(stain, np.float64), img)
    return Expected(rec, ALL_FIXED, "ok", -1)


@functools.lru_cache(maxsize=None)
def expected(case: Case, mode: str = "macenko", index: int = 0) -> Expected:
    """The oracle's record of a case (cached).  ``mode``: "macenko", "ruifrok", "skew" or "given" (the matrix of patch ``index``)."""
    img = image(case)
    if mode == "macenko":
        exp = oracle_macenko(img, case.z1)
    else:
        exp = oracle_fixed(img, fixed_matrix(mode, index), case.z1)
    exp.rec.setflags(write=False)
    return exp


def fixed_matrix(mode: str, index: int = 0) -> np.ndarray:
    return {"ruifrok": RUIFROK, "skew": SKEW}[mode] if mode != "given" else given_matrix(index)


# ------------------------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ------------------------------------------------------------------------------------------------------------------------------------
def field_ratio(name: str, got: np.ndarray, exp: np.ndarray) -> float:
    """Largest error of one field as a fraction of its gate (exact fields: 0 or inf; a non-finite value on one side only: inf)."""
    lo, n, kind = FIELDS[name]
    g, e = np.asarray(got[lo:lo + n], np.float64), np.asarray(exp[lo:lo + n], np.float64)
    if kind == "exact":
        return 0.0 if np.array_equal(g, e) else np.inf
    if not (np.isfinite(g).all() and np.isfinite(e).all()):
        return 0.0 if np.array_equal(g, e, equal_nan=True) else np.inf
    err = np.abs(g - e)
    if kind == "cov":
        return float((err / (COV_ATOL + COV_RTOL * np.abs(e))).max())
    if kind == "abs":
        return float(err.max() / STAT_TOL)
    return float(err.max() / (STAT_TOL * np.abs(e).max())) if np.abs(e).max() > 0 else (0.0 if err.max() == 0 else np.inf)


def compare(got: np.ndarray, exp: Expected, what: str, *, tighten: float = 1.0) -> dict:
    """Every field of ``exp.fields`` within its gate (times ``tighten``); returns error / gate per field.  A failure names ``what``
    (case, route, patch index), the fields and both values."""
    ratios = {name: field_ratio(name, got, exp.rec) for name in exp.fields}
    bad = [name for name, r in ratios.items() if not r <= tighten]
    if bad:
        lines = []
        for name in bad:
            lo, n, _ = FIELDS[name]
            lines.append(f"  {name}: got {np.asarray(got[lo:lo + n]).tolist()} expected {exp.rec[lo:lo + n].tolist()} (error / gate {ratios[name]:.3g})")
        raise AssertionError(f"{what} [{exp.status}, n_tissue {exp.n_tissue}]: {', '.join(bad)} outside the gate\n" + "\n".join(lines))
    return ratios


def merge_worst(worst: dict, ratios: dict) -> None:
    for k, v in ratios.items():
        worst[k] = max(worst.get(k, 0.0), v)


def show(worst: dict) -> str:
    return ", ".join(f"{k[3:]} {v:.2g}" for k, v in worst.items() if FIELDS[k][2] != "exact") or "exact fields only"


@functools.lru_cache(maxsize=None)
def stability(case: Case, mode: str = "macenko") -> float:
    """Largest disagreement (as a fraction of the gates) between the oracle's record of the case and of three permuted copies, over
    the fields the case compares; inf when a permuted copy changes the status."""
    exp = expected(case, mode)
    worst = 0.0
    for which in range(3):
        img = permuted(image(case), which)
        other = oracle_macenko(img, case.z1) if mode == "macenko" else oracle_fixed(img, fixed_matrix(mode), case.z1)
        if other.status != exp.status:
            return np.inf
        worst = max([worst] + [field_ratio(name, other.rec, exp.rec) for name in exp.fields])
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# host restatements used by the property checks
# ------------------------------------------------------------------------------------------------------------------------------------
def sample_members(img: np.ndarray, z1: bool = False) -> int:
    """Tissue pixels among the window-placing sample (``sample_index`` of stain_stats_common.hpp, restated)."""
    h, w = img.shape[:2]
    hw = h * w
    stride = -(-hw // SAMPLE_TARGET)
    k = np.arange(SAMPLE_TARGET, dtype=np.uint64)
    hsh = ((k * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)
    idx = k * np.uint64(stride) + (hsh % np.uint64(stride) if stride > 1 else np.uint64(0))
    idx = idx[idx < hw].astype(np.int64)
    try:
        mask = ostain.get_luminosity_tissue_mask(_edit(img, z1), threshold=LUMINOSITY_THRESHOLD).ravel()
    except ValueError:
        return 0
    return int(mask[idx].sum())


def angles(img: np.ndarray, z1: bool = False) -> np.ndarray:
    """The oracle's per-pixel angles ``phi`` of the tissue pixels."""
    dbg: dict = {}
    ostain.MacenkoExtractor().get_stain_matrix(_edit(img, z1), debug=dbg)
    od = tissue_od(img, z1)
    proj = od @ dbg["eigen_vectors"]
    return np.arctan2(proj[:, 1], proj[:, 0])


def macenko_variant(img: np.ndarray, *, pct: str = "lerp", sign_fix: bool = True, swap: bool = False, ddof: int = 1,
                    maxc_tissue_only: bool = False, mask_unenhanced: bool = False) -> np.ndarray:
    """The Macenko record restated step by step, with switches for the mistakes this code can make; with the defaults it is the
    oracle's record bit for bit (asserted by the test module)."""
    s_t, maxc_t = target()

    def pick(v: np.ndarray, q: float) -> float:
        v = np.sort(v)
        n = len(v)
        if pct == "lerp":
            return float(np.percentile(v, q))
        vi = (n if pct == "n" else n - 1) * (q / 100)
        k = min(int(np.floor(vi)), n - 1)
        nxt = min(k + 1, n - 1)
        return float(v[nxt]) if pct == "next" else float(v[k] + (v[nxt] - v[k]) * (vi - np.floor(vi)))

    if mask_unenhanced:
        from oracle import cvref

        mask = (cvref.rgb2lab_u8(img.copy())[:, :, 0] / 255.0 < LUMINOSITY_THRESHOLD).ravel()
    else:
        mask = ostain.get_luminosity_tissue_mask(img.copy(), threshold=LUMINOSITY_THRESHOLD).ravel()
    od_all = ostain.rgb2od(img.copy()).reshape(-1, 3)
    od = od_all[mask]
    cov = np.cov(od, rowvar=False, ddof=ddof)
    _, ev = np.linalg.eigh(cov)
    ev = ev[:, [2, 1]]
    if sign_fix:
        ev = ostain.vectors_in_correct_direction(ev)
    proj = np.dot(od, ev)
    phi = np.arctan2(proj[:, 1], proj[:, 0])
    min_phi, max_phi = pick(phi, 1), pick(phi, 99)
    v1 = np.dot(ev, np.array([np.cos(min_phi), np.sin(min_phi)]))
    v2 = np.dot(ev, np.array([np.cos(max_phi), np.sin(max_phi)]))
    he = ostain.h_and_e_in_right_order(v1, v2)
    if swap:
        he = he[::-1]
    stain = he / np.linalg.norm(he, axis=1)[:, None]
    conc = ostain.StainNormalizer.get_concentrations(img.copy(), stain)
    maxc = np.percentile(conc[mask] if maxc_tissue_only else conc, 99, axis=0)
    rec = np.full(STRIDE, np.nan)
    full = make_record(stain, maxc_t / maxc, s_t)
    for lo, n in ((ST_STAIN, 6), (ST_PINV, 6), (ST_M, 9), (ST_SCALE, 2)):
        rec[lo:lo + n] = full[lo:lo + n]
    rec[ST_MAXC:ST_MAXC + 2] = maxc
    rec[ST_NTISSUE], rec[ST_FLAGS] = int(mask.sum()), 0.0
    rec[ST_PLOW], rec[ST_PHIGH] = percentiles(img)
    rec[ST_COV:ST_COV + 6] = [cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]]
    rec[ST_EVEC:ST_EVEC + 6] = ev.T.ravel()
    rec[ST_MINPHI], rec[ST_MAXPHI] = min_phi, max_phi
    return rec


CASES = _cases()

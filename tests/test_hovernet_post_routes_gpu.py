"""Every route of the HoVer-Net post-processing (``hover_proc_impl``, ``csrc/hover_post.hip``) stage by stage against the oracle:
``blb``, the raw float64 Sobel planes, ``dist``, the labelled markers and the instance map must EQUAL ``oracle.hovernet.proc_np_hv``'s
locals on the fused route (A), the wide-row route (B), the middle route (C), the multi-launch route (D, every whole-slide tile) and
the one remaining mix (E); at compile-time and run-time Sobel sizes; on planes thinner than the filter's anchor; and on batches in
which one plane's normalisation degenerates.  ``torch.profiler`` proves which kernels ran.  ``inst_stats_kernel`` is compared with
a per-pixel NumPy statement that has no run logic.  No tolerance anywhere except the exact-arithmetic cross-check of the border rule,
whose bound is derived where it is used."""

from __future__ import annotations

import functools
import os
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import cvref
from oracle import hovernet as oh

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _hover_routes_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

STAGES = (("blb", "blb"), ("sobel_h", "sobel_h_raw"), ("sobel_v", "sobel_v_raw"), ("dist", "dist"), ("marker", "marker"))


def _hd():
    from tiatoolbox_amd.models.architecture import _hover_device as hd

    return hd


def _run_stages(npm: np.ndarray, hv: np.ndarray, scale: float) -> dict:
    got = _hd().proc_np_hv_stages(torch.from_numpy(npm).cuda(), torch.from_numpy(hv).cuda(), ksize=ref.ksize_of(scale),
                                  obj_size=ref.obj_size_of(scale))
    return {k: v.cpu().numpy() for k, v in got.items()}


def _oracle(np_plane: np.ndarray, hv_plane: np.ndarray, scale: float) -> dict:
    dbg = {}
    dbg["inst"] = oh.proc_np_hv(np_plane, hv_plane, scale_factor=scale, debug=dbg)
    return dbg


def _stage_mismatches(got: dict, exp: dict, i: int) -> list[str]:
    """Every stage plane of batch plane ``i`` that is not EQUAL to the oracle's, with the number of differing pixels and the
    maximum absolute difference."""
    bad = []
    for mine, theirs in (*STAGES, ("inst", "inst")):
        g, e = got[mine][i], exp[theirs]
        if g.shape != e.shape or not np.array_equal(g, e):
            diff = np.abs(g.astype(np.float64) - e.astype(np.float64)) if g.shape == e.shape else np.array([np.inf])
            bad.append(f"plane {i} {mine}: {int((diff != 0).sum())} px differ, max |d| = {diff.max():.3e}")
    if int(got["n_markers"][i]) < int(got["inst"][i].max()):
        bad.append(f"plane {i} n_markers {int(got['n_markers'][i])} < inst.max() {int(got['inst'][i].max())}")
    return bad


@functools.lru_cache(maxsize=None)
def _case(h: int, w: int, scale: float, n: int = 2):
    """Inputs and oracle planes of one ``ROUTE_CASES`` row: computed once, shared by the tests, never modified."""
    npm, hv = ref.case_maps(n, h, w, seed=1000 + h + w)
    exp = tuple(_oracle(npm[i], hv[i], scale) for i in range(n))
    for a in (npm, hv, *(v for e in exp for v in e.values())):
        a.setflags(write=False)
    return npm, hv, exp


# ------------------------------------------------------------------------------------------------------- stage planes on every route
@pytest.mark.parametrize(("want", "h", "w", "scale"), ref.ROUTE_CASES, ids=[f"{r}-{h}x{w}-k{ref.ksize_of(s)}" for r, h, w, s in ref.ROUTE_CASES])
def test_stage_planes_on_every_route(want, h, w, scale):
    assert ref.route(h, w, ref.ksize_of(scale)) == want
    npm, hv, exp = _case(h, w, scale)
    got = _run_stages(npm, hv, scale)
    bad = [m for i in range(len(exp)) for m in _stage_mismatches(got, exp[i], i)]
    assert not bad, (want, h, w, scale, bad)


# ----------------------------------------------------------------------------------------------------------------- the route really ran
TILE_SOBEL = ("sobel_energy_tile_kernel",)
ALONE_SOBEL = ("minmax_hv_kernel", "sobel_row_kernel", "sobel_col_kernel", "minmax_pair_kernel", "energy_kernel")
GAUSS = ("gauss3_neg_kernel",)
TILE_LABEL, ALONE_LABEL = ("ccl_tile_kernel",), ("np_threshold_kernel",)
TILE_MARKER = ("marker_tile_kernel",)
# route -> (one case of it, kernels that define it, kernels that must not run)
ROUTE_KERNELS = {
    "A": ((96, 120, 1), TILE_LABEL + TILE_SOBEL + TILE_MARKER, ALONE_SOBEL + GAUSS + ALONE_LABEL),
    "B": ((24, 440, 1), TILE_LABEL + ALONE_SOBEL + GAUSS + TILE_MARKER, TILE_SOBEL + ALONE_LABEL),
    "C": ((180, 200, 0.3), TILE_LABEL + TILE_SOBEL + GAUSS, ALONE_SOBEL + TILE_MARKER + ALONE_LABEL),
    "D": ((193, 192, 1), ALONE_LABEL + ALONE_SOBEL + GAUSS, TILE_SOBEL + TILE_MARKER + TILE_LABEL),
    "E": ((48, 700, 1), TILE_LABEL + ALONE_SOBEL + GAUSS, TILE_SOBEL + TILE_MARKER + ALONE_LABEL),
}


@pytest.mark.parametrize("name", sorted(ROUTE_KERNELS))
def test_the_route_really_ran(name):
    if os.environ.get("TIA_NO_CCL_TILE") is not None:
        pytest.skip("TIA_NO_CCL_TILE is set: the developer switch sends every plane down the multi-launch route")
    from torch.profiler import ProfilerActivity, profile

    (h, w, scale), present, absent = ROUTE_KERNELS[name]
    assert ref.route(h, w, ref.ksize_of(scale)) == name and (name, h, w, scale) in ref.ROUTE_CASES
    npm, hv, _ = _case(h, w, scale)
    d_np, d_hv = torch.from_numpy(npm).cuda(), torch.from_numpy(hv).cuda()
    kw = {"ksize": ref.ksize_of(scale), "obj_size": ref.obj_size_of(scale)}
    _hd().proc_np_hv_stages(d_np, d_hv, **kw)  # library load, one-time attributes
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        _hd().proc_np_hv_stages(d_np, d_hv, **kw)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()}
    kernels = {k for k in names if "memcpy" not in k.lower() and "memset" not in k.lower()}
    print(f"route {name} {h}x{w} ksize {kw['ksize']}: " + " ".join(sorted({k.split("(")[0].split("::")[-1] for k in kernels})))
    for wanted in present:
        assert any(wanted in k for k in kernels), (name, wanted, kernels)
    for banned in absent:
        assert not any(banned in k for k in kernels), (name, banned, kernels)
    if name in "AC":  # which instance of the tile kernel: <21> for ksize 21, the run-time form <0> for ksize 7
        tile = [k for k in kernels if TILE_SOBEL[0] in k]
        tile = [k for k in tile if "<" in k or "ILi" in k]  # names that carry their template argument, plain or mangled
        assert all(("<21>" in k or "ILi21E" in k) if kw["ksize"] == 21 else ("<0>" in k or "ILi0E" in k) for k in tile), tile  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------------------------ thin and tiny planes
def _border_101(p: int, n: int) -> int:
    """OpenCV ``borderInterpolate(p, n, BORDER_REFLECT_101)``: reflect until the index is inside; ``n == 1`` gives 0."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def _sobel_exact(src: np.ndarray, ksize: int, dx: int, dy: int, pixels) -> tuple[list[Fraction], list[Fraction]]:
    """The Sobel sum at ``pixels`` in exact rational arithmetic, straight from its definition
    ``sum_j sum_k ky[j] kx[k] S[r(y + j - a), r(x + k - a)]`` (taps from ``cvref.sobel_kernels``, ``r`` = ``_border_101``), and the
    sum of the terms' magnitudes (what the rounding error of a float64 evaluation scales with)."""
    kx, ky = (np.asarray(k).astype(np.int64).tolist() for k in cvref.sobel_kernels(ksize, dx, dy))
    h, w = src.shape
    a = ksize // 2
    unit = 2**149  # every finite float32 is an integer multiple of 2^-149: the sums below are exact integer arithmetic
    s = [[int(Fraction(float(v)) * unit) for v in row] for row in src]
    exact, mag = [], []
    for (y, x) in pixels:
        rows = [_border_101(y + j - a, h) for j in range(ksize)]
        cols = [_border_101(x + k - a, w) for k in range(ksize)]
        tot = m = 0
        for j, r in enumerate(rows):
            tot += ky[j] * sum(kx[k] * s[r][c] for k, c in enumerate(cols))
            m += abs(ky[j]) * sum(abs(kx[k] * s[r][c]) for k, c in enumerate(cols))
        exact.append(Fraction(tot, unit))
        mag.append(Fraction(m, unit))
    return exact, mag


def _border_rule_errors(planes: dict, src32: np.ndarray, ksize: int, dx: int, dy: int) -> list[str]:
    """For each float64 Sobel plane in ``planes`` (name -> plane): the pixels of one row and one column, both on the border, where
    it is further from the exact value than a float64 evaluation can be.  The products tap x float32 are exact in float64 (taps
    < 2^28, 24-bit significands); the row pass adds ksize of them in sequence (ksize - 1 roundings); the column pass rounds each
    term's inner sum, its product and at most ksize / 2 + 1 accumulations (ksize / 2 + 3 roundings at most).  To first order the
    error is at most (ksize - 1 + ksize / 2 + 3) u <= 2 ksize u times the sum of the terms' magnitudes, u = 2^-53; one more u
    covers the second-order terms.  A wrong border index changes a term by its own magnitude: some 2^45 times more."""
    h, w = src32.shape
    pixels = [(h - 1, x) for x in range(w)] + [(y, 0) for y in range(h - 1)]
    exact, mag = _sobel_exact(src32, ksize, dx, dy, pixels)
    out = []
    for side, plane in planes.items():
        errs = [f"({y},{x}): {float(plane[y, x])!r} vs exact {float(e)!r}" for (y, x), e, m in zip(pixels, exact, mag)
                if abs(Fraction(float(plane[y, x])) - e) > Fraction(2 * ksize + 1, 2**53) * m]
        if errs:
            out.append(f"{side} off the exact sums at {len(errs)} of {len(pixels)} px, first {errs[0]}")
    return out


@pytest.mark.parametrize("scale", [1, 0.5], ids=["k21", "k11"])
@pytest.mark.parametrize(("h", "w"), ref.TINY_SHAPES, ids=[f"{h}x{w}" for h, w in ref.TINY_SHAPES])
def test_thin_and_tiny_planes(h, w, scale):
    """Planes with ``h <= ksize / 2`` or ``w <= ksize / 2`` (the tile kernel's general reflection: border taps reflect more than
    once) and their neighbours just above.  The oracle is the reference; the exact sums say which side is right if they differ."""
    ksize = ref.ksize_of(scale)
    npm, hv = ref.tiny_maps(2, h, w)
    got = _run_stages(npm, hv, scale)
    exp = [_oracle(npm[i], hv[i], scale) for i in range(2)]
    bad = [m for i in range(2) for m in _stage_mismatches(got, exp[i], i)]
    for ch, (name, dx, dy) in enumerate((("sobel_h", 1, 0), ("sobel_v", 0, 1))):
        src32 = cvref.normalize_minmax_to_f32(hv[0, ..., ch])
        bad += [f"{name}: {m}" for m in _border_rule_errors({"oracle": exp[0][name + "_raw"], "kernel": got[name][0]}, src32, ksize, dx, dy)]
    assert not bad, (h, w, ksize, bad)


# --------------------------------------------------------------------------------------------------------- degenerate maps in a batch
@pytest.mark.parametrize(("h", "w"), [(64, 64), (193, 192)], ids=["A-64x64", "D-193x192"])
def test_degenerate_normalisation_inside_a_batch(h, w):
    """One call, three planes: ordinary; the same ``np`` with a constant h map (range below DBL_EPSILON: ``norm_params`` gives
    scale 0); the same ``np`` with both maps zero.  Each plane equals the oracle's -- so planes 2 and 3 do not disturb plane 1."""
    assert ref.route(h, w, 21) == ("A" if h == 64 else "D")  # noqa: PLR2004
    npm1, hv1, _ = oh.synth_maps(1, h, w, seed=77, n_blobs=max(6, h * w // 450))
    npm = np.concatenate([npm1, npm1, npm1])
    hv = np.concatenate([hv1, hv1, np.zeros_like(hv1)])
    hv[1, ..., 0] = 0.25
    got = _run_stages(npm, hv, 1)
    exp = [_oracle(npm[i], hv[i], 1) for i in range(3)]
    assert exp[0]["marker"].max() > 3 and exp[0]["inst"].max() > 3  # noqa: PLR2004 -- plane 1 is an ordinary one
    assert not exp[1]["sobel_h_raw"].any() and exp[1]["sobel_v_raw"].any() and not exp[2]["sobel_v_raw"].any()
    bad = [m for i in range(3) for m in _stage_mismatches(got, exp[i], i)]
    alone = _run_stages(npm[:1], hv[:1], 1)
    bad += ["alone: " + m for m in _stage_mismatches(alone, exp[0], 0)]
    assert not bad, (h, w, bad)


# ------------------------------------------------------------------------------------------------------- instance statistics vs NumPy
def _stats_ref(inst: np.ndarray, types: np.ndarray | None, max_inst: int, num_types: int):
    """Per-pixel statement of ``tia_hover_instance_stats``: area, x/y minimum, x/y maximum, x/y sums per id in ``1..max_inst``
    (other ids ignored); histogram of the type values below ``num_types``."""
    n, h, w = inst.shape
    stats = np.zeros((n, max_inst + 1, 7), np.int64)
    stats[..., 1:3] = 0x7FFFFFFF
    stats[..., 3:5] = -1
    hist = np.zeros((n, max_inst + 1, num_types), np.int32) if types is not None else None
    for p in range(n):
        ids = inst[p].ravel().astype(np.int64)
        keep = np.flatnonzero((ids > 0) & (ids <= max_inst))
        i, y, x = ids[keep], keep // w, keep % w
        stats[p, :, 0] = np.bincount(i, minlength=max_inst + 1)
        np.minimum.at(stats[p, :, 1], i, x)
        np.minimum.at(stats[p, :, 2], i, y)
        np.maximum.at(stats[p, :, 3], i, x)
        np.maximum.at(stats[p, :, 4], i, y)
        np.add.at(stats[p, :, 5], i, x)
        np.add.at(stats[p, :, 6], i, y)
        if types is not None:
            t = types[p].ravel()[keep].astype(np.int64)
            sel = t < num_types
            np.add.at(hist[p], (i[sel], t[sel]), 1)
    return stats, hist


def _check_stats(inst: np.ndarray, types: np.ndarray | None, max_inst: int, num_types: int, tag) -> None:
    d_types = torch.from_numpy(types).cuda() if types is not None else None
    stats, hist = _hd().instance_stats(torch.from_numpy(inst).cuda(), d_types, max_inst, num_types)
    stats = stats.cpu().numpy()
    exp_stats, exp_hist = _stats_ref(inst, types, max_inst, num_types)
    assert stats.dtype == np.int64 and stats.shape == (*exp_stats.shape[:2], 8)
    assert np.array_equal(stats[..., 0], exp_stats[..., 0]), (tag, "area", np.argwhere(stats[..., 0] != exp_stats[..., 0])[:5])
    live = exp_stats[..., 0] > 0
    assert live.any(), tag
    wrong = np.argwhere(stats[..., :7][live] != exp_stats[live])
    assert wrong.size == 0, (tag, wrong[:5], stats[..., :7][live][wrong[0][0]], exp_stats[live][wrong[0][0]])
    if types is None:
        assert hist is None
    else:
        hist = hist.cpu().numpy()
        assert hist.dtype == np.int32 and np.array_equal(hist, exp_hist), (tag, np.argwhere(hist != exp_hist)[:5])


def _runs(rng, total: int, lengths, values) -> np.ndarray:
    """``total`` values laid out in runs of random lengths along the FLAT index, so that runs cross row ends."""
    out = np.empty(total, np.int64)
    at = 0
    while at < total:
        n = int(rng.choice(lengths))
        out[at:at + n] = rng.choice(values)
        at += n
    return out


@pytest.mark.parametrize("w", [1, 63, 64, 65, 129, 256])
def test_instance_stats_vs_numpy_widths(w):
    """Random runs (1 to 130 pixels, so shorter and longer than a wave) of ids and, independently, of types over ``n = 3`` planes
    with different id sets; ids ``-1`` and ``max_inst + 1`` and types ``>= num_types`` present; with and without a type map."""
    rng = np.random.default_rng(100 + w)
    max_inst, num_types = 12, 5
    for h in (3, 9) if w > 1 else (9, 300):
        id_sets = ([0, 0, 1, 2, 3, 4, -1, max_inst + 1], [0, 5, 6, 7, 8, 12, 12, max_inst + 1], [9, 10, 11, -1])
        inst = np.stack([_runs(rng, h * w, (1, 2, 5, 17, 64, 70, 130), ids) for ids in id_sets]).reshape(3, h, w).astype(np.int32)
        types = np.stack([_runs(rng, h * w, (1, 3, 40, 64, 100), np.arange(num_types + 3)) for _ in range(3)])
        types = types.reshape(3, h, w).astype(np.uint8)
        inst.reshape(3, -1)[:, h * w // 2] = -1             # whatever the runs drew: every plane has both ignored ids and,
        inst.reshape(3, -1)[:, h * w // 2 + 1] = max_inst + 1
        types.reshape(3, -1)[:, h * w // 2 + 2] = num_types  # under a counted id, a type outside the histogram
        inst.reshape(3, -1)[:, h * w // 2 + 2] = [1, 5, 9]
        assert (inst == -1).any() and (inst == max_inst + 1).any() and (types >= num_types).any()
        _check_stats(inst, types, max_inst, num_types, (w, h, "types"))
        _check_stats(inst, None, max_inst, 0, (w, h, "no types"))


def test_instance_stats_runs_at_wave_and_row_ends():
    """Hand-placed runs: longer than a wave; ending at lane 63; and one that continues across a row end (the same id in the last
    pixels of a row and the first of the next, inside one wave: only the ``x == 0`` head separates the two rows' runs)."""
    h, w, max_inst = 6, 65, 6
    flat = np.zeros(h * w, np.int32)
    flat[10:40] = 6
    flat[40:64] = 1        # ends at lane 63 (flat index = lane in the first wave)
    flat[64:64 + 150] = 2  # starts at lane 0, longer than two waves, crosses rows 0 -> 1 -> 2 -> 3
    flat[257:262] = 3      # row 3 (x = 62..64) into row 4 (x = 0, 1): flat 260 is x == 0 at lane 4
    flat[300:320] = 4
    flat[325:330] = 5      # row 4 ends at flat 324; row 5 starts at flat 325 with a new id (head by id change and by x == 0)
    inst = flat.reshape(1, h, w)
    assert inst[0, 3, 62:].tolist() == [3, 3, 3] and inst[0, 4, :3].tolist() == [3, 3, 0] and 260 % 64 != 0  # noqa: PLR2004
    types = np.zeros((1, h, w), np.uint8)
    types[0, 3:5] = 2      # one type over the row-crossing run: the type does not cut it either
    _check_stats(inst, types, max_inst, 4, "hand-placed")
    _check_stats(inst, None, max_inst, 0, "hand-placed, no types")


def test_instance_stats_second_grid_stride_trip():
    """1025 x 1024 = 1,049,600 pixels: more than the 4096 x 256 the grid covers at once, so the first blocks take a second trip
    (every 1280 x 1280 whole-slide tile does).  Blocked random ids; the rows of the second trip carry ids found nowhere else."""
    rng = np.random.default_rng(7)
    max_inst, num_types = 300, 6
    inst = np.kron(rng.integers(0, 281, (205, 128)), np.ones((5, 8), np.int64))[None].astype(np.int32)
    assert inst.shape == (1, 1025, 1024) and inst.size > 4096 * 256  # noqa: PLR2004
    inst[0, 1024, :512] = 290
    inst[0, 1024, 512:900] = 300
    inst[0, 1024, 900:] = max_inst + 1
    types = np.kron(rng.integers(0, num_types + 2, (205, 256)), np.ones((5, 4), np.int64))[None].astype(np.uint8)
    _check_stats(inst, types, max_inst, num_types, "1025x1024")

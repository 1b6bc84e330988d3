"""The two border followers of ``csrc/contours.hip`` in the regimes the engines run them in.

``tia_hover_contour_scan`` / ``tia_hover_contour_write`` (``_hover_device.contours``): batches whose entry count lies on both sides of
the 1024 threads of ``contour_offsets_kernel`` (chunks of 1, 2 and 3 entries per thread), planes that differ in everything, one plane
of 3025 ids; raw ``meta`` (all four columns of every entry) and every slice of ``points`` must EQUAL the oracle statement of
``_contour_ref``, for every id with pixels, and satisfy the scipy statement of outer borders.  ``tia_label_first_pixel_i32`` /
``tia_border_trace_u8`` (``_hover_device.all_borders``): a plane one row larger than the first-pixel kernel's grid covers in one trip,
batches whose planes differ in component count, thin planes; same length and order of borders as ``cvref.find_contours`` and every
array equal.  Then the refusals and the ``capacity`` guards of all four entry points.  Equality everywhere: there is no tolerance."""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import cvref
from oracle import hovernet as oh

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _contour_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

OK, EINVAL, ESIZE = 0, -1, -3


def _hd():
    from tiatoolbox_amd.models.architecture import _hover_device as hd

    return hd


def _dev(a: np.ndarray) -> torch.Tensor:
    """A device copy of a (read-only) case array."""
    return torch.from_numpy(np.array(a)).cuda()


def _contours(lab: np.ndarray, max_inst: int) -> tuple[np.ndarray, np.ndarray]:
    """``hd.contours`` with the statistics of ``hd.instance_stats`` of the same map (they bound the follower's loop)."""
    d = _dev(lab)
    stats, _ = _hd().instance_stats(d, None, max_inst)
    return _hd().contours(d, stats, max_inst)


@functools.lru_cache(maxsize=None)
def _expected(case: str):
    lab, max_inst = ref.label_case(case)
    meta, points = ref.expected_contours(ref.borders_of(case), lab.shape[0], max_inst)
    meta.setflags(write=False)
    points.setflags(write=False)
    return meta, points


# ------------------------------------------------------------------------------------------------------- hd.contours on batches
@pytest.mark.parametrize("case", ref.LABEL_CASES)
def test_contours_of_batches_vs_oracle(case):
    lab, max_inst = ref.label_case(case)
    n, h, w = lab.shape
    exp_meta, exp_points = _expected(case)
    meta, points = _contours(lab, max_inst)
    entries = n * (max_inst + 1)
    print(f"{case}: {n} x {h} x {w}, {entries} entries (chunk {ref.offsets_chunk(entries)}), {int((exp_meta[..., 2] > 0).sum())} polygons, "
          f"{len(exp_points)} vertices")
    bad = ref.compare_contours(meta, points, exp_meta, exp_points, sorted(ref.borders_of(case)))
    assert not bad, (case, len(bad), bad[:8])
    assert points.dtype == np.int32 and len(points) == int(meta[..., 2].astype(np.int64).sum())  # total == len(points)
    assert ((points >= 0) & (points < np.array([w, h]))).all()
    again = _contours(lab, max_inst)
    assert np.array_equal(again[0], meta) and np.array_equal(again[1], points)  # two runs agree bit for bit


@pytest.mark.parametrize("case", ref.LABEL_CASES)
def test_contours_of_batches_vs_scipy_statement(case):
    """Start pixels and expanded chains against the statement that does not follow borders at all."""
    lab, max_inst = ref.label_case(case)
    meta, points = _contours(lab, max_inst)
    bad = ref.scipy_mismatches(lab, meta, points)
    assert not bad, (case, len(bad), bad[:8])


def test_contours_do_not_depend_on_the_order_of_planes():
    """The same planes in another order: every plane's start pixels, counts and polygons are unchanged, and its offsets are
    shifted exactly by the number of vertices in front of it."""
    lab, max_inst = ref.label_case("mixed")
    exp_meta, exp_points = _expected("mixed")
    order = [2, 0, 3, 1]
    meta, points = _contours(np.ascontiguousarray(lab[order]), max_inst)
    base = np.concatenate([[0], np.cumsum(meta[..., 2].sum(axis=1))])
    exp_base = np.concatenate([[0], np.cumsum(exp_meta[..., 2].sum(axis=1))])
    assert len(points) == len(exp_points) == base[-1]
    for at, plane in enumerate(order):
        assert np.array_equal(meta[at, :, :3], exp_meta[plane, :, :3]), plane
        assert np.array_equal(meta[at, :, 3] - base[at], exp_meta[plane, :, 3] - exp_base[plane]), plane
        assert np.array_equal(points[base[at]:base[at + 1]], exp_points[exp_base[plane]:exp_base[plane + 1]]), plane
    borders = {(order.index(p), i): v for (p, i), v in ref.borders_of("mixed").items()}
    m2, p2 = ref.expected_contours(borders, len(order), max_inst)
    assert not ref.compare_contours(meta, points, m2, p2, sorted(borders))


def test_postproc_batch_equals_per_plane_postproc_and_the_oracle():
    """``HoVerNet.postproc_batch`` on three synthetic head-map planes == per-plane ``postproc`` == ``oracle.get_instance_info``,
    column by column."""
    from tiatoolbox_amd.models.architecture.hovernet import HoVerNet

    npm, hv, tp = oh.synth_maps(3, 96, 96, seed=31, n_blobs=14)
    npm = npm.copy()
    npm[2, :, 40:] = 0  # the third plane keeps fewer nuclei: the planes of the batch differ in instance count
    model = HoVerNet(num_types=6, mode="fast")
    batch = model.postproc_batch(_dev(npm), _dev(hv), _dev(tp))
    assert len(batch) == 3  # noqa: PLR2004
    sizes = []
    for i in range(3):
        (single,) = model.postproc([npm[i], hv[i], tp[i]])
        inst = oh.proc_np_hv(npm[i], hv[i])
        info = oh.get_instance_info(inst, np.around(tp[i]).astype("uint8")[..., 0])
        sizes.append(len(info))
        assert np.array_equal(batch[i]["predictions"], inst) and np.array_equal(single["predictions"], inst)
        for got in (batch[i]["info_dict"], single["info_dict"]):
            assert len(got["box"]) == len(info)
            assert np.array_equal(np.asarray(got["box"]), np.array([v["box"] for v in info.values()]))
            np.testing.assert_array_equal(np.asarray(got["centroid"]), np.array([v["centroid"] for v in info.values()]))
            for a, v in zip(got["contours"], info.values()):
                assert a.dtype == np.int32 and np.array_equal(a, v["contours"])
            assert list(got["type"]) == [v["type"] for v in info.values()]
            assert list(got["prob"]) == [v["prob"] for v in info.values()]
    assert min(sizes) > 3 and sizes[2] < sizes[0], sizes  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------------------------ all_borders
def _all_borders(planes: np.ndarray, simple: bool) -> list:  # noqa: FBT001
    return _hd().all_borders(_dev(planes), simple=simple)


@pytest.mark.parametrize("simple", [False, True], ids=["none", "simple"])
def test_all_borders_of_each_kind_of_plane(simple):
    for name, m in ref.binary_planes().items():
        exp = ref.expected_borders(name, simple)
        got = _all_borders(m[None], simple)
        assert len(got) == 1
        bad = ref.compare_borders(got[0], exp)
        assert not bad, (name, m.shape, bad[:5])


@pytest.mark.parametrize("simple", [False, True], ids=["none", "simple"])
def test_all_borders_of_six_very_different_planes(simple):
    """All-zero, all-one, 0.5 random, nested one-pixel rings, the pockets plane and a single pixel in ONE call: ``kmax`` is the
    batch maximum, so most planes leave most cells of the first-pixel tables at their fill."""
    six = ref.six_planes()
    got = _all_borders(six, simple)
    assert len(got) == len(six)
    print("borders per plane:", [len(g) for g in got])
    for i in range(len(six)):
        bad = ref.compare_borders(got[i], ref.expected_borders(f"six{i}", simple))
        assert not bad, (i, bad[:5])
    back = _all_borders(six[::-1], simple)  # the sparse planes first
    for i in range(len(six)):
        assert not ref.compare_borders(back[len(six) - 1 - i], ref.expected_borders(f"six{i}", simple)), i


@pytest.mark.parametrize("simple", [False, True], ids=["none", "simple"])
def test_all_borders_beyond_the_first_pixel_kernels_grid(simple):
    """1025 x 1024: the last row is reached by the second grid-stride trip only.  Alone, and as plane 1 behind an empty plane."""
    big = ref.big_plane()
    assert big.size > ref.first_pixel_cap()
    exp = ref.expected_borders("big", simple)
    got = _all_borders(big[None], simple)
    bad = ref.compare_borders(got[0], exp)
    assert not bad, bad[:5]
    pair = _all_borders(np.stack([np.zeros_like(big), big]), simple)
    assert pair[0] == []
    bad = ref.compare_borders(pair[1], exp)
    assert not bad, bad[:5]


# ------------------------------------------------------------------------------------------------- the entry points themselves
def _starts_of(planes: np.ndarray) -> tuple[np.ndarray, list, list]:
    """Start table of ``tia_border_trace_u8`` (plane, x0, y0, is_hole) for every border of every plane, in ``cvref``'s order of
    discovery, and the borders themselves in both modes."""
    rows, chains, simples = [], [], []
    for p, m in enumerate(planes):
        tree_n = cvref.find_contours_tree(m, simple=False)
        tree_s = cvref.find_contours_tree(m, simple=True)
        for b, s in zip(tree_n, tree_s):
            rows.append((p, int(b["points"][0, 0]), int(b["points"][0, 1]), int(b["is_hole"])))
            chains.append(b["points"].astype(np.int32))
            simples.append(s["points"].astype(np.int32))
    return np.asarray(rows, np.int32).reshape(-1, 4), chains, simples


def test_border_trace_counts_and_capacity_guard():
    """``tia_border_trace_u8`` on a start table stated by the oracle (no labelling kernel involved): the count pass, then the write
    pass with a ``capacity`` that cuts one border in two.  Every border that fits is written and equal, the others are skipped, and no
    row at or beyond ``capacity`` changes."""
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    planes = np.stack([ref.binary_planes()["random0.62"], ref.pockets_plane(), np.zeros((40, 52), np.uint8)])
    starts, chains, simples = _starts_of(planes)
    nb = len(starts)
    assert nb > 2 * ref.source_constants()["CT"] and nb % ref.source_constants()["CT"] != 0
    n, h, w = planes.shape
    d_mask, d_starts = _dev(planes), _dev(starts)
    sentinel = -7
    for simple, exp in ((1, simples), (0, chains)):
        counts = torch.full((nb + 8,), sentinel, dtype=torch.int32, device="cuda")
        assert lib.tia_border_trace_u8(d_mask.data_ptr(), n, h, w, d_starts.data_ptr(), nb, simple, counts.data_ptr(), 0, 0, 0, stream) == OK
        cnt = counts.cpu().numpy()
        assert np.array_equal(cnt[:nb], [len(e) for e in exp]) and (cnt[nb:] == sentinel).all()
        off = np.cumsum(cnt[:nb].astype(np.int64)) - cnt[:nb]
        total = int(cnt[:nb].sum())
        long_ones = np.flatnonzero(cnt[:nb] >= 3)  # noqa: PLR2004
        cut = int(long_ones[len(long_ones) // 2])  # this border straddles the capacity
        capacity = int(off[cut]) + 1
        assert 0 < capacity < total
        d_off = _dev(off)
        points = torch.full((total + 16, 2), sentinel, dtype=torch.int32, device="cuda")
        assert lib.tia_border_trace_u8(d_mask.data_ptr(), n, h, w, d_starts.data_ptr(), nb, simple, counts.data_ptr(), d_off.data_ptr(),
                                       capacity, points.data_ptr(), stream) == OK
        pts = points.cpu().numpy()
        fits = off + cnt[:nb] <= capacity
        assert fits.any() and not fits.all() and np.array_equal(counts.cpu().numpy(), cnt)
        for e in range(nb):
            got = pts[off[e]:off[e] + cnt[e]]
            assert np.array_equal(got, exp[e]) if fits[e] else (got == sentinel).all(), (simple, e)
        assert (pts[int(off[cut]):] == sentinel).all()
        assert lib.tia_border_trace_u8(d_mask.data_ptr(), n, h, w, d_starts.data_ptr(), nb, simple, counts.data_ptr(), d_off.data_ptr(),
                                       total, points.data_ptr(), stream) == OK
        pts = points.cpu().numpy()
        assert np.array_equal(pts[:total], np.concatenate(exp)) and (pts[total:] == sentinel).all()


def _scan_setup():
    lab, max_inst = ref.label_case("mixed")
    d_inst = _dev(lab)
    stats, _ = _hd().instance_stats(d_inst, None, max_inst)
    return lab, max_inst, d_inst, stats


def test_contour_write_capacity_guard():
    """The write pass with a ``capacity`` smaller than ``total`` that cuts one polygon in two, on a ``points`` buffer with sentinel
    rows behind it: every polygon that fits is written and equal, the others are skipped, no row at or beyond ``capacity`` changes."""
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    lab, max_inst, d_inst, stats = _scan_setup()
    n, h, w = lab.shape
    exp_meta, exp_points = _expected("mixed")
    meta = torch.empty((n, max_inst + 1, 4), dtype=torch.int32, device="cuda")
    mark = torch.empty((n, h, w), dtype=torch.int8, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert lib.tia_hover_contour_scan(d_inst.data_ptr(), n, h, w, max_inst, stats.data_ptr(), mark.data_ptr(), meta.data_ptr(),
                                      total.data_ptr(), stream) == OK
    assert int(total.item()) == len(exp_points) and np.array_equal(meta.cpu().numpy(), exp_meta)
    flat = exp_meta.reshape(-1, 4).astype(np.int64)
    sentinel = -7
    big = np.flatnonzero(flat[:, 2] >= 3)  # noqa: PLR2004
    for cut in (int(big[len(big) // 2]), int(big[0]), int(big[-1])):
        capacity = int(flat[cut, 3]) + 1  # the polygon of entry `cut` straddles it
        points = torch.full((len(exp_points) + 16, 2), sentinel, dtype=torch.int32, device="cuda")
        assert lib.tia_hover_contour_write(d_inst.data_ptr(), n, h, w, max_inst, stats.data_ptr(), meta.data_ptr(), capacity,
                                           points.data_ptr(), stream) == OK
        pts = points.cpu().numpy()
        fits = (flat[:, 2] > 0) & (flat[:, 3] + flat[:, 2] <= capacity)
        assert not fits[cut] and fits.sum() < (flat[:, 2] > 0).sum()
        assert np.array_equal(pts[:flat[cut, 3]], exp_points[:flat[cut, 3]])  # everything in front of the cut fits, and is equal
        assert (pts[flat[cut, 3]:] == sentinel).all()                         # the cut polygon and all behind it: skipped
    points = torch.full((len(exp_points) + 16, 2), sentinel, dtype=torch.int32, device="cuda")
    assert lib.tia_hover_contour_write(d_inst.data_ptr(), n, h, w, max_inst, stats.data_ptr(), meta.data_ptr(), len(exp_points),
                                       points.data_ptr(), stream) == OK
    pts = points.cpu().numpy()
    assert np.array_equal(pts[:len(exp_points)], exp_points) and (pts[len(exp_points):] == sentinel).all()


def test_refusals_launch_nothing():
    from tiatoolbox_amd import _lib

    lib, stream = _lib.load(), _lib.current_stream()
    lab, max_inst, d_inst, stats = _scan_setup()
    n, h, w = lab.shape
    sentinel = 77
    meta = torch.full((n * (max_inst + 1) * 4 + 8,), sentinel, dtype=torch.int32, device="cuda")
    mark = torch.full((n * h * w + 8,), sentinel, dtype=torch.int8, device="cuda")
    total = torch.full((2,), sentinel, dtype=torch.int64, device="cuda")
    points = torch.full((4096, 2), sentinel, dtype=torch.int32, device="cuda")
    good_meta = _dev(_expected("mixed")[0])
    pi, ps, pm, pk, pt, pp, pg = (t.data_ptr() for t in (d_inst, stats, meta, mark, total, points, good_meta))

    def scan(i=pi, n=n, h=h, w=w, k=max_inst, s=ps, mk=pk, m=pm, t=pt):  # noqa: PLR0913
        return lib.tia_hover_contour_scan(i, n, h, w, k, s, mk, m, t, stream)

    assert scan(i=0) == EINVAL and scan(s=0) == EINVAL and scan(mk=0) == EINVAL and scan(m=0) == EINVAL and scan(t=0) == EINVAL
    assert all(scan(**{a: v}) == EINVAL for a in "nhw" for v in (0, -1))
    assert scan(k=-1) == EINVAL

    def write(i=pi, n=n, h=h, w=w, k=max_inst, s=ps, m=pg, cap=2048, p=pp):  # noqa: PLR0913
        return lib.tia_hover_contour_write(i, n, h, w, k, s, m, cap, p, stream)

    assert write(i=0) == EINVAL and write(s=0) == EINVAL and write(m=0) == EINVAL and write(p=0) == EINVAL
    assert all(write(**{a: v}) == EINVAL for a in "nhw" for v in (0, -1))
    assert write(k=-1) == EINVAL and write(cap=-1) == EINVAL
    assert write(cap=0) == OK and write(cap=0, p=0) == OK  # nothing can be written: nothing is launched

    labels = _dev(lab)
    kmax = int(lab.max())
    first = torch.full((n * (kmax + 1) + 8,), sentinel, dtype=torch.int32, device="cuda")
    edge = torch.full((n * (kmax + 1) + 8,), sentinel, dtype=torch.int32, device="cuda")
    pl, pf, pe = labels.data_ptr(), first.data_ptr(), edge.data_ptr()

    def first_pixel(l=pl, n=n, h=h, w=w, k=kmax, f=pf, e=pe):  # noqa: E741, PLR0913
        return lib.tia_label_first_pixel_i32(l, n, h, w, k, f, e, stream)

    assert first_pixel(l=0) == EINVAL and first_pixel(f=0) == EINVAL and first_pixel(e=0) == EINVAL
    assert all(first_pixel(**{a: v}) == EINVAL for a in "nhw" for v in (0, -1))
    assert first_pixel(k=-1) == EINVAL and first_pixel(n=65536) == EINVAL
    assert first_pixel(n=1, h=46341, w=46341) == ESIZE and first_pixel(n=1, h=1, w=2**31) == ESIZE  # h * w > 2^31 - 1

    mask = (labels != 0).to(torch.uint8)
    starts = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
    counts = torch.full((16,), sentinel, dtype=torch.int32, device="cuda")
    offsets = torch.zeros(8, dtype=torch.int64, device="cuda")
    pmk, pst, pc, po = mask.data_ptr(), starts.data_ptr(), counts.data_ptr(), offsets.data_ptr()

    def trace(m=pmk, n=n, h=h, w=w, st=pst, nb=8, c=pc, o=po, cap=2048, p=pp):  # noqa: PLR0913
        return lib.tia_border_trace_u8(m, n, h, w, st, nb, 1, c, o, cap, p, stream)

    assert trace(m=0) == EINVAL and trace(st=0) == EINVAL and trace(c=0) == EINVAL
    assert all(trace(**{a: v}) == EINVAL for a in "nhw" for v in (0, -1))
    assert trace(nb=-1) == EINVAL and trace(o=0) == EINVAL and trace(cap=-1) == EINVAL  # d_points without d_offsets; capacity < 0
    assert trace(nb=0) == OK and trace(nb=0, o=0, p=0) == OK
    torch.cuda.synchronize()
    for name, t in (("meta", meta), ("mark", mark), ("total", total), ("points", points), ("first", first), ("edge", edge), ("counts", counts)):
        assert bool((t == sentinel).all()), name  # no refusal, and no call with nothing to do, launched or set anything

    # the same calls with valid arguments do run
    assert first_pixel() == OK
    f, e = (t.cpu().numpy() for t in (first, edge))
    cells = n * (kmax + 1)
    exp_first = np.full((n, kmax + 1), ref.NO_PIXEL, np.int64)
    exp_edge = np.zeros((n, kmax + 1), np.int64)
    for p in range(n):
        ids, at = np.unique(lab[p], return_index=True)
        exp_first[p, ids[ids > 0]] = at[ids > 0]
        frame = np.concatenate([lab[p][0], lab[p][-1], lab[p][:, 0], lab[p][:, -1]])
        exp_edge[p, np.unique(frame[frame > 0])] = 1
    assert np.array_equal(f[:cells].reshape(n, -1), exp_first) and np.array_equal(e[:cells].reshape(n, -1), exp_edge)
    assert (f[cells:] == sentinel).all() and (e[cells:] == sentinel).all() and (exp_first[1, 1:] == ref.NO_PIXEL).all()
    assert scan() == OK and write(m=pm) == OK
    exp_meta, exp_points = _expected("mixed")
    assert int(total[0]) == len(exp_points) <= 2048 and int(total[1]) == sentinel  # noqa: PLR2004
    got = meta.cpu().numpy()
    assert np.array_equal(got[:exp_meta.size].reshape(exp_meta.shape), exp_meta) and (got[exp_meta.size:] == sentinel).all()
    assert np.array_equal(points.cpu().numpy()[:len(exp_points)], exp_points) and bool((points[len(exp_points):] == sentinel).all())
    assert bool((mark[n * h * w:] == sentinel).all())

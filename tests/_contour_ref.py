"""References and case builders for the contour kernels of ``csrc/contours.hip``.  No GPU here.

THE ORACLE STATEMENT.  Instance polygons: for a label map ``[N, H, W]`` and every (plane, id) with pixels, the polygon is
``cvref.first_contour`` of the id's bounding-box crop plus the crop's top-left corner -- what ``oracle.hovernet.get_instance_info``
computes, kept for EVERY id (the 1- and 2-vertex polygons too).  The ``meta`` row of an entry is start x, start y, vertex count,
offset: the start is the first pixel of the border's CHAIN_APPROX_NONE chain (the raster-first pixel of the chosen component; for a
1-vertex border the polygon's only point), the offset the exclusive prefix sum of the counts in (plane, id) order, to which id 0 and
absent ids contribute 0.  Binary planes: ``cvref.find_contours(mask, simple=...)``.

THE SCIPY STATEMENT of outer borders is independent of ``cvref`` (both ``cvref`` and the kernels restate Suzuki & Abe by one hand):
 * the outer-border pixel set of an 8-connected component S is the pixels of S with a 4-neighbour in the 4-connected background
   region that reaches the frame of the zero-padded plane;
 * a CHAIN_APPROX_SIMPLE polygon expands into a full chain by walking each consecutive vertex pair along its one of 8 directions;
   the expanded chain is a rotation of the CHAIN_APPROX_NONE chain and its pixel set is that outer-border set;
 * the component whose border ``findContours(...)[0][0]`` is, is -- among the 8-connected components that touch the outside
   background of the whole mask -- the one whose raster-first pixel comes last.
It says nothing about hole borders.

Every builder is deterministic; every array it returns is read-only.
"""

from __future__ import annotations

import functools
import re
from pathlib import Path

import numpy as np
from scipy import ndimage

from oracle import cvref

SOURCE = Path(__file__).resolve().parents[1] / "tiatoolbox_amd" / "csrc" / "contours.hip"
NO_PIXEL = 0x7F7F7F7F
EIGHT = np.ones((3, 3), int)
FOUR = ndimage.generate_binary_structure(2, 1)


# ------------------------------------------------------------------------------------------------ constants the cases rest on
@functools.lru_cache(maxsize=1)
def source_constants() -> dict:
    """The sizes the cases are built around, read out of ``contours.hip``; every form in which the source states one must agree."""
    text = SOURCE.read_text()

    def one(pattern: str) -> tuple[int, ...]:
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return tuple(int(v) for v in (found[0] if isinstance(found[0], tuple) else (found[0],)))

    bounds, = one(r"__launch_bounds__\((\d+)\) void contour_offsets_kernel")
    part, = one(r"__shared__ long long part\[(\d+)\]")
    plus, per = one(r"const long chunk = \(entries \+ (\d+)\) / (\d+);")
    launch, = one(r"contour_offsets_kernel, dim3\(1\), dim3\((\d+)\)")
    assert bounds == part == per == launch == plus + 1, (bounds, part, plus, per, launch)
    cap_if, cap_set = one(r"if \(blocks > (\d+)\) blocks = (\d+);")
    fp_bounds, = one(r"__launch_bounds__\((\d+)\) void label_first_pixel_kernel")
    fp_a, fp_b = one(r"\(long\)blockIdx\.x \* (\d+) \+ threadIdx\.x; i < hw; i \+= \(long\)gridDim\.x \* (\d+)\)")
    fp_div_plus, fp_div = one(r"long blocks = \(\(long\)h \* w \+ (\d+)\) / (\d+);")
    fp_launch, = one(r"label_first_pixel_kernel, dim3\(\(unsigned\)blocks, \(unsigned\)n\), dim3\((\d+)\)")
    assert cap_if == cap_set and fp_bounds == fp_a == fp_b == fp_div == fp_launch == fp_div_plus + 1
    ct, = one(r"constexpr int CT = (\d+);")
    return {"offset_threads": bounds, "first_pixel_blocks": cap_if, "first_pixel_threads": fp_bounds, "CT": ct}


def offsets_chunk(entries: int) -> int:
    """Entries per thread of ``contour_offsets_kernel``."""
    t = source_constants()["offset_threads"]
    return (entries + t - 1) // t


def first_pixel_cap() -> int:
    """Pixels of one plane that ``label_first_pixel_kernel`` covers in its first grid-stride trip."""
    c = source_constants()
    return c["first_pixel_blocks"] * c["first_pixel_threads"]


# ------------------------------------------------------------------------------------------------------- the oracle statement
def outer_borders(mask: np.ndarray) -> list[dict]:
    """Every outer border of a binary crop in raster order of discovery: ``simple`` and ``chain`` (CHAIN_APPROX_SIMPLE / NONE points,
    ``(k, 2)`` int32) and ``top`` (its parent is the frame)."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    s = [b for b in cvref.find_contours_tree(m, simple=True) if not b["is_hole"]]
    c = [b for b in cvref.find_contours_tree(m, simple=False) if not b["is_hole"]]
    assert len(s) == len(c)
    return [{"simple": a["points"].astype(np.int32), "chain": b["points"].astype(np.int32), "top": a["parent"] == -1}
            for a, b in zip(s, c)]


def choose_first_contour(borders: list[dict]) -> tuple[np.ndarray, np.ndarray]:
    """``findContours(...)[0][0]``: the top-level outer border discovered last.  Returns (polygon, start pixel)."""
    b = [b for b in borders if b["top"]][-1]
    return b["simple"], b["chain"][0]


def instance_crops(lab: np.ndarray):
    """(plane, id, top-left (x, y), bounding-box crop of ``lab[plane] == id``) for every id with pixels, in (plane, id) order."""
    for p in range(lab.shape[0]):
        for i, sl in enumerate(ndimage.find_objects(lab[p]), start=1):
            if sl is not None:
                yield p, i, np.array([sl[1].start, sl[0].start], np.int32), lab[p][sl] == i


def instance_borders(lab: np.ndarray) -> dict:
    """``{(plane, id): (top-left, outer_borders(crop))}`` for every id with pixels."""
    return {(p, i): (tl, outer_borders(crop)) for p, i, tl, crop in instance_crops(lab)}


def expected_contours(borders: dict, n: int, max_inst: int, choose=choose_first_contour) -> tuple[np.ndarray, np.ndarray]:
    """What ``_hover_device.contours`` must return for the label map that ``borders`` (``instance_borders``) came from:
    ``meta [n, max_inst + 1, 4]`` int32 and ``points [total, 2]`` int32.  Ids above ``max_inst`` do not exist for the kernels."""
    meta = np.zeros((n, max_inst + 1, 4), np.int64)
    polys = []
    for (p, i), (tl, found) in sorted(borders.items()):
        if i > max_inst:
            continue
        poly, start = choose(found)
        meta[p, i, :2] = start + tl
        meta[p, i, 2] = len(poly)
        polys.append(poly + tl)
    counts = meta[..., 2].ravel()
    meta[..., 3] = (np.cumsum(counts) - counts).reshape(n, max_inst + 1)
    points = np.concatenate(polys).astype(np.int32) if polys else np.zeros((0, 2), np.int32)
    return meta.astype(np.int32), points


def compare_contours(meta, points, exp_meta, exp_points, present) -> list[str]:
    """Everything in which ``(meta, points)`` differs from the expected pair: types and shapes, the four ``meta`` columns of EVERY
    entry (absent ids and id 0 included), the grand total, and the slice of ``points`` of every (plane, id) in ``present``."""
    bad = []
    if meta.dtype != np.int32 or points.dtype != np.int32:
        bad.append(f"dtypes {meta.dtype} {points.dtype}")
    if meta.shape != exp_meta.shape or points.ndim != 2 or points.shape[1] != 2:  # noqa: PLR2004
        return [*bad, f"shapes {meta.shape} {points.shape}, expected {exp_meta.shape} {exp_points.shape}"]
    for col, name in enumerate(("start x", "start y", "count", "offset")):
        wrong = np.argwhere(meta[..., col] != exp_meta[..., col])
        if wrong.size:
            p, i = wrong[0]
            bad.append(f"{name}: {len(wrong)} entries differ, first (plane {p}, id {i}): {meta[p, i].tolist()} vs {exp_meta[p, i].tolist()}")
    if len(points) != len(exp_points) or len(points) != int(exp_meta[..., 2].sum()):
        bad.append(f"total {len(points)}, expected {len(exp_points)}")
    seen = 0
    for (p, i) in present:
        if i >= meta.shape[1]:
            continue
        seen += 1
        (_, _, k, off), (_, _, ek, eoff) = meta[p, i].tolist(), exp_meta[p, i].tolist()
        got, exp = points[off:off + k], exp_points[eoff:eoff + ek]
        if got.shape != exp.shape or not np.array_equal(got, exp):
            bad.append(f"polygon (plane {p}, id {i}): {got.tolist()} vs {exp.tolist()}")
    if seen != int((exp_meta[..., 2] > 0).sum()):
        bad.append(f"{seen} polygons compared, {int((exp_meta[..., 2] > 0).sum())} entries have one")
    return bad


# -------------------------------------------------------------------------------------------------------- the scipy statement
def outer_border_set(comp: np.ndarray) -> np.ndarray:
    """Pixels of the 8-connected component ``comp`` (bool) with a 4-neighbour in the 4-connected background region that reaches the
    frame of the zero-padded plane."""
    p = np.pad(np.asarray(comp, bool), 1)
    bg, _ = ndimage.label(~p)
    near = ndimage.binary_dilation(bg == bg[0, 0], structure=FOUR)
    return (near & p)[1:-1, 1:-1]


def expand(poly) -> list[tuple[int, int]]:
    """CHAIN_APPROX_SIMPLE polygon -> every pixel of the closed chain.  Consecutive vertices must lie on one of the 8 directions."""
    poly = [tuple(int(v) for v in p) for p in np.asarray(poly).tolist()]
    if len(poly) == 1:
        return poly
    pts = []
    for (x0, y0), (x1, y1) in zip(poly, poly[1:] + poly[:1]):
        dx, dy = x1 - x0, y1 - y0
        n = max(abs(dx), abs(dy))
        if n == 0 or not (dx == 0 or dy == 0 or abs(dx) == abs(dy)):
            msg = f"vertices {(x0, y0)} -> {(x1, y1)} are not on one of the 8 directions"
            raise ValueError(msg)
        pts += [(x0 + t * int(np.sign(dx)), y0 + t * int(np.sign(dy))) for t in range(n)]
    return pts


def is_rotation(a: list, b: list) -> bool:
    return len(a) == len(b) and (a == b or any(a[r:] + a[:r] == b for r in range(1, len(a))))


def chosen_component(mask: np.ndarray, *, connectivity: int = 8) -> tuple[np.ndarray, tuple[int, int]]:
    """Among the components of ``mask`` that touch the outside background (the 4-connected background region of the zero-padded
    mask that holds its frame), the one whose raster-first pixel is last: ``(component (bool), that pixel (x, y))``."""
    m = np.asarray(mask, bool)
    p = np.pad(m, 1)
    bg, _ = ndimage.label(~p)
    near = ndimage.binary_dilation(bg == bg[0, 0], structure=FOUR)[1:-1, 1:-1]
    comps, k = ndimage.label(m, structure=EIGHT if connectivity == 8 else FOUR)  # noqa: PLR2004
    tops = np.unique(comps[near & m])
    assert k > 0 and tops.size > 0
    first = ndimage.minimum(np.arange(m.size).reshape(m.shape), comps, tops)  # raster-first flat index of each candidate
    c = int(tops[int(np.argmax(first))])
    idx = int(np.max(first))
    return comps == c, (idx % m.shape[1], idx // m.shape[1])


def scipy_mismatches(lab: np.ndarray, meta: np.ndarray, points: np.ndarray) -> list[str]:
    """``(meta, points)`` of ``lab`` against the scipy statement, for every id with pixels: the start pixel is the chosen component's
    raster-first pixel, the polygon expands into a closed chain on the 8 directions, and the chain's pixel set is the component's
    outer-border set."""
    bad = []
    for p, i, tl, crop in instance_crops(lab):
        if i >= meta.shape[1]:
            continue
        comp, (x0, y0) = chosen_component(crop)
        sx, sy, k, off = meta[p, i].tolist()
        if (sx, sy) != (x0 + int(tl[0]), y0 + int(tl[1])):
            bad.append(f"(plane {p}, id {i}) start {(sx, sy)}, scipy {(x0 + int(tl[0]), y0 + int(tl[1]))}")
        try:
            chain = expand(points[off:off + k] - tl)
        except ValueError as e:
            bad.append(f"(plane {p}, id {i}) {e}")
            continue
        got = np.zeros_like(comp)
        inside = [(x, y) for x, y in chain if 0 <= x < comp.shape[1] and 0 <= y < comp.shape[0]]
        for x, y in inside:
            got[y, x] = True
        if k < 1 or len(inside) != len(chain) or not np.array_equal(got, outer_border_set(comp)):
            bad.append(f"(plane {p}, id {i}) chain's pixel set is not the outer-border set")
    return bad


# ------------------------------------------------------------------------------------------------------------ label-map cases
def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def blob_grid(gy: int, gx: int, cell: int = 10, seed: int = 1, n_ids: int | None = None, shape: tuple[int, int] | None = None):
    """``gy x gx`` cells of ``cell`` pixels; cell number ``i`` (1-based, raster order) holds id ``i`` as a random blob in the cell
    minus a one-pixel gutter, at a density drawn from {0.45, 0.6, 0.8, 1.0}.  About a tenth of the cells stay empty (absent ids), and
    so does every cell above ``n_ids``.  ``shape`` pads the plane at the bottom and right."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape or (gy * cell, gx * cell), np.int32)
    i = 0
    for a in range(gy):
        for b in range(gx):
            i += 1
            empty = rng.random() < 0.1  # noqa: PLR2004
            blk = rng.random((cell - 1, cell - 1)) < rng.choice([0.45, 0.6, 0.8, 1.0])
            if not empty and (n_ids is None or i <= n_ids):
                lab[a * cell:a * cell + cell - 1, b * cell:b * cell + cell - 1][blk] = i
    return _frozen(lab)


def _rings(size: int, thick: int) -> np.ndarray:
    """Concentric square rings of one id, ``thick`` pixels thick and ``thick`` apart."""
    a = np.zeros((size, size), bool)
    for k, r in enumerate(range(0, (size + 1) // 2, thick)):
        a[r:size - r, r:size - r] = k % 2 == 0
    return a


def _spiral(k: int) -> np.ndarray:
    """One-pixel-wide square spiral with one-pixel gaps: segment lengths k-1, k-1, k-1, k-3, k-3, k-5, k-5, ..."""
    a = np.zeros((k, k), bool)
    y = x = 0
    a[0, 0] = True
    lengths = [k - 1] + [v for s in range(k - 1, 0, -2) for v in (s, s)]
    for step, n in enumerate(lengths):
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[step % 4]
        for _ in range(n):
            y, x = y + dy, x + dx
            a[y, x] = True
    return a


def adversarial_blocks() -> dict:
    """name -> small int array with local ids 1, 2, ...; each block is one of the named adversarial instances."""
    b = {}
    b["hline"] = np.ones((1, 12), int)
    b["vline"] = np.ones((12, 1), int)
    b["diag"] = np.eye(10, dtype=int)
    b["antidiag"] = np.eye(10, dtype=int)[:, ::-1]
    b["pixel"] = np.ones((1, 1), int)
    b["checker"] = (np.indices((7, 7)).sum(0) % 2 == 0).astype(int)
    b["rings4"] = _rings(28, 4).astype(int)
    b["rings1"] = _rings(9, 1).astype(int)
    isl = np.ones((8, 10), int)
    isl[2:6, 2:6] = 0
    isl[3, 3] = 1
    b["island_in_own_hole"] = isl
    ab = np.ones((7, 7), int)
    ab[1:6, 1:6] = 2
    b["ring_a_filled_by_b"] = ab
    rr = np.zeros((5, 9), int)
    rr[:, :5] = 1
    rr[1:4, 1:4] = 0
    rr[1:4, 7:9] = 1
    b["ring_then_component_on_its_rows"] = rr
    two = np.zeros((4, 8), int)
    two[0, 5:8] = 1
    two[2:4, 0:3] = 1
    b["last_found_starts_further_left"] = two
    b["spiral"] = _spiral(15).astype(int)
    return b


def _pack(lab: np.ndarray, region: tuple[int, int, int, int], names: list[str], next_id: int, where: dict) -> int:
    """Shelf-packs the named blocks into ``lab[y0:y1, x0:x1]`` two pixels apart, with fresh ids; nothing may be overwritten."""
    y0, x0, y1, x1 = region
    blocks = adversarial_blocks()
    y, x, shelf = y0, x0, 0
    for name in names:
        blk = blocks[name]
        bh, bw = blk.shape
        if x + bw > x1:
            y, x, shelf = y + shelf + 2, x0, 0
        assert y + bh <= y1 and x + bw <= x1, (name, "does not fit")
        assert not lab[y:y + bh, x:x + bw].any()
        lab[y:y + bh, x:x + bw] = np.where(blk > 0, blk + next_id - 1, 0)
        where[name] = (list(range(next_id, next_id + int(blk.max()))), (y, x))
        next_id += int(blk.max())
        x, shelf = x + bw + 2, max(shelf, bh)
    return next_id


def _set(lab: np.ndarray, sl, i: int, where: dict, name: str) -> None:
    assert not lab[sl].any(), name
    lab[sl] = i
    where[name] = ([i], None)


@functools.lru_cache(maxsize=None)
def adversarial_plane(kind: str, h: int = 90, w: int = 100):
    """``(label map [h, w] int32, {name: (ids, top-left or None)})``.

    ``"rects"``: filled rectangles on each frame edge and in each corner, and in the interior the thick rings, the spiral, the four
    one-pixel lines and a single pixel.  ``"pixels"``: single pixels at (0, 0) and (w-1, h-1), an S-shaped instance whose bounding
    box is the whole plane, and in its two pockets the thin rings, the checkerboard, the island in its own hole, the ring of A filled
    by B, the component right of a one-pixel ring, and the two components of which the last found starts further left."""
    lab = np.zeros((h, w), np.int32)
    where: dict = {}
    if kind == "rects":
        spots = {"corner_tl": np.s_[0:3, 0:4], "corner_tr": np.s_[0:3, w - 4:w], "corner_bl": np.s_[h - 3:h, 0:4],
                 "corner_br": np.s_[h - 3:h, w - 4:w], "edge_top": np.s_[0:3, 10:15], "edge_bottom": np.s_[h - 3:h, 10:15],
                 "edge_left": np.s_[10:15, 0:3], "edge_right": np.s_[10:15, w - 3:w]}
        for i, (name, sl) in enumerate(spots.items(), start=1):
            _set(lab, sl, i, where, name)
        _pack(lab, (5, 5, h - 5, w - 5), ["rings4", "spiral", "diag", "antidiag", "hline", "vline", "pixel"], len(spots) + 1, where)
    elif kind == "pixels":
        mid = h // 2
        _set(lab, np.s_[0, 0], 1, where, "pixel_at_origin")
        _set(lab, np.s_[h - 1, w - 1], 2, where, "pixel_at_far_corner")
        for sl in (np.s_[0, 2:w], np.s_[0:h - 2, w - 1], np.s_[2:h, 0], np.s_[h - 1, 0:w - 2], np.s_[mid, :]):
            lab[sl] = 3
        where["whole_plane_bbox"] = ([3], None)
        nxt = _pack(lab, (2, 2, mid - 1, w - 2), ["rings1", "checker", "ring_a_filled_by_b", "ring_then_component_on_its_rows"], 4, where)
        _pack(lab, (mid + 2, 2, h - 2, w - 2), ["island_in_own_hole", "last_found_starts_further_left", "pixel"], nxt, where)
    else:
        raise ValueError(kind)
    return _frozen(lab), where


@functools.lru_cache(maxsize=1)
def tiny_label_batches() -> tuple:
    """Label maps of 1 x 1, 1 x W and H x 1 planes (batches of one and two planes)."""
    row = np.array([[1, 1, 0, 2, 0, 3, 3, 3, 4], [0, 5, 5, 5, 5, 5, 5, 5, 0]], np.int32)
    return (_frozen(np.ones((1, 1, 1), np.int32)), _frozen(row[:, None, :].copy()), _frozen(row[:, :, None].copy()))


CHUNK_CASES = (  # name, planes (gy, gx, seed), n_ids, max_inst: entries n * (max_inst + 1) on both sides of the offset kernel's 1024
    ("1023-entries", ((32, 32, 11),), 1022, 1022),
    ("1024-entries", ((32, 32, 12),), 1023, 1023),
    ("1025-entries", ((32, 32, 13),), 1024, 1024),
    ("3x701-entries", ((26, 27, 14), (26, 27, 15), (26, 27, 16)), 700, 700),
    ("3026-entries", ((55, 55, 17),), None, 3025),
)


@functools.lru_cache(maxsize=None)
def chunk_case(name: str) -> tuple[np.ndarray, int]:
    """``(label maps [n, H, W], max_inst)`` of one ``CHUNK_CASES`` row."""
    _, planes, n_ids, max_inst = next(c for c in CHUNK_CASES if c[0] == name)
    return _frozen(np.stack([blob_grid(gy, gx, 10, seed, n_ids) for gy, gx, seed in planes])), max_inst


MIXED_MAX_INST = 120  # above every plane's maximum: the trailing ids are absent everywhere


@functools.lru_cache(maxsize=1)
def mixed_batch() -> np.ndarray:
    """Planes that differ in everything: the two adversarial planes, an empty plane and a blob grid (90 cells)."""
    return _frozen(np.stack([adversarial_plane("rects")[0], np.zeros((90, 100), np.int32), blob_grid(9, 10, 10, 21),
                             adversarial_plane("pixels")[0]]))


@functools.lru_cache(maxsize=None)
def borders_of(case: str) -> dict:
    """``instance_borders`` of a named label-map case, computed once: ``"mixed"``, ``"tiny0..2"`` or a ``CHUNK_CASES`` name."""
    return instance_borders(label_case(case)[0])


def label_case(case: str) -> tuple[np.ndarray, int]:
    if case == "mixed":
        return mixed_batch(), MIXED_MAX_INST
    if case.startswith("tiny"):
        lab = tiny_label_batches()[int(case[4:])]
        return lab, int(lab.max())
    return chunk_case(case)


LABEL_CASES = ("mixed", "tiny0", "tiny1", "tiny2", *(c[0] for c in CHUNK_CASES))


# ---------------------------------------------------------------------------------------------------------- binary-plane cases
@functools.lru_cache(maxsize=1)
def pockets_plane() -> np.ndarray:
    """40 x 52: a hole that touches the frame only diagonally (top-left corner); a background pocket open to the frame through a
    4-connected channel (no hole border); the same pocket with the channel closed diagonally (a hole border)."""
    m = np.zeros((40, 52), np.uint8)
    m[0:3, 0:3] = 1
    m[0, 0] = m[1, 1] = 0          # (1, 1) is a hole: its only way out is the diagonal to the frame pixel (0, 0)
    ring = np.ones((6, 6), np.uint8)
    ring[1:5, 1:5] = 0
    opened, closed = ring.copy(), ring.copy()
    opened[0, 2] = 0                # channel straight up, 4-connected to the outside
    closed[0, 0] = 0                # the corner: the pocket meets the outside by a diagonal only
    m[10:16, 10:16] = opened
    m[10:16, 30:36] = closed
    m[30:36, 46:52] = opened[::-1, ::-1]   # the open pocket again, on the right frame edge and upside down
    return _frozen(m)


@functools.lru_cache(maxsize=1)
def binary_planes() -> dict:
    """name -> uint8 plane.  The kinds of ``test_hip_all_borders_match_suzuki_abe_oracle`` and the new ones."""
    rng = np.random.default_rng(5)
    out = {f"random{p}": (rng.random((40, 52)) < p).astype(np.uint8) for p in (0.3, 0.5, 0.62, 0.8)}
    out["kron"] = np.kron((rng.random((12, 15)) < 0.55).astype(np.uint8), np.ones((3, 4), np.uint8))  # noqa: PLR2004
    out["rings3"] = _rings(41, 3).astype(np.uint8)
    out["full"] = np.ones((9, 11), np.uint8)
    out["empty"] = np.zeros((9, 11), np.uint8)
    out["padded_full"] = np.pad(out["full"], 1)
    out["identity"] = np.eye(13, dtype=np.uint8)
    thin = np.zeros((10, 12), np.uint8)
    thin[2:8, 2] = thin[2:8, 9] = thin[2, 2:10] = thin[7, 2:10] = 1
    out["thin_ring"] = thin
    out["pockets"] = pockets_plane()
    row = np.array([1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1], np.uint8)
    out["1xW"] = row[None, :].copy()
    out["Hx1"] = row[:, None].copy()
    out["1x1"] = np.ones((1, 1), np.uint8)
    return {k: _frozen(v) for k, v in out.items()}


@functools.lru_cache(maxsize=1)
def six_planes() -> np.ndarray:
    """One batch of very different component counts, foreground and background: all-zero, all-one, 0.5 random, nested one-pixel
    rings, the pockets plane, a single pixel."""
    shape = (60, 80)
    rings = np.zeros(shape, np.uint8)
    rings[:39, :39] = _rings(39, 1)
    single = np.zeros(shape, np.uint8)
    single[17, 23] = 1
    pockets = np.zeros(shape, np.uint8)
    pockets[:40, :52] = pockets_plane()   # the corner hole stays in the frame's corner
    random = (np.random.default_rng(6).random(shape) < 0.5).astype(np.uint8)  # noqa: PLR2004
    return _frozen(np.stack([np.zeros(shape, np.uint8), np.ones(shape, np.uint8), random, rings, pockets, single]))


@functools.lru_cache(maxsize=1)
def big_plane() -> np.ndarray:
    """One row more than ``label_first_pixel_kernel`` covers in one trip at width 1024 (1025 x 1024 with the cap of 4096 x 256),
    mostly empty.  The last row is reached by the second trip only: it holds whole components (their first pixels), one of them in
    the corner, and the only frame pixels of a background pocket -- which therefore is no hole only if that trip ran.  Rows 1020 to
    1023 hold the rest of those shapes and a true hole; row 0 and the middle hold more."""
    w = 1024
    h = first_pixel_cap() // w + 1
    m = np.zeros((h, w), np.uint8)
    m[0, :5] = 1
    m[0, 100:103] = 1
    m[500:520, 500:530] = 1
    m[505:510, 505:510] = 0
    m[507, 507] = 1
    m[h - 5:h, 3:9] = 1
    m[h - 3, 5] = 0                  # a true hole
    m[h - 5:h, 20:27] = 1
    m[h - 3:h, 22:25] = 0            # a pocket that opens onto the last row only
    m[h - 1, 40] = 1
    m[h - 1, 500:510] = 1
    m[h - 1, 1000:] = 1
    return _frozen(m)


@functools.lru_cache(maxsize=None)
def expected_borders(name: str, simple: bool) -> list:  # noqa: FBT001
    """``cvref.find_contours`` of a named plane (``binary_planes`` names, ``"big"``, ``"six<i>"``), computed once."""
    if name == "big":
        m = big_plane()
    elif name.startswith("six"):
        m = six_planes()[int(name[3:])]
    else:
        m = binary_planes()[name]
    return [_frozen(b.astype(np.int32)) for b in cvref.find_contours(m, simple=simple)]


def compare_borders(got: list, exp: list) -> list[str]:
    """Same length, same order, every array equal and int32."""
    if len(got) != len(exp):
        return [f"{len(got)} borders, expected {len(exp)}"]
    return [f"border {j}: {a.tolist()[:6]}... vs {b.tolist()[:6]}..." for j, (a, b) in enumerate(zip(got, exp))
            if a.dtype != np.int32 or a.shape != b.shape or not np.array_equal(a, b)]

"""NumPy statement of the canvas stitching (``tia_canvas_row_merge_f32`` / ``tia_canvas_finalize_f32``) for the tests, written from
the specification alone: it imports nothing from the package and nothing from ``oracle/``.  Also the case lists that the host and
the device tests share, so that what the host tests prove about a list (its depth, its wraps, its NaN ties) holds for the very
data the device sees.

The contract is NumPy's: float32 added to float32 one block at a time in the order given, a ``uint8`` count that wraps, one float32
division by ``where(count == 0, 1, count)``, ``np.argmax`` for the label (the first NaN wins, else the first maximum)."""

from __future__ import annotations

import numpy as np

U = 2.0 ** -24  # unit round-off of float32


# ------------------------------------------------------------------------------------------------ the statement
def row_merge_ref(blocks, xs, width: int):
    """``(row [oh, width, c] float32, cnt [oh, width] uint8)``: the blocks of one patch row added at their left edges ``xs`` IN THE
    ORDER GIVEN; a block with ``not np.any(block)`` is skipped for sum and count alike; columns are clipped at ``width``."""
    blocks = np.asarray(blocks, dtype=np.float32)
    _, oh, ow, c = blocks.shape
    row = np.zeros((oh, width, c), dtype=np.float32)
    cnt = np.zeros((oh, width), dtype=np.uint8)
    for block, x in zip(blocks, xs):
        if not np.any(block):
            continue
        x0, x1 = max(int(x), 0), min(int(x) + ow, width)
        if x1 <= x0:
            continue
        row[:, x0:x1] = row[:, x0:x1] + block[:, x0 - int(x):x1 - int(x)]
        cnt[:, x0:x1] += np.uint8(1)  # uint8: wraps at 256
    return row, cnt


def finalize_ref(row_a, cnt_a, ys_a: int, row_b, cnt_b, ys_b: int, oh: int, y0: int, y1: int):
    """``(probs [y1 - y0, width, c] float32, pred [y1 - y0, width] uint8)`` of canvas rows ``[y0, y1)``: patch row ``a`` covers
    canvas rows ``[ys_a, ys_a + oh)``, ``b`` (may be ``None``) ``[ys_b, ys_b + oh)``; outside its rows a patch row contributes
    nothing.  Counts are added in uint8, sums ``a + b`` in float32, then one float32 division; the label is ``np.argmax``."""
    width, c = row_a.shape[1:]
    total = np.zeros((y1 - y0, width, c), dtype=np.float32)
    count = np.zeros((y1 - y0, width), dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(y0, y1):
            ya, yb = y - ys_a, y - ys_b
            if 0 <= ya < oh:
                total[y - y0] = row_a[ya]
                count[y - y0] = cnt_a[ya]
            if row_b is not None and 0 <= yb < oh:
                total[y - y0] = total[y - y0] + row_b[yb]
                count[y - y0] += cnt_b[yb]  # uint8 + uint8: wraps
        divisor = np.where(count == 0, 1, count).astype(np.float32)
        probs = total / divisor[..., None]
    return probs, np.argmax(probs, -1).astype(np.uint8)


def row_ys_of(locs) -> np.ndarray:
    return np.unique(np.asarray(locs).reshape(-1, 4)[:, 1])


def stitch_ref(blocks, locs, shape):
    """``(probs [h, w, c] float32, pred [h, w] uint8)``: the two functions above composed the way the engines compose them.  Per
    patch row (ascending ``ys``, its blocks in the order given) a row merge; canvas rows ``[ys, min(next ys, h))`` -- the last
    row: ``[ys, min(ys + oh, h))`` -- are finalised from the previous and the current patch row.  ``ValueError`` where a third
    patch row reaches a canvas row: two is all the composition (and the reference) can add."""
    h, w = shape
    blocks = np.asarray(blocks, dtype=np.float32)
    locs = np.asarray(locs).reshape(-1, 4)
    oh, c = blocks.shape[1], blocks.shape[3]
    row_ys = row_ys_of(locs)
    for i in range(len(row_ys) - 2):
        if row_ys[i + 2] < row_ys[i] + oh:
            msg = f"patch rows at y = {row_ys[i]}, {row_ys[i + 1]} and {row_ys[i + 2]} all cover canvas row {row_ys[i + 2]}"
            raise ValueError(msg)
    probs = np.zeros((h, w, c), dtype=np.float32)
    pred = np.zeros((h, w), dtype=np.uint8)
    prev = None
    for i, ys in enumerate(int(v) for v in row_ys):
        sel = np.flatnonzero(locs[:, 1] == ys)
        row, cnt = row_merge_ref(blocks[sel], locs[sel, 0], w)
        y1 = min(int(row_ys[i + 1]) if i + 1 < len(row_ys) else ys + oh, h)
        if y1 > ys:
            if prev is None:
                probs[ys:y1], pred[ys:y1] = finalize_ref(row, cnt, ys, None, None, 0, oh, ys, y1)
            else:
                probs[ys:y1], pred[ys:y1] = finalize_ref(prev[0], prev[1], prev[2], row, cnt, ys, oh, ys, y1)
        prev = (row, cnt, ys)
    return probs, pred


def wide_ref(blocks, locs, shape):
    """The same sums in float64 from the same float32 inputs, block by block straight into the canvas (no patch rows, so it shares
    no structure with ``stitch_ref``): ``(total64, quotient64, bound, depth)``.  ``depth`` d = the number of terms of an element,
    S = the float64 sum of their magnitudes, the divisor the statement's own (``d mod 256``, 1 where that is 0: a rule, not an
    error).  The float32 statement makes d - 1 additions and one division, each rounded once, so per element
    ``|ref32 - quotient64| <= bound = d * 2^-24 * S / divisor`` -- plus half a subnormal step where the quotient underflows;
    derived, not measured.  For the sums before the division the same reasoning gives ``(d - 1) * 2^-24 * S <= bound * divisor``."""
    h, w = shape
    blocks = np.asarray(blocks, dtype=np.float32)
    locs = np.asarray(locs).reshape(-1, 4)
    oh, ow, c = blocks.shape[1:]
    total = np.zeros((h, w, c), dtype=np.float64)
    mag = np.zeros((h, w, c), dtype=np.float64)
    depth = np.zeros((h, w), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for block, (x, y) in zip(blocks, locs[:, :2].tolist()):
            if not np.any(block):
                continue
            x0, x1, y0, y1 = max(x, 0), min(x + ow, w), max(y, 0), min(y + oh, h)
            if x1 <= x0 or y1 <= y0:
                continue
            part = block[y0 - y:y1 - y, x0 - x:x1 - x].astype(np.float64)
            total[y0:y1, x0:x1] += part
            mag[y0:y1, x0:x1] += np.abs(part)
            depth[y0:y1, x0:x1] += 1
        divisor = np.where(depth % 256 == 0, 1, depth % 256).astype(np.float64)[..., None]
        return total, total / divisor, depth[..., None] * U * mag / divisor + 2.0 ** -150, depth


def within_wide(got32, blocks, locs, shape, *, divided: bool = True) -> bool:
    """``got32`` (the float32 statement's quotients, or its undivided sums) lies within ``wide_ref``'s bound of the float64 value
    wherever that is finite, and is non-finite exactly where it is not."""
    total, quotient, bound, depth = wide_ref(blocks, locs, shape)
    exact = quotient if divided else total
    if not divided:
        bound = bound * np.where(depth % 256 == 0, 1, depth % 256)[..., None]
    finite = np.isfinite(exact)
    if not np.array_equal(np.isfinite(got32), finite):
        return False
    return bool(np.all(np.abs(got32.astype(np.float64) - exact)[finite] <= bound[finite]))


def gt_scan_argmax(values) -> np.ndarray:
    """The label a ``k == 0 or v > best`` scan gives (what ``np.argmax`` is NOT, with a NaN): for the tests that show the
    difference."""
    values = np.asarray(values)
    best = np.zeros(values.shape[:-1], dtype=np.uint8)
    bestv = values[..., 0].copy()
    for k in range(1, values.shape[-1]):
        with np.errstate(invalid="ignore"):
            take = values[..., k] > bestv
        best[take] = k
        bestv[take] = values[..., k][take]
    return best


def row_locs(xs, oh: int, ow: int) -> np.ndarray:
    """``[x0, 0, x1, oh]`` of the blocks of one patch row at canvas row 0."""
    xs = np.asarray(xs, dtype=np.int64)
    return np.stack([xs, np.zeros_like(xs), xs + ow, np.full_like(xs, oh)], axis=-1)


def grid_locs(h: int, w: int, oh: int, ow: int, sy: int, sx: int) -> np.ndarray:
    """Output bounds of a patch grid: from 0 at stride ``(sy, sx)``, ``ceil(dim / stride)`` per axis, x fastest."""
    return np.array([[x, y, x + ow, y + oh] for y in range(0, -(-h // sy) * sy, sy) for x in range(0, -(-w // sx) * sx, sx)],
                    dtype=np.int64)


# ------------------------------------------------------------------------------------------------ row-merge case lists
def _normal(rng, shape) -> np.ndarray:
    return rng.standard_normal(shape).astype(np.float32)  # N(0, 1): signed, like HoVer-Net's hv maps


def channel_cases() -> dict:
    """``name -> (blocks [n, oh, ow, c], xs, width)``: every channel count the kernel has registers for at ``(oh, ow, width) =
    (5, 12, 53)`` with blocks at x stride 5 (three deep), the first at ``x = 0``; the tenth block (x = 45) hangs over the right
    edge, which nine blocks of 12 columns at stride 5 do not reach.  Then a canvas one column wide, one-pixel blocks, and a block
    wider than the canvas."""
    rng = np.random.default_rng(41)
    cases = {f"c{c}": (_normal(rng, (10, 5, 12, c)), np.arange(10) * 5, 53) for c in range(1, 9)}
    cases["width1"] = (_normal(rng, (3, 3, 7, 2)), np.array([0, 0, 0]), 1)
    cases["pixel_blocks"] = (_normal(rng, (4, 1, 1, 3)), np.array([0, 3, 3, 8]), 9)
    cases["wider_than_canvas"] = (_normal(rng, (2, 2, 40, 2)), np.array([0, 5]), 17)
    return cases


DEEP_XS = np.array([20, 0, 10, 5, 15, 24])


def deep_case():
    """Six shuffled blocks of 16 columns on 40, four deep: the order of the additions shows in the last bit."""
    return _normal(np.random.default_rng(42), (6, 4, 16, 3)), DEEP_XS, 40


ZERO_KINDS = ("plus_zero", "minus_zero", "subnormal", "nan")
ZERO_XS = np.array([0, 1, 0, 2, 0])  # five blocks of three columns: all of them cover column 2


def zero_case(kind: str, c: int):
    """A stack of five over column 2 whose THIRD block is all ``+0.0`` / all ``-0.0`` (skipped: neither summed nor counted) / zero
    but for one ``2^-149`` / zero but for one NaN (both count: ``np.any`` is true)."""
    blocks = _normal(np.random.default_rng(43 + c), (5, 2, 3, c))
    third = np.zeros((2, 3, c), dtype=np.float32)
    if kind == "minus_zero":
        third[:] = -0.0
    elif kind == "subnormal":
        third[1, 2, c - 1] = np.float32(2.0 ** -149)
    elif kind == "nan":
        third[0, 1, 0] = np.nan
    blocks[2] = third
    return blocks, ZERO_XS, 5


def wrap_case(n: int):
    """``n`` blocks of ``(2, 3, 1)`` at ``x = 0`` on five columns: 300 of them count to 44, 256 to exactly 0."""
    return _normal(np.random.default_rng(n), (n, 2, 3, 1)), np.zeros(n, dtype=np.int64), 5


GRID_STRIDE_WIDTH = 2_100_000  # 2 rows of it: more elements than the launcher's 16384 workgroups of 256 threads


def grid_stride_case():
    """Three blocks of 64 columns on a row of 2.1 million: the first, one in the middle, one hanging over the end."""
    return _normal(np.random.default_rng(44), (3, 2, 64, 1)), np.array([0, 1_000_000, GRID_STRIDE_WIDTH - 30]), GRID_STRIDE_WIDTH


def row_merge_cases() -> dict:
    """Every row-merge case of the small kind, by name."""
    cases = dict(channel_cases())
    cases["deep"] = deep_case()
    for kind in ZERO_KINDS:
        for c in (1, 4):
            cases[f"zero_{kind}_c{c}"] = zero_case(kind, c)
    cases["wrap300"] = wrap_case(300)
    cases["wrap256"] = wrap_case(256)
    return cases


# ------------------------------------------------------------------------------------------------ whole-canvas case lists
def stitch_cases() -> dict:
    """``name -> (blocks, locs, (h, w))``, all with at most two patch rows over a canvas row: rows two deep and columns four deep
    with masked (all-zero) blocks -- the whole first patch row, one middle row, patches inside rows --, no overlap at all with
    signed one-channel values, and an odd stride with a clipped last row and column."""
    rng = np.random.default_rng(45)
    cases = {}
    locs = grid_locs(70, 96, 16, 16, 8, 5)
    blocks = _normal(rng, (len(locs), 16, 16, 3))
    rows = row_ys_of(locs)
    drop = (locs[:, 1] == rows[0]) | (locs[:, 1] == rows[4]) | (rng.random(len(locs)) < 0.2)
    blocks[drop] = 0.0
    cases["two_by_four_deep_masked"] = (blocks, locs, (70, 96))
    locs = grid_locs(40, 50, 16, 16, 16, 16)
    cases["no_overlap_c1"] = (_normal(rng, (len(locs), 16, 16, 1)), locs, (40, 50))
    locs = grid_locs(45, 37, 16, 16, 11, 9)
    cases["odd_stride_c2"] = (_normal(rng, (len(locs), 16, 16, 2)), locs, (45, 37))
    return cases


# ------------------------------------------------------------------------------------------------ finalize case lists
FIN_OH, FIN_WIDTH, FIN_YS_A = 6, 11, 4
FIN_OFFSETS = (1, 3, 5, 6, 9)  # ys_b - ys_a: overlaps of 5, 3 and 1 rows, none (HoVer-Net's 164 / 164), a gap of 3 rows


def finalize_geometry_cases(c: int) -> list:
    """Dicts of ``finalize_ref``'s arguments (+ ``name``) at ``c`` channels, ``oh = 6``, ``width = 11``: for every row offset the
    engine's two ranges (``[ys_b, ys_b + offset)`` of a middle row, ``[ys_b, ys_b + oh)`` of the last), a strict sub-range, the
    whole span of both rows (rows of ``a`` alone, of both, of ``b`` alone and, at offset 9, of neither), a range that ends at
    ``ys_b`` and the first-row call without ``b``.  Counts 0 .. 3, so some pixels divide by 1 with nothing under them."""
    rng = np.random.default_rng(100 + c)
    cases = []
    for off in FIN_OFFSETS:
        ys_a, ys_b = FIN_YS_A, FIN_YS_A + off
        rows = {k: _normal(rng, (FIN_OH, FIN_WIDTH, c)) for k in "ab"}
        cnts = {k: rng.integers(0, 4, (FIN_OH, FIN_WIDTH)).astype(np.uint8) for k in "ab"}
        ranges = {"middle": (ys_b, ys_b + min(off, FIN_OH)), "last": (ys_b, ys_b + FIN_OH), "sub": (ys_b + 1, ys_b + FIN_OH - 2),
                  "span": (ys_a, ys_b + FIN_OH), "ends_at_b": (ys_a, ys_b)}
        for tag, (y0, y1) in ranges.items():
            cases.append({"name": f"c{c}_off{off}_{tag}", "row_a": rows["a"], "cnt_a": cnts["a"], "ys_a": ys_a, "row_b": rows["b"],
                          "cnt_b": cnts["b"], "ys_b": ys_b, "oh": FIN_OH, "y0": y0, "y1": y1})
        cases.append({"name": f"c{c}_off{off}_no_b", "row_a": rows["a"], "cnt_a": cnts["a"], "ys_a": ys_a, "row_b": None, "cnt_b": None,
                      "ys_b": 0, "oh": FIN_OH, "y0": ys_a, "y1": ys_a + FIN_OH})
    return cases


def finalize_count_cases() -> list:
    """Counts no real merge reaches cheaply: 200 + 100 wraps to 44, 156 + 100 to exactly 0 (divisor 1), and 0 + 0."""
    rng = np.random.default_rng(46)
    cases = []
    for name, ca, cb in (("wrap44", 200, 100), ("wrap0", 156, 100), ("zero", 0, 0)):
        cases.append({"name": f"count_{name}", "row_a": _normal(rng, (3, 7, 3)) * 50, "cnt_a": np.full((3, 7), ca, np.uint8), "ys_a": 0,
                      "row_b": _normal(rng, (3, 7, 3)) * 50, "cnt_b": np.full((3, 7), cb, np.uint8), "ys_b": 0, "oh": 3, "y0": 0, "y1": 3})
    return cases


_NAN, _INF = np.nan, np.inf
LABEL_VECTORS = np.array([
    [0.5, 0.5, 0.1, 0.5],          # exact ties: the first wins
    [0.1, 0.7, 0.7, 0.2],
    [0.0, -0.0, -1.0, -1.0],       # +0.0 against -0.0: equal, the first wins
    [-0.0, 0.0, -1.0, -1.0],
    [-3.0, -1.0, -2.0, -1.0],      # all negative, as in an hv map
    [1.0, _INF, _INF, -_INF],
    [-_INF, -_INF, -_INF, -_INF],
    [0.2, _NAN, 0.9, 0.1],         # a NaN in channel k > 0: np.argmax says 1, a > scan 2
    [0.2, 0.9, _NAN, _NAN],        # NaNs in two channels: the first of them
    [_NAN, 0.9, 1.0, 2.0],         # a NaN in channel 0
    [_NAN, _NAN, _NAN, _NAN],
    [0.9, 0.1, _NAN, 0.95],        # a NaN between a maximum and a larger one
    [-_INF, _NAN, _INF, 0.0],
], dtype=np.float32)


def finalize_label_cases() -> list:
    """``LABEL_VECTORS`` as the pixels of one patch row: alone with count 1, alone with count 3 (divided), and with a second
    patch row under them whose ``+inf`` meets a ``-inf`` (a NaN made by the addition itself)."""
    n = len(LABEL_VECTORS)
    row = np.ascontiguousarray(np.broadcast_to(LABEL_VECTORS, (2, n, 4)))
    one = np.ones((2, n), np.uint8)
    row_b = np.zeros((2, n, 4), dtype=np.float32)
    row_b[:, 5] = [0.0, -_INF, 1.0, _INF]
    row_b[:, 4] = [2.0, 0.0, 1.0, 0.0]
    base = {"row_a": row, "ys_a": 0, "ys_b": 0, "oh": 2, "y0": 0, "y1": 2}
    return [{**base, "name": "labels_alone", "cnt_a": one, "row_b": None, "cnt_b": None},
            {**base, "name": "labels_divided", "cnt_a": one * 3, "row_b": None, "cnt_b": None},
            {**base, "name": "labels_two_rows", "cnt_a": one, "row_b": row_b, "cnt_b": one}]


def finalize_cases() -> list:
    cases = [case for c in range(1, 9) for case in finalize_geometry_cases(c)]
    return cases + finalize_count_cases() + finalize_label_cases()


def finalize_args(case: dict) -> tuple:
    return tuple(case[k] for k in ("row_a", "cnt_a", "ys_a", "row_b", "cnt_b", "ys_b", "oh", "y0", "y1"))

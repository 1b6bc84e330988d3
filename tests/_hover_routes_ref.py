"""CPU helpers of the HoVer-Net post-processing route tests: which kernel set ``hover_proc_impl`` (``csrc/hover_post.hip``) picks
for a plane, the table of shapes that reaches every one of them, and hand-made head maps for planes too thin for ``synth_maps``.

``route`` restates the conditions of ``hover_proc_impl``::

    tile          = ccl_tile_enabled() && h*w <= kCclTileMaxPixels
    band_rows_max = (144 * 1024) / (w * 12) - (ksize - 1)
    fused         = tile && h*w <= kMarkerTileMaxPixels && band_rows_max >= 8
    tile_sobel    = tile && band_rows_max >= 8

    A "fused"        fused                                      tile labelling, tile Sobel (+ Gaussian), marker_tile (+ watershed state)
    B "wide rows"    tile, h*w <= 32000, band_rows_max < 8      tile labelling, stand-alone Sobel / energy / Gaussian, marker_tile
    C "middle"       32000 < h*w <= 36864, band_rows_max >= 8   tile labelling, tile Sobel (dist == nullptr) + gauss3_neg, multi-launch markers
    D "multi-launch" h*w > 36864                                every stage in its stand-alone kernels
    E "wide middle"  32000 < h*w <= 36864, band_rows_max < 8    tile labelling, stand-alone Sobel / energy / Gaussian, multi-launch markers

(E is the one mix of the same conditions that is none of A-D.)  ``tests/test_hovernet_post_routes.py`` reads the constants out
of the sources and fails if one of them moves, so that the table cannot silently send every case down one route.
"""

from __future__ import annotations

import math

import numpy as np

CCL_TILE_MAX_PIXELS = 36864      # kCclTileMaxPixels (csrc/common.hpp)
MARKER_TILE_MAX_PIXELS = 32000   # kMarkerTileMaxPixels (csrc/common.hpp)
SOBEL_LDS_BYTES = 144 * 1024     # the tile Sobel kernel's dynamic LDS
SOBEL_LDS_BYTES_PER_PIXEL = 12   # f64 row-pass band + f32 input band
MIN_BAND_ROWS = 8

# scale_factor of ``_proc_np_hv`` -> the odd Sobel size ``int(20 * scale + 1)`` it is meant to give
KSIZE_OF_SCALE = {1: 21, 0.5: 11, 0.2: 5, 0.3: 7, 0.7: 15, 1.5: 31}
TEMPLATED_KSIZES = (21, 11)      # sobel_energy_tile_kernel<21> / <11>; every other size runs <0>


def ksize_of(scale: float) -> int:
    return int((20 * scale) + 1)    # hovernet.py:566, as the oracle writes it


def obj_size_of(scale: float) -> int:
    return math.ceil(10 * (scale**2))


def band_rows_max(w: int, ksize: int) -> int:
    return SOBEL_LDS_BYTES // (w * SOBEL_LDS_BYTES_PER_PIXEL) - (ksize - 1)


def route(h: int, w: int, ksize: int) -> str:
    hw = h * w
    if hw > CCL_TILE_MAX_PIXELS:
        return "D"
    banded = band_rows_max(w, ksize) >= MIN_BAND_ROWS
    if hw <= MARKER_TILE_MAX_PIXELS:
        return "A" if banded else "B"
    return "C" if banded else "E"


# (route, h, w, scale).  The smallest planes that still select the route, both sides of every threshold:
#   band_rows_max 8 | 7:  72 x 438 | 72 x 439 (21),  46 x 682 | 46 x 683 (11),  96 x 323 | 96 x 324 (31)
#   h*w 32000 | 32001:    160 x 200 | 10667 x 3       h*w 36864 | 36865:  192 x 192 | 365 x 101
ROUTE_CASES = (
    ("A", 96, 120, 1), ("A", 96, 120, 0.2), ("A", 96, 120, 0.3), ("A", 96, 120, 0.7), ("A", 96, 120, 1.5),
    ("A", 181, 176, 1), ("A", 72, 438, 1), ("A", 160, 200, 1), ("A", 46, 682, 0.5), ("A", 96, 323, 1.5),
    ("B", 24, 440, 1), ("B", 40, 700, 1), ("B", 72, 439, 1), ("B", 40, 700, 0.5), ("B", 46, 683, 0.5), ("B", 96, 324, 1.5),
    ("C", 180, 200, 1), ("C", 190, 190, 1), ("C", 192, 192, 1), ("C", 10667, 3, 1), ("C", 180, 200, 0.5), ("C", 180, 200, 0.3),
    ("D", 193, 192, 1), ("D", 2, 18433, 1), ("D", 365, 101, 1), ("D", 193, 192, 0.5), ("D", 193, 192, 0.2),
    ("E", 48, 700, 1),
)

# planes with h <= ksize / 2 or w <= ksize / 2 (the tile kernel's general reflection), and their neighbours on the other side:
# 10 | 11 rows for ksize 21 (anchor 10), 5 | 6 rows for ksize 11 (anchor 5)
TINY_SHAPES = ((7, 50), (50, 9), (10, 40), (11, 40), (5, 40), (6, 40), (2, 300), (1, 64), (64, 1), (3, 3), (1, 1))
# of those, the ones that can hold a blob of 10 pixels and, with tiny_maps' seed below, do
TINY_NONEMPTY = ((7, 50), (50, 9), (10, 40), (11, 40), (5, 40), (6, 40), (2, 300), (1, 64), (64, 1))
TINY_SEED = 42

SYNTH_MIN_SIDE = 9   # hover_head_maps draws blob centres from uniform(4, side - 4)


def tiny_maps(n: int, h: int, w: int, seed: int = TINY_SEED):
    """Hand-made ``(np [n,h,w,1], hv [n,h,w,2])`` float32 head maps for any ``h, w >= 1``: ``np`` random at about 80 % foreground,
    ``hv`` one tanh ramp per axis (h along x, v along y) plus a little noise."""
    rng = np.random.default_rng(seed)
    fg = rng.random((n, h, w, 1)) < 0.8
    np_map = np.where(fg, rng.uniform(0.6, 1.0, fg.shape), rng.uniform(0.0, 0.4, fg.shape)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    hv = np.empty((n, h, w, 2), np.float64)
    hv[..., 0] = np.tanh((xx - (w - 1) / 2) / max(w / 4, 1.0))
    hv[..., 1] = np.tanh((yy - (h - 1) / 2) / max(h / 4, 1.0))
    hv += rng.normal(0, 0.02, hv.shape)
    return np_map, hv.astype(np.float32)


def case_maps(n: int, h: int, w: int, seed: int):
    """Head maps of a ``ROUTE_CASES`` row: ``synth_maps`` where it accepts the shape, ``tiny_maps`` for the long thin planes."""
    if min(h, w) < SYNTH_MIN_SIDE:
        return tiny_maps(n, h, w, seed)
    from oracle import hovernet as oh

    npm, hv, _ = oh.synth_maps(n, h, w, seed=seed, n_blobs=max(3, h * w // 450))
    return npm, hv

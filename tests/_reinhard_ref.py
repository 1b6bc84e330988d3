"""Host-only side of tests/test_reinhard_routes_gpu.py: which kernel of csrc/lab.hip a shape reaches, the shapes that walk every one
of them, the hard inputs, and the oracle's results (``oracle.stain`` Reinhard on ``oracle.cvref``; computed once per case and shared)."""

from __future__ import annotations

import numpy as np

from oracle import cvref
from oracle import stain as ostain
from tiatoolbox_amd.utils import synth

# ---- the dispatch, restated -------------------------------------------------------------------------------------------------------
# KEEP IN STEP with tiatoolbox_amd/csrc/lab.hip: `resident_ok` / `scratch_ok` (lab.hip:823-824), `need` and the TIA_RESIDENT ladder of
# `launch_resident` (lab.hip:835-856), the 4-byte pointer test of tia_reinhard_transform_u8 / tia_lab_moments_u8, and `wide_ok`
# (hw % kPxChunk == 0 and 16-byte aligned bases) of the three streaming kernels.  Whoever edits one edits the other.
LADDER = (1, 2, 4, 6, 8, 10, 13, 16)   # NG of reinhard_resident_kernel<NG, .>
RESIDENT_THREADS = 1024                # a thread owns the 4-pixel groups t, t + 1024, ...
RESIDENT_MAX_PIXELS = 16 * 4096
FUSED_MAX_PIXELS = 1 << 18
FUSED_STEP_PIXELS = 256                # one wave step of reinhard_fused_kernel: 64 lanes x 4 pixels
FUSED_WAVES = 4
WIDE_CHUNK_PIXELS = 1024


def need(h: int, w: int) -> int:
    """4-pixel groups the busiest thread of the register-resident kernel owns: ceil((hw / 4) / 1024)."""
    return -(-((h * w) >> 2) // RESIDENT_THREADS)


def route(h: int, w: int, aligned: bool = True, *, align: int | None = None) -> tuple[str, int | None]:  # noqa: FBT001, FBT002
    """``("resident", NG)``, ``("fused", None)``, ``("three_wide", None)`` or ``("three_scalar", None)`` for an ``h x w`` image whose
    batch base is 16-byte aligned (``aligned``), byte aligned (``not aligned``), or aligned to ``align`` bytes."""
    a = align if align is not None else (16 if aligned else 1)
    hw = h * w
    if a % 4 == 0:
        if hw % 4 == 0 and hw <= RESIDENT_MAX_PIXELS:
            return "resident", next(g for g in LADDER if g >= need(h, w))
        if hw % FUSED_STEP_PIXELS == 0 and hw <= FUSED_MAX_PIXELS:
            return "fused", None
    return ("three_wide" if hw % WIDE_CHUNK_PIXELS == 0 and a % 16 == 0 else "three_scalar"), None


# ---- the shapes -------------------------------------------------------------------------------------------------------------------
# Per kernel: the smallest shape, shapes whose last group of a thread is ragged or wholly idle (need < NG), the full one.
SHAPES: dict[tuple[str, int | None], list[tuple[int, int]]] = {
    ("resident", 1): [(1, 4), (2, 6), (64, 64)],            # one group on one thread; three groups; every thread one group
    ("resident", 2): [(72, 72), (64, 128)],                 # need 2 with a ragged second group; full
    ("resident", 4): [(96, 96), (128, 128)],                # need 3: the whole fourth group idle; full
    ("resident", 6): [(4, 4097), (128, 192)],               # need 5 with ONE group in the fifth; full
    ("resident", 8): [(160, 176), (128, 256)],              # need 7; full
    ("resident", 10): [(192, 192), (200, 200)],             # need 9 exactly; need 10 ragged
    ("resident", 13): [(208, 208), (224, 224)],             # need 11; need 13 ragged
    ("resident", 16): [(236, 236), (240, 240), (256, 256)],  # need 14, 15, 16 (full: the upper limit)
    # 257 / 258 / 259 wave steps: every remainder but 0 modulo the 4 waves (320 x 320 = 400 steps has remainder 0); the upper limit
    ("fused", None): [(257, 256), (258, 256), (259, 256), (320, 320), (384, 384), (512, 512)],
    # % 4 but above the resident limit and not % 256; one step past the fused limit and not % 1024
    ("three_scalar", None): [(1, 3), (37, 53), (16385, 4), (1025, 256)],
    ("three_wide", None): [(257, 1024)],                    # the smallest (1024 x 1536 is in test_reinhard.py)
}
ALL_SHAPES = [s for shapes in SHAPES.values() for s in shapes]
ZERO_STD_SHAPES = [(64, 64), (256, 256), (320, 320), (37, 53), (257, 1024)]   # one per route
FLAT_SHAPE = (320, 320)
TINY_PIXELS = 16    # up to here (1x4, 2x6, 1x3, the 3x3 of the chunking test) an image has no room for bands: seeded noise

# the eight 255/0 combinations: black, the primaries, the secondaries, white -- a / b at their extremes, the byte dot products at
# their largest
SATURATED = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.uint8)


def batch(h: int, w: int, n: int = 3) -> np.ndarray:
    """uint8 ``[n, h, w, 3]``: synthetic H&E with, in image 0, a flat white band (every lane on one histogram counter) and a band of
    near-black pixels 0..11 (the cube's linear branch); in image 1 runs of the saturated colours; in the last image uniform noise
    over the left half.  Images too small for bands are seeded noise (all three Lab stds non-zero: asserted by the host tests)."""
    rng = np.random.default_rng(1000003 * h + 7 * w + n)
    if h * w <= TINY_PIXELS:
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    imgs = synth.g_he(n, h, w, seed=h + w)
    band = max(1, h // 8)
    imgs[0, : h // 3] = 255
    imgs[0, h // 3: h // 3 + band] = rng.integers(0, 12, imgs[0, h // 3: h // 3 + band].shape, dtype=np.uint8)
    flat = imgs[1].reshape(-1, 3)
    cnt = max(8, (h * w) // 4)
    flat[-cnt:] = SATURATED[(np.arange(cnt) * 8) // cnt]
    imgs[-1, :, : w // 2] = rng.integers(0, 256, (h, w // 2, 3), dtype=np.uint8)
    return imgs


def grey_ramp(h: int, w: int) -> np.ndarray:
    """R == G == B ramp: a == b == 128 on every pixel (zero std of both, L's std is not zero)."""
    v = (np.arange(h * w) % 256).astype(np.uint8).reshape(h, w)
    return np.repeat(v[..., None], 3, axis=2)


def flat_image(h: int, w: int, value: int = 200) -> np.ndarray:
    return np.full((h, w, 3), value, np.uint8)


def zero_std_batch(h: int, w: int, middle: np.ndarray) -> np.ndarray:
    """Three images, the degenerate one in the MIDDLE: the flag must land on image 1 alone."""
    imgs = batch(h, w, 3)
    imgs[1] = middle
    return imgs


# ---- the oracle, once per case ----------------------------------------------------------------------------------------------------
_REF: list = []
_CACHE: dict[tuple, tuple[np.ndarray, np.ndarray]] = {}


def oracle(target: np.ndarray) -> ostain.ReinhardNormalizer:
    """The oracle's normaliser fitted to the suite's target image (one per process)."""
    if not _REF:
        ref = ostain.get_normalizer("reinhard")
        ref.fit(target.copy())
        _REF.append(ref)
    return _REF[0]


def reference(ref, imgs: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(transform ``[n,h,w,3]`` uint8, ``[n,6]`` float64 means then stds) of the oracle, image by image."""
    out = np.stack([ref.transform(i.copy()) for i in imgs])
    ms = np.array([np.concatenate(ref.get_mean_std(i.copy())) for i in imgs], dtype=np.float64)
    return out, ms


def expected(target: np.ndarray, h: int, w: int, n: int = 3) -> tuple[np.ndarray, np.ndarray]:
    """``reference`` of ``batch(h, w, n)``, computed once and shared: treat as read-only."""
    key = (h, w, n)
    if key not in _CACHE:
        out, ms = reference(oracle(target), batch(h, w, n))
        out.setflags(write=False)
        ms.setflags(write=False)
        _CACHE[key] = (out, ms)
    return _CACHE[key]


def lab_hist(imgs: np.ndarray) -> np.ndarray:
    """``[n, 3, 256]`` counts of the 8-bit Lab bytes (what tia_lab_hist_u8 accumulates)."""
    lab = cvref.rgb2lab_u8(imgs).reshape(len(imgs), -1, 3)
    return np.stack([[np.bincount(im[:, c], minlength=256) for c in range(3)] for im in lab]).astype(np.int64)

"""Every route of the ResNet stem kernels (``csrc/stem_mfma.hip``) against a float64 reference on the operands they multiply.

Host tests (no marker): the reference's hand-worked answers, the launch geometry restated in ``_stem_ref`` and the proof that the case
lists reach every route of it, the bound helpers, and the sensitivity of each comparison to a deliberately wrong reference.

Device tests (``gpu``), all variants (float32 / fp16 / bf16 / split arithmetic, uint8 / float32 input, float32 / half pooled output, with
and without the pre-pool output) at every case:
  1. float64 tier: ``|got - ref| <= gamma(K + 1) (conv64(|x|, |w|) + |bias|)`` (+ half an ulp of a half output); ``max(err / bound)``
     is printed per case.  Largest ratios measured on an MI355X: DESIGN 4.7.
  2. consistency, bit for bit: fast against slow V-tile path, the two outputs, half outputs = float32 outputs rounded once, uint8 =
     float32 input.
  3. exact tier on integer data, 4. exact tier on one-hot taps through the uint8 staging at every dword alignment, 5. every window
     position reaches the pooled output, 6. batches beyond 2 GiB (the group split), 7. the refusals of ``stem_impl``.
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F  # noqa: N812

import _stem_ref as sr
from _conv_ref import HALF_EPS

GRID = sr.variant_grid()


def _fmt(case) -> str:
    return "x".join(str(v) for v in case)


# ====================================================================================================================================
# host: the reference
# ====================================================================================================================================
def _conv_by_hand(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """relu(conv 7x7 / 2 / 3 + bias) of ONE NHWC image by the definition, in Python floats (float64)."""
    h, w, _ = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.zeros((64, ho, wo), dtype=torch.float64)
    taps = [(o, c, ky, kx, float(weight[o, c, ky, kx])) for o, c, ky, kx in torch.nonzero(weight).tolist()]
    for cy in range(ho):
        for cx in range(wo):
            acc = [0.0] * 64
            for o, c, ky, kx, wv in taps:
                iy, ix = 2 * cy - 3 + ky, 2 * cx - 3 + kx
                if 0 <= iy < h and 0 <= ix < w:
                    acc[o] += float(x[iy, ix, c]) * wv
            for o in range(64):
                out[o, cy, cx] = max(acc[o] + float(bias[o]), 0.0)
    return out


def _pool_by_hand(conv: torch.Tensor) -> torch.Tensor:
    _, ho, wo = conv.shape
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    out = torch.zeros((conv.shape[0], hp, wp), dtype=torch.float64)
    for p in range(hp):
        for q in range(wp):
            rows = [r for r in (2 * p - 1, 2 * p, 2 * p + 1) if 0 <= r < ho]
            cols = [c for c in (2 * q - 1, 2 * q, 2 * q + 1) if 0 <= c < wo]
            out[:, p, q] = torch.stack([conv[:, r, c] for r in rows for c in cols]).amax(0)
    return out


def test_reference_one_hot_tap_on_a_9x9_image():
    """One active channel, one tap (output 5 reads channel 1 at ky = 2, kx = 4 with weight 2): conv[5, cy, cx] = 2 x[2 cy - 1, 2 cx + 1]."""
    x = torch.zeros((1, 9, 9, 3))
    x[0, :, :, 1] = torch.arange(81.0).view(9, 9) + 1
    x[0, :, :, 2] = 1000.0  # not read by any tap
    weight = torch.zeros((64, 3, 7, 7))
    weight[5, 1, 2, 4] = 2.0
    bias = torch.zeros(64)
    bias[5], bias[6] = -7.0, 0.25
    conv64, pooled64 = sr.stem_ref64(x, weight, bias, "f32")
    assert conv64.shape == (1, 64, 5, 5) and pooled64.shape == (1, 64, 3, 3)
    want = torch.zeros((5, 5), dtype=torch.float64)
    for cy in range(5):
        for cx in range(5):
            iy, ix = 2 * cy - 1, 2 * cx + 1
            v = 2.0 * (9 * iy + ix + 1) if 0 <= iy < 9 and ix < 9 else 0.0  # noqa: PLR2004
            want[cy, cx] = max(v - 7.0, 0.0)
    assert torch.equal(conv64[0, 5], want)
    assert float(want[1, 0]) == 2.0 * (9 + 1 + 1) - 7.0 and float(want[0, 0]) == 0.0 and float(want[4, 4]) == 0.0  # column 9 is off the image
    assert torch.equal(conv64[0, 6], torch.full((5, 5), 0.25, dtype=torch.float64))
    assert float(conv64[0, :5].abs().max()) == 0.0
    assert torch.equal(pooled64[0], _pool_by_hand(conv64[0]))
    assert float(pooled64[0, 5, 2, 1]) == float(want[4, 3])  # the largest of rows 3 .. 4 (5 is off the map), columns 1 .. 3
    assert torch.equal(conv64[0], _conv_by_hand(x[0], weight, bias))


def test_reference_1x1_image_and_operand_rounding():
    """A 1x1 image sees the centre taps only; each variant's operands are the values its kernel multiplies."""
    x, weight, bias = sr.make_data(1, 1, 1, seed=5)
    for arith in sr.ARITHMETICS:
        conv64, pooled64 = sr.stem_ref64(x, weight, bias, arith)
        assert conv64.shape == pooled64.shape == (1, 64, 1, 1)
        if arith == "split":
            lin = (x[0, 0, 0].double() * weight[:, :, 3, 3].double()).sum(1) / 255.0
        elif arith == "f32":
            lin = (x[0, 0, 0].float().div(255).double() * weight[:, :, 3, 3].double()).sum(1)
        else:
            dt = getattr(torch, arith)
            lin = (x[0, 0, 0].float().div(255).to(dt).double() * weight[:, :, 3, 3].to(dt).double()).sum(1)
        want = torch.relu(lin + bias.double())
        assert float((conv64.view(-1) - want).abs().max()) <= 1e-15 and torch.equal(pooled64, conv64)  # noqa: PLR2004
    # float32 input is taken as it is
    xf = x.float().div(255)
    assert torch.equal(sr.stem_ref64(xf, weight, bias, "f32")[0], sr.stem_ref64(x, weight, bias, "f32")[0])
    assert not torch.equal(sr.stem_ref64(x.float(), weight, bias, "f32")[0], sr.stem_ref64(x, weight, bias, "f32")[0])


@pytest.mark.parametrize("shape", [(9, 9), (5, 18), (13, 3)])
def test_reference_pooled_value_where_the_conv_map_is_odd(shape):
    """``wo`` (and ``ho``) odd: the last pooled pixel's window is cut by the map's edge.  By the definition on a random image."""
    h, w = shape
    x, weight, bias = sr.make_data(1, h, w, seed=h + w)
    weight = weight * (torch.rand(weight.shape, generator=torch.Generator().manual_seed(1)) < 0.04)  # noqa: PLR2004  (a few taps: by hand in Python)
    conv64, pooled64 = sr.stem_ref64(x, weight, bias, "f32")
    geom = sr.stem_geometry(1, h, w)
    assert conv64.shape == (1, 64, geom.ho, geom.wo) and pooled64.shape == (1, 64, geom.hp, geom.wp)
    by_hand = _conv_by_hand(x[0].float().div(255), weight, bias)
    assert float((conv64[0] - by_hand).abs().max()) <= 1e-14  # noqa: PLR2004
    assert torch.equal(pooled64[0], _pool_by_hand(conv64[0]))
    if geom.wo % 2:
        assert torch.equal(pooled64[0, :, 0, -1], conv64[0, :, :2, -2:].amax((1, 2)))


# ====================================================================================================================================
# host: geometry and route coverage
# ====================================================================================================================================
def test_restated_geometry_on_known_launches():
    g = sr.stem_geometry(1024, 256, 256)
    assert (g.ho, g.wo, g.hp, g.wp) == (128, 128, 64, 64) and g.strips == (sr.Strip(0, 64, 0, 128),)
    assert g.group >= 1024 and g.launches == (sr.Launch(0, 1024, 1, 64, 0),)
    g = sr.stem_geometry(1, 70, 600)
    assert (g.wo, g.wp) == (300, 150) and g.strips == (sr.Strip(0, 64, 0, 128), sr.Strip(64, 127, 127, 127), sr.Strip(127, 150, 253, 47))
    assert g.launches[0].chunks == 2 and g.launches[0].rows_per_chunk == 9 and g.hp == 18
    assert sr.even_group(11009, 11008) == 5505 and sr.even_group(7, 8) == 8 and sr.even_group(17, 8) == 6
    for n, h, w in sr.ALL_CASES:
        geom = sr.stem_geometry(n, h, w)
        # pooled columns are covered once, conv columns with the one-column overlap; no strip is wider than the 128-column tile
        assert [s.p0 for s in geom.strips[1:]] == [s.p1 for s in geom.strips[:-1]] and geom.strips[-1].p1 == geom.wp
        assert all(0 < s.ncols <= 128 and s.p1 - s.p0 <= 64 for s in geom.strips)
        assert geom.strips[-1].c_start + geom.strips[-1].ncols == geom.wo
        assert all(a.c_start + a.ncols - 1 in (b.c_start, b.c_start + 1) for a, b in zip(geom.strips, geom.strips[1:]))
        for launch in geom.launches:
            rows = sr.chunk_rows(geom, launch)
            assert rows[0][0] == 0 and rows[-1][1] == geom.hp and all(q0 < q1 for q0, q1 in rows)


def test_a_non_first_strip_never_has_128_columns():
    """A strip of 63 pooled columns needs conv columns ``2 p0 - 1 .. 2 p1 - 1``: 127.  Only the first strip (64 pooled columns from
    the map's edge) fills all 128 columns of the tile; the widest non-first strip is one column short, which is why its last wave
    is never on the fast V-tile path."""
    widest = 0
    for w in range(1, 1200):
        geom = sr.stem_geometry(1, 8, w)
        widest = max([widest] + [s.ncols for s in geom.strips[1:]])
    assert widest == 127  # noqa: PLR2004
    assert any(s.ncols == 127 for n, h, w in sr.ALL_CASES for s in sr.stem_geometry(n, h, w).strips[1:])  # noqa: PLR2004


def test_case_lists_reach_every_route():
    geoms = {case: sr.stem_geometry(*case) for case in sr.ALL_CASES}
    assert len(geoms) == len(sr.ALL_CASES)  # no case twice
    strips = {len(g.strips) for g in geoms.values()}
    assert {1, 2, 3, 4} <= strips
    last = {g.strips[-1].p1 - g.strips[-1].p0 for g in geoms.values() if len(g.strips) > 1}
    assert {1, 63} <= last
    assert any(s.ncols == 128 for g in geoms.values() for s in g.strips[:1])  # noqa: PLR2004  (non-first strips: 127 at the most, above)
    assert any(s.ncols == 127 for g in geoms.values() for s in g.strips[1:])  # noqa: PLR2004
    waves = {cols for g in geoms.values() for s in g.strips for cols in s.wave_columns()}
    assert 0 in waves and 32 in waves and any(0 < c < 32 for c in waves)  # noqa: PLR2004
    assert {1, 2, 31} <= waves  # a third strip of ONE column pair, and one column short of a whole wave
    chunks = {launch.chunks for g in geoms.values() for launch in g.launches}
    assert {1, 2} <= chunks and max(chunks) >= 4  # noqa: PLR2004
    assert any(launch.chunks > 1 and g.hp % launch.rows_per_chunk for g in geoms.values() for launch in g.launches)  # shorter last chunk
    assert any(launch.chunks == 1 and g.hp >= 16 for g in geoms.values() for launch in g.launches)  # noqa: PLR2004  (held to 1 by the batch)
    assert sr.stem_geometry(1100, 64, 8).launches[0].chunks == 1 and sr.stem_geometry(1, 64, 8).launches[0].chunks == 2  # noqa: PLR2004
    # chunk seams on an odd conv row count: the last pooled row of the map has one conv row, and a chunk's first row a carried row
    assert any(g.ho % 2 and launch.chunks > 1 for g in geoms.values() for launch in g.launches)
    assert {g.ho % 2 for g in geoms.values()} == {0, 1}
    for wp in (64, 65, 127, 128):
        assert {g.wo % 2 for g in geoms.values() if g.wp == wp} == {0, 1}, wp
    assert {(3 * w) % 4 for _, _, w in sr.WIDTH_CASES if w >= 253} == {0, 1, 2, 3}  # noqa: PLR2004
    for seam in (range(253, 263), range(505, 519), range(757, 763)):
        assert {(3 * w) % 4 for w in seam} == {0, 1, 2, 3}
    # fast and slow V-tile waves in the same launch; all slow once the pre-pool output is wanted
    mixed = [case for case, g in geoms.items() if sr.vtile_paths(g, conv_out=False) == {"fast", "slow"}]
    assert mixed and any(len(geoms[c].strips) > 1 for c in mixed) and any(geoms[c].ho % 2 for c in mixed)
    assert sr.vtile_paths(sr.stem_geometry(2, 256, 256), conv_out=False) == {"fast"}  # (the benchmark's shape: no slow wave at all)
    assert all(sr.vtile_paths(g, conv_out=True) == {"slow"} for g in geoms.values())
    assert any(sr.vtile_paths(g, conv_out=True, split=True) == {"fast", "slow"} for g in geoms.values())
    # images smaller than the 7x7 window, in both directions
    assert any(h < 7 and w < 7 for _, h, w in sr.ALL_CASES)  # noqa: PLR2004
    # the alignment cases: every offset at every residue of the row length, on two and three strips
    assert {off for *_, off in sr.ALIGN_CASES} == {0, 1, 2, 3}
    assert {len(sr.stem_geometry(n, h, w).strips) for n, h, w, _ in sr.ALIGN_CASES} == {2, 3}
    for n, h, w, off in sr.ALIGN_CASES:
        assert sr.stem_geometry(n, h, w, base=4096 + off).launches[0].x_shift == off
    for case in sr.WINDOW_CASES:
        g = sr.stem_geometry(*case)
        assert len(g.strips) >= 2 and g.launches[0].chunks >= 2  # noqa: PLR2004


def test_big_batches_split_into_groups_off_the_dword():
    n, h, w = sr.BIG_F32
    g = sr.stem_geometry(n, h, w, x_u8=False)
    assert n * h * w * 12 > 2 ** 31 and g.group == 86 and [(la.first, la.nb) for la in g.launches] == [(0, 86), (86, 85)]
    assert all(la.nb * h * w * 12 <= sr.INT_MAX for la in g.launches)
    n, h, w = sr.BIG_U8
    g = sr.stem_geometry(n, h, w, x_u8=True, base=0)
    assert (h * w * 3) % 2 == 1 and n * h * w * 3 > 2 ** 31
    assert g.group == 5505 and [(la.first, la.nb, la.x_shift) for la in g.launches] == [(0, 5505, 0), (5505, 5504, 3)]
    assert n * g.hp * g.wp * 64 * 2 > 5.7e9 and n * g.hp * g.wp * 64 * 4 > 11.5e9  # the outputs of the two variants


# ====================================================================================================================================
# host: bound helpers and sensitivity
# ====================================================================================================================================
def test_bound_helpers():
    assert sr.K_TERMS == {"f32": 148, "float16": 176, "bfloat16": 176, "split": 528}
    assert sr.gamma(149) == 149 * 2.0 ** -24 / (1 - 149 * 2.0 ** -24)
    ref = torch.tensor([1.0, 2.0 ** -15, 0.0, 3.0], dtype=torch.float64)
    b = torch.full((4,), 1e-6, dtype=torch.float64)
    assert torch.equal(sr.output_bound(b, ref, "float32"), b)
    assert torch.equal(sr.output_bound(b, ref, "bfloat16"), b + 2.0 ** -8 * ref)
    want = b + 2.0 ** -11 * ref + torch.tensor([0.0, 2.0 ** -25, 2.0 ** -25, 0.0], dtype=torch.float64)
    assert torch.equal(sr.output_bound(b, ref, "float16"), want)
    got = ref.clone().view(1, 1, 1, 4)
    got[..., 3] = float("nan")
    ratio, idx = sr.bound_ratio(got, ref.view(1, 1, 1, 4), b.view(1, 1, 1, 4))
    assert ratio == float("inf") and idx == (0, 0, 0, 3)
    # the bound on real data: pooled = window maximum, the split term, and the order of magnitude (K u sum |x w|)
    x, weight, bias = sr.make_data(2, 10, 257, seed=3)
    for arith in sr.ARITHMETICS:
        conv64, pooled64 = sr.stem_ref64(x, weight, bias, arith)
        bc, bp = sr.stem_bound(x, weight, bias, arith, conv64)
        assert bc.shape == conv64.shape and bp.shape == pooled64.shape and torch.equal(bp, F.max_pool2d(bc, 3, 2, 1))
        assert 1e-7 < float(bc.min()) and float(bc.max()) < (3e-4 if arith == "split" else 1e-4)  # noqa: PLR2004
    # a float32 evaluation in another order (the CPU's) lies inside it
    conv64, pooled64 = sr.stem_ref64(x, weight, bias, "f32")
    bc, bp = sr.stem_bound(x, weight, bias, "f32")
    c32 = F.relu(F.conv2d(x.float().div(255).permute(0, 3, 1, 2), weight, bias, 2, 3))
    assert sr.bound_ratio(c32, conv64, bc)[0] <= 1.0 and sr.bound_ratio(F.max_pool2d(c32, 3, 2, 1), pooled64, bp)[0] <= 1.0
    for out in ("float16", "bfloat16"):
        dt = getattr(torch, out)
        assert sr.bound_ratio(F.max_pool2d(c32, 3, 2, 1).to(dt), pooled64, sr.output_bound(bp, pooled64, out))[0] <= 1.0
        assert HALF_EPS[out] == torch.finfo(dt).eps


SENSITIVITY_CASES = [(2, 10, 257), (2, 10, 509), (2, 10, 761), (1, 131, 258), (3, 129, 66), (1, 70, 600), (2, 9, 13), (1, 8, 9)]


def test_sensitivity_cases_come_from_the_fixed_lists():
    assert set(SENSITIVITY_CASES) <= set(sr.ALL_CASES)


@pytest.mark.parametrize("case", SENSITIVITY_CASES, ids=_fmt)
def test_wrong_references_fail_the_comparison(case):
    """Each wrong reference, put in the kernel's place, must exceed the bound (or differ, in the exact tier) at every case it applies to."""
    n, h, w = case
    geom = sr.stem_geometry(n, h, w)
    x, weight, bias = sr.make_data(n, h, w, sr.case_seed(n, h, w))
    chunked = any(la.chunks > 1 for la in geom.launches)
    for arith in sr.ARITHMETICS:
        conv64, pooled64 = sr.stem_ref64(x, weight, bias, arith)
        bc, bp = sr.stem_bound(x, weight, bias, arith, conv64)
        assert sr.bound_ratio(pooled64, pooled64, bp)[0] == 0.0
        for name, (c_bad, p_bad) in (("tap dropped", sr.wrong_tap_dropped(x, weight, bias, arith)),
                                     ("taps transposed", sr.wrong_taps_transposed(x, weight, bias, arith))):
            assert sr.bound_ratio(c_bad, conv64, bc)[0] > 1.0, (name, arith)
            assert sr.bound_ratio(p_bad, pooled64, bp)[0] > 1.0, (name, arith)
        if chunked:
            assert sr.bound_ratio(sr.wrong_carried_row_missing(conv64, geom), pooled64, bp)[0] > 1.0, arith
        if len(geom.strips) > 1:
            for last in (False, True):
                assert sr.bound_ratio(sr.wrong_strip_column_zeroed(conv64, geom, last=last), pooled64, bp)[0] > 1.0, (arith, last)
        for out in ("float16", "bfloat16"):
            if arith in ("f32", out):
                bad = sr.wrong_bias_after_half_rounding(x, weight, bias, arith, out)
                assert sr.bound_ratio(bad, pooled64, sr.output_bound(bp, pooled64, out))[0] > 1.0, (arith, out)
                good = pooled64.float().to(getattr(torch, out))
                assert sr.bound_ratio(good, pooled64, sr.output_bound(bp, pooled64, out))[0] <= 1.0, (arith, out)


def test_reciprocal_instead_of_division_fails_the_one_hot_tier():
    """``x * fl(1 / 255)`` is inside any summation bound (one ulp of a term); the one-hot tier, a single exact product, sees it."""
    for n, h, w, _ in sr.ALIGN_CASES[::4]:
        x, weight, _ = sr.make_onehot_data(n, h, w, sr.case_seed(n, h, w))
        assert len(torch.unique(x)) == 256  # noqa: PLR2004  (every byte value)
        magnitudes = {float(v) for v in torch.unique(weight.abs())}
        assert magnitudes <= {0.0} | {2.0 ** k for k in range(-4, 4)} and len(magnitudes) >= 7  # noqa: PLR2004
        for v in (sr.Variant("f32", True, "float32", True), sr.Variant("f32", True, "bfloat16", True)):
            conv, pooled = sr.onehot_expected(x, weight, v)
            conv_bad, pooled_bad = sr.onehot_expected(x, weight, v, reciprocal=True)
            if v.out == "float32":
                assert not torch.equal(conv, conv_bad) and not torch.equal(pooled, pooled_bad)
            assert float(pooled.float().max()) > 0 and float((pooled == 0).float().mean()) > 0.2  # noqa: PLR2004  (negative taps: ReLU)


@pytest.mark.parametrize("case", sr.WINDOW_CASES, ids=_fmt)
def test_window_codes_single_out_the_own_pixel(case):
    """The pooled map of the coded conv map is the code of the window's own pixel wherever that pixel is on the map: an
    implementation that loses one of the nine window positions, at any strip or chunk seam, returns another number there."""
    n, h, w = case
    geom = sr.stem_geometry(n, h, w)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for axis in (0, 1):
                conv, pooled, own = sr.window_code_map(n, h, w, (a, b), axis)
                idx = torch.arange(geom.hp).view(-1, 1) if axis == 0 else torch.arange(geom.wp).view(1, -1)
                ph = a if axis == 0 else b
                code = (250 - idx if ph < 0 else 1 + idx).float().expand(geom.hp, geom.wp)
                assert torch.equal(pooled[0][own], code[own]) and int(own.sum()) >= (geom.hp - 1) * (geom.wp - 1)
                x = sr.window_input(conv, h, w, as_bytes=True)
                assert x.shape == (n, h, w, 3) and int((x != 0).sum()) == n * int(own.sum())
                if (a, b, axis) == (1, -1, 1):  # the reference agrees that the input produces this conv map (both forms)
                    c64, p64 = sr.stem_ref64(x, sr.window_weight(255.0), torch.zeros(64), "split")
                    assert torch.equal(c64[:, 7], conv.double()) and torch.equal(p64[:, 63], pooled.double())
                    c64, _ = sr.stem_ref64(sr.window_input(conv, h, w, as_bytes=False), sr.window_weight(1.0), torch.zeros(64), "bfloat16")
                    assert torch.equal(c64[:, 0], conv.double())


# ====================================================================================================================================
# device
# ====================================================================================================================================
def _dt(name: str) -> torch.dtype:
    return getattr(torch, name)


def _pack(weight: torch.Tensor, ariths) -> dict:
    from tiatoolbox_amd.models.architecture import fused

    wd = weight.cuda()
    packs = {}
    for arith in ariths:
        if arith == "f32":
            packs[arith] = fused.pack_stem_weights(wd)
        elif arith == "split":
            packs[arith] = fused.pack_stem_weights_split(wd)
            assert packs[arith] is not None
        else:
            packs[arith] = fused.pack_stem_weights_h(wd, _dt(arith))
    return packs


def _run(v: sr.Variant, x: torch.Tensor, packs: dict, bias_d: torch.Tensor):
    """(pooled, pre-pool or None) of variant ``v`` on the device tensor ``x`` (uint8 or float32 NHWC, as ``v.x_u8`` says)."""
    from tiatoolbox_amd.models.architecture import fused

    assert (x.dtype == torch.uint8) == v.x_u8
    if v.arith == "f32":
        out = fused.hip_stem_conv_pool(x, packs["f32"], bias_d, out_dtype=_dt(v.out), return_conv=v.conv)
        return out if v.conv else (out, None)
    if v.arith == "split":
        return fused.hip_stem_conv_pool_split(x, packs["split"], bias_d), None
    return fused.hip_stem_conv_pool_h(x, packs[v.arith], bias_d, dtype=_dt(v.arith)), None


def _offset_view(x: torch.Tensor, off: int) -> torch.Tensor:
    """The uint8 batch on the device at a base address ``off`` bytes past a dword."""
    flat = torch.zeros(x.numel() + 8, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    view = flat[off:off + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 4 == off and view.is_contiguous()
    return view


def _check_bound(tag: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, worst: dict, key: str) -> None:
    ratio, idx = sr.bound_ratio(got.cpu(), ref, bound)
    worst[key] = max(worst.get(key, 0.0), ratio)
    assert ratio <= 1.0, (f"{tag}: error {ratio:.3g} x the bound at (image, channel, row, column) {idx}: got {float(got[idx])!r}, "
                          f"float64 reference {float(ref[idx])!r}, bound {float(bound[idx]):.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sr.ALL_CASES, ids=_fmt)
def test_stem_within_the_float64_bound_and_consistent(case):
    """Tiers 1 and 2 at one case: every variant within the derived bound of the float64 reference (two draws: the second with the bias
    shifted by -0.3, so that about half the windows pool to exactly 0), and the bit-for-bit relations between the variants."""
    n, h, w = case
    for draw, shift in enumerate((0.0, -0.3)):
        x, weight, bias = sr.make_data(n, h, w, sr.case_seed(n, h, w) + draw, shift)
        packs, bias_d = _pack(weight, sr.ARITHMETICS), bias.cuda()
        inputs = {True: x.cuda(), False: x.float().div(255).cuda()}
        refs, bounds, worst = {}, {}, {}
        for arith in sr.ARITHMETICS:
            refs[arith] = sr.stem_ref64(x, weight, bias, arith)
            bounds[arith] = sr.stem_bound(x, weight, bias, arith, refs[arith][0])
        if draw == 1:
            zeros = float((refs["f32"][1] == 0).double().mean())
            assert n * h * w < 64 or 0.3 < zeros < 0.98, zeros  # noqa: PLR2004
        res = {v: _run(v, inputs[v.x_u8], packs, bias_d) for v in GRID}
        torch.cuda.synchronize()
        for v, (pooled, conv) in res.items():
            (ref_c, ref_p), (b_c, b_p) = refs[v.arith], bounds[v.arith]
            assert pooled.dtype == _dt(v.out) and pooled.shape == ref_p.shape and pooled.is_contiguous(memory_format=torch.channels_last)
            tag, key = f"{_fmt(case)} draw {draw} {v.name}", f"{v.arith}->{v.out}"
            _check_bound(tag + " pooled", pooled, ref_p, sr.output_bound(b_p, ref_p, v.out), worst, key)
            if v.conv:
                assert conv.dtype == _dt(v.out) and conv.shape == ref_c.shape
                _check_bound(tag + " pre-pool", conv, ref_c, sr.output_bound(b_c, ref_c, v.out), worst, key + " pre-pool")
        print(f"stem err/bound {_fmt(case)} draw {draw}: " + "  ".join(f"{k} {r:.3f}" for k, r in sorted(worst.items())))
        # ---- consistency, bit for bit ----
        for u8 in (True, False):
            p32, c32 = res[sr.Variant("f32", u8, "float32", True)]
            assert torch.equal(F.max_pool2d(c32, 3, 2, 1), p32), (case, u8)
            for out in ("float32", "float16", "bfloat16"):
                p_fast, _ = res[sr.Variant("f32", u8, out, False)]
                p_slow, c_slow = res[sr.Variant("f32", u8, out, True)]
                assert torch.equal(p_fast, p_slow), (case, u8, out)  # fast against slow V-tile path
                assert torch.equal(p_slow, p32.to(_dt(out))) and torch.equal(c_slow, c32.to(_dt(out))), (case, u8, out)  # rounded once
        for v in GRID:
            if v.x_u8 and v.arith != "split":
                other = res[v._replace(x_u8=False)]
                assert torch.equal(res[v][0], other[0]), (case, v.name)
                assert not v.conv or torch.equal(res[v][1], other[1]), (case, v.name)


@pytest.mark.gpu
@pytest.mark.parametrize("width", sorted({w for _, _, w, _ in sr.ALIGN_CASES}))
def test_stem_unaligned_uint8_batches_equal_the_aligned_one(width):
    """Tiers 1 and 2 on the alignment list: random data at the seam widths with the batch 1, 2 and 3 bytes off a dword gives every
    uint8 variant's aligned result bit for bit, and that result lies within the float64 bound."""
    n, h, w = next(case[:3] for case in sr.ALIGN_CASES if case[2] == width)
    x, weight, bias = sr.make_data(n, h, w, sr.case_seed(n, h, w) + 2)
    packs, bias_d = _pack(weight, sr.ARITHMETICS), bias.cuda()
    variants = [v for v in GRID if v.x_u8]
    worst, aligned = {}, {}
    for off in sorted({off for *_, off in sr.ALIGN_CASES}):
        view = _offset_view(x.cuda(), off)
        for v in variants:
            pooled, conv = _run(v, view, packs, bias_d)
            if off == 0:
                aligned[v] = (pooled, conv)
                ref_c, ref_p = sr.stem_ref64(x, weight, bias, v.arith)
                b_c, b_p = sr.stem_bound(x, weight, bias, v.arith, ref_c)
                _check_bound(f"2x10x{w} {v.name} pooled", pooled, ref_p, sr.output_bound(b_p, ref_p, v.out), worst, f"{v.arith}->{v.out}")
                if v.conv:
                    _check_bound(f"2x10x{w} {v.name} pre-pool", conv, ref_c, sr.output_bound(b_c, ref_c, v.out), worst, f"{v.arith}->{v.out} pre-pool")
            else:
                assert torch.equal(pooled, aligned[v][0]), (w, off, v.name)
                assert not v.conv or torch.equal(conv, aligned[v][1]), (w, off, v.name)
    print(f"stem err/bound {n}x{h}x{w} alignments: " + "  ".join(f"{k} {r:.3f}" for k, r in sorted(worst.items())))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sr.ALL_CASES, ids=_fmt)
def test_stem_integer_data_bit_for_bit(case):
    """Tier 3: float32 inputs 0 .. 15, integer weights and bias: every partial sum is an integer below 2^24, exact in any order.  The
    float32 stem returns the integers, a half output (and the half stems, whose operands are representable) ONE rounding of them."""
    n, h, w = case
    x, weight, bias = sr.make_exact_data(n, h, w, sr.case_seed(n, h, w))
    assert 147 * float(x.max()) * float(weight.abs().max()) + float(bias.abs().max()) < 2 ** 24
    conv64, pooled64 = sr.stem_ref64(x, weight, bias, "f32")
    assert torch.equal(conv64, conv64.round())
    packs, bias_d, xd = _pack(weight, ("f32", "float16", "bfloat16")), bias.cuda(), x.cuda()
    for v in GRID:
        if v.x_u8:
            continue
        pooled, conv = _run(v, xd, packs, bias_d)
        want_p = pooled64.float().to(_dt(v.out))
        bad = int((pooled.cpu() != want_p).sum())
        assert bad == 0, f"{_fmt(case)} {v.name}: {bad} of {want_p.numel()} pooled values differ from the exact result"
        if v.conv:
            want_c = conv64.float().to(_dt(v.out))
            bad = int((conv.cpu() != want_c).sum())
            assert bad == 0, f"{_fmt(case)} {v.name}: {bad} of {want_c.numel()} pre-pool values differ from the exact result"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sr.ALIGN_CASES, ids=_fmt)
def test_stem_one_hot_taps_through_the_uint8_staging(case):
    """Tier 4: one tap of weight +-2^k per output channel, random bytes, the batch 0 .. 3 bytes off a dword at the seam widths: every
    output is one exact product of ``fl(b / 255)`` -- the funnel shift, the byte masks and the strip overlap with no tolerance."""
    n, h, w, off = case
    x, weight, bias = sr.make_onehot_data(n, h, w, sr.case_seed(n, h, w))
    packs, bias_d = _pack(weight, ("f32", "float16", "bfloat16")), bias.cuda()
    view = _offset_view(x.cuda(), off)
    assert sr.stem_geometry(n, h, w, base=view.data_ptr()).launches[0].x_shift == off
    for v in GRID:
        if not v.x_u8 or v.arith == "split":
            continue
        pooled, conv = _run(v, view, packs, bias_d)
        want_c, want_p = sr.onehot_expected(x, weight, v)
        bad = int((pooled.cpu() != want_p).sum())
        assert bad == 0, f"{_fmt(case)} {v.name}: {bad} of {want_p.numel()} pooled values differ"
        if v.conv:
            bad = int((conv.cpu() != want_c).sum())
            assert bad == 0, f"{_fmt(case)} {v.name}: {bad} of {want_c.numel()} pre-pool values differ"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sr.WINDOW_CASES, ids=_fmt)
def test_every_window_position_reaches_the_pooled_output(case):
    """Tier 5, for the variants whose convolution is only seen through the maximum (half MFMA, split; the float32 stem is the
    control): per phase of the 3x3 window only one conv pixel per pooled pixel is non-zero and carries a code of its pooled row
    (or column); the pooled map must be the code map exactly."""
    n, h, w = case
    zero_bias = torch.zeros(64, device="cuda")
    packs = _pack(sr.window_weight(1.0), ("f32", "float16", "bfloat16"))
    packs["split"] = _pack(sr.window_weight(255.0), ("split",))["split"]
    variants = [sr.Variant("f32", False, "float32", False), sr.Variant("float16", False, "float16", False),
                sr.Variant("bfloat16", False, "bfloat16", False), sr.Variant("split", True, "float32", False)]
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for axis in (0, 1):
                conv_map, pooled_map, _ = sr.window_code_map(n, h, w, (a, b), axis)
                xf = sr.window_input(conv_map, h, w, as_bytes=False).cuda()
                xb = sr.window_input(conv_map, h, w, as_bytes=True).cuda()
                want = pooled_map[:, None].expand(n, 64, -1, -1)
                for v in variants:
                    pooled, _ = _run(v, xb if v.x_u8 else xf, packs, zero_bias)
                    got = pooled.float().cpu()
                    if not torch.equal(got, want):
                        wrong = torch.nonzero(got != want)
                        raise AssertionError(f"{_fmt(case)} {v.name} phase ({a}, {b}) coding {'rows' if axis == 0 else 'columns'}: "
                                             f"{len(wrong)} pooled values are not the code; first at (image, channel, row, column) "
                                             f"{tuple(wrong[0].tolist())}: got {float(got[tuple(wrong[0])])}, code {float(want[tuple(wrong[0])])}")


def _need_memory(gib: float) -> None:
    free, _ = torch.cuda.mem_get_info()
    if free < gib * 2 ** 30:
        pytest.skip(f"the batch beyond 2 GiB needs about {gib:.0f} GiB of free device memory; {free / 2 ** 30:.1f} GiB are free")


def _big_batch_check(v: sr.Variant, x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, geom: sr.Geometry) -> None:
    """Tier 6: the whole batch (several groups inside ``stem_impl``) against the same images as three sub-batches cut elsewhere, bit
    for bit on the device, and the images around each group boundary and the last one against the float64 bound."""
    n = x.shape[0]
    packs, bias_d = _pack(weight, (v.arith,)), bias.cuda()
    full, _ = _run(v, x, packs, bias_d)
    cuts = [0, n // 3 + 1, 2 * n // 3 + 2, n]
    firsts = {la.first for la in geom.launches}
    assert len(geom.launches) >= 2 and not firsts & set(cuts[1:-1])  # noqa: PLR2004
    for lo, hi in zip(cuts, cuts[1:]):
        assert sr.stem_geometry(hi - lo, geom.h, geom.w, x_u8=v.x_u8).group >= hi - lo  # one group each
        part, _ = _run(v, x[lo:hi], packs, bias_d)
        assert torch.equal(part, full[lo:hi]), f"{v.name}: images {lo} .. {hi - 1} differ between the whole batch and the sub-batch"
        del part
    worst = 0.0
    for i in sorted({la.first - 1 for la in geom.launches[1:]} | firsts - {0} | {0, n - 1}):
        xi = x[i:i + 1].cpu()
        ref_c, ref_p = sr.stem_ref64(xi, weight, bias, v.arith)
        _, b_p = sr.stem_bound(xi, weight, bias, v.arith, ref_c)
        ratio, idx = sr.bound_ratio(full[i:i + 1].cpu(), ref_p, sr.output_bound(b_p, ref_p, v.out))
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{v.name}: image {i} of {n}: error {ratio:.3g} x the bound at {idx}"
    print(f"stem err/bound beyond 2 GiB {n}x{geom.h}x{geom.w} {v.name}: {worst:.3f}")


@pytest.mark.gpu
def test_float32_batch_beyond_2_gib_runs_in_groups():
    n, h, w = sr.BIG_F32
    geom = sr.stem_geometry(n, h, w, x_u8=False)
    assert n * h * w * 12 > 2 ** 31 and geom.group < n
    _need_memory(12)
    _, weight, bias = sr.make_data(1, 8, 8, seed=171)
    x = torch.rand((n, h, w, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(171))
    _big_batch_check(sr.Variant("f32", False, "float32", False), x, weight, bias, geom)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [sr.Variant("f32", True, "bfloat16", False), sr.Variant("split", True, "float32", False)],
                         ids=lambda v: v.name.replace("/", "-"))
def test_uint8_batch_beyond_2_gib_second_group_off_the_dword(variant):
    n, h, w = sr.BIG_U8
    _need_memory(24)
    _, weight, bias = sr.make_data(1, 8, 8, seed=11009)
    x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11009))
    geom = sr.stem_geometry(n, h, w, x_u8=True, base=x.data_ptr())
    assert n * h * w * 3 > 2 ** 31 and geom.group < n and len(geom.launches) == 2  # noqa: PLR2004
    assert geom.launches[0].x_shift == 0 and geom.launches[1].x_shift in (1, 2, 3)  # the second group starts off a dword
    _big_batch_check(variant, x, weight, bias, geom)


@pytest.mark.gpu
def test_stem_impl_refuses_and_goes_on_working():
    """Tier 7: each refusal of ``stem_impl`` by its code, followed by a valid call that returns what it returned before."""
    from tiatoolbox_amd import _lib

    lib, inval, esize = _lib.load(), _lib.TIA_EINVAL, _lib.TIA_ESIZE
    n, h, w = 2, 10, 13
    x, weight, bias = sr.make_data(n, h, w, seed=7)
    packs, bias_d = _pack(weight, ("f32", "float16", "split")), bias.cuda()
    xb, xf = x.cuda(), x.float().div(255).cuda()
    geom = sr.stem_geometry(n, h, w)
    y = torch.zeros(n * geom.hp * geom.wp * 64 + 16, dtype=torch.float32, device="cuda")
    c = torch.zeros(n * geom.ho * geom.wo * 64 + 16, dtype=torch.float32, device="cuda")
    wf, wh, ws, bp, st = packs["f32"].data_ptr(), packs["float16"].data_ptr(), packs["split"].data_ptr(), bias_d.data_ptr(), _lib.current_stream()
    f32, f16 = 0, 1
    valid = sr.Variant("f32", True, "float16", True)
    before = _run(valid, xb, packs, bias_d)

    def still_works():
        after = _run(valid, xb, packs, bias_d)
        torch.cuda.synchronize()
        assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
        assert float(y.abs().max()) == 0.0 and float(c.abs().max()) == 0.0  # no refused call wrote anything

    conv_nhwc, plain, half, split = (lib.tia_stem_conv7x7_pool_conv_nhwc, lib.tia_stem_conv7x7_pool_nhwc, lib.tia_stem_conv7x7_pool_nhwc_h,
                                     lib.tia_stem_conv7x7_pool_nhwc_u8x3)
    refusals = [
        ("d_y 4 bytes off", inval, lambda: plain(xb.data_ptr(), 1, wf, bp, y.data_ptr() + 4, f32, 0, n, h, w, st)),
        ("d_y 8 bytes off, half", inval, lambda: half(xb.data_ptr(), 1, wh, bp, y.data_ptr() + 8, f16, n, h, w, st)),
        ("d_y 4 bytes off, split", inval, lambda: split(xb.data_ptr(), ws, bp, y.data_ptr() + 4, n, h, w, st)),
        ("weights 4 bytes off", inval, lambda: plain(xb.data_ptr(), 1, wf + 4, bp, y.data_ptr(), f32, 0, n, h, w, st)),
        ("half weights 8 bytes off", inval, lambda: half(xb.data_ptr(), 1, wh + 8, bp, y.data_ptr(), f16, n, h, w, st)),
        ("float32 input 1 byte off", inval, lambda: plain(xf.data_ptr() + 1, 0, wf, bp, y.data_ptr(), f32, 0, n, h, w, st)),
        ("float32 input 2 bytes off", inval, lambda: half(xf.data_ptr() + 2, 0, wh, bp, y.data_ptr(), f16, n, h, w, st)),
        ("half pre-pool 8 bytes off", inval, lambda: conv_nhwc(xb.data_ptr(), 1, wf, bp, y.data_ptr(), f16, c.data_ptr() + 8, n, h, w, st)),
        ("half pre-pool 2 bytes off", inval, lambda: conv_nhwc(xb.data_ptr(), 1, wf, bp, y.data_ptr(), 2, c.data_ptr() + 2, n, h, w, st)),
        ("y_dtype 3", inval, lambda: plain(xb.data_ptr(), 1, wf, bp, y.data_ptr(), 3, 0, n, h, w, st)),
        ("y_dtype -1", inval, lambda: conv_nhwc(xb.data_ptr(), 1, wf, bp, y.data_ptr(), -1, c.data_ptr(), n, h, w, st)),
        ("half stem, float32 code", inval, lambda: half(xb.data_ptr(), 1, wh, bp, y.data_ptr(), f32, n, h, w, st)),
        ("n = 0", inval, lambda: plain(xb.data_ptr(), 1, wf, bp, y.data_ptr(), f32, 0, 0, h, w, st)),
        ("h = 0", inval, lambda: plain(xb.data_ptr(), 1, wf, bp, y.data_ptr(), f32, 0, n, 0, w, st)),
        ("w = -1", inval, lambda: split(xb.data_ptr(), ws, bp, y.data_ptr(), n, h, -1, st)),
        ("n = -5, half", inval, lambda: half(xb.data_ptr(), 1, wh, bp, y.data_ptr(), f16, -5, h, w, st)),
        # one image beyond 2^31 - 1 bytes: the dimensions alone are refused, before any launch
        ("uint8 image of 26755^2", esize, lambda: plain(xb.data_ptr(), 1, wf, bp, y.data_ptr(), f32, 0, 1, 26755, 26755, st)),
        ("float32 image of 13378^2", esize, lambda: plain(xf.data_ptr(), 0, wf, bp, y.data_ptr(), f32, 0, 1, 13378, 13378, st)),
        ("split, image of 1 x 2^30", esize, lambda: split(xb.data_ptr(), ws, bp, y.data_ptr(), 1, 1, 1 << 30, st)),
    ]
    assert 26755 * 26755 * 3 > sr.INT_MAX >= 26754 * 26754 * 3 and 13378 * 13378 * 12 > sr.INT_MAX
    for name, code, call in refusals:
        rc = call()
        assert rc == code, (name, rc, code)
        still_works()

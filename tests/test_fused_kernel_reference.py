"""The kernels ``FusedHoVerNet`` and ``FusedUNet`` launch between their plain convolutions, each against a plain reference on the CPU
computed from exactly the values the kernel is given, never by another kernel of this library:

* ``tia_conv2d_post_nhwc_f32`` (both tile widths of ``conv_mfma_f32_kernel<BN, POST>``), ``tia_conv1x1_pre_nhwc_f32`` (``<BN, false,
  PRE>``), ``tia_conv2d_thin_nhwc_f32``, ``tia_conv1x1_head_nhwc_f32`` and ``tia_grouped_conv_valid_nhwc_f32`` against float64;
* ``tia_scale_shift_act(_view)_nhwc_f32``, ``tia_upsample2x_add(_act)_nhwc_f32``, ``tia_bias_act_nhwc`` and
  ``tia_bias_relu_maxpool_nhwc`` against the specified sequence of float32 operations, by equality.

Four tiers, as in ``tests/test_conv_reference_sweep.py``: (1) fixed edge cases with every argument combination, including one case
per grid-stride kernel of more than twice its grid cap; (2) a seeded random sweep; (3) integer data bit for bit; (4) the > 2 GiB
batch split of ``conv2d_impl`` for POST and PRE.  Helpers, case lists and bounds are in ``tests/_fused_ref.py``; the tests without the
``gpu`` mark check them on the host, including that every comparison rejects a reference that is wrong in a way a kernel can be."""

from __future__ import annotations

import gc
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _conv_ref as R  # noqa: E402, N812
import _fused_ref as X  # noqa: E402, N812

QUARTER, HALF = 0.25, 0.5


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
def test_references_match_hand_computed_examples():
    """One written-out example per reference: a post value, a pre value, a head pixel, a 1 x 2 upsample-add, a 3 x 3 pool with cut
    windows, bias_act with one rounding."""
    # post: 32 channels of which two are non-zero, 1x1: lin = 2 * 3 + (-1) * 4 = 2; v = 2 + 0.5 (bias) - 4 (residual) = -1.5;
    # y2 = relu(-1.5 * -2 + 0.25) = 3.25; with the ReLU in the epilogue v = 0 and y2 = relu(0.25) = 0.25
    case = X._post(1, 32, 64, 1, 1)  # noqa: SLF001
    x = torch.zeros((1, 32, 1, 1))
    x[0, 0], x[0, 5] = 2.0, -1.0
    w = torch.zeros((64, 32, 1, 1))
    w[7, 0], w[7, 5] = 3.0, 4.0
    bias, res, ps, pt = torch.full((64,), 0.5), torch.full((1, 64, 1, 1), -4.0), torch.full((64,), -2.0), torch.full((64,), 0.25)
    v, y2 = X.post_ref64(case, x, w, bias, res, False, ps, pt)
    assert (float(v[0, 7, 0, 0]), float(y2[0, 7, 0, 0])) == (-1.5, 3.25)
    assert (float(v[0, 0, 0, 0]), float(y2[0, 0, 0, 0])) == (-3.5, 7.25)  # a channel without weights: bias + residual only
    v, y2 = X.post_ref64(case, x, w, bias, res, True, ps, pt)
    assert (float(v[0, 7, 0, 0]), float(y2[0, 7, 0, 0])) == (0.0, 0.25)
    # pre: operand relu(x * sc + sh) = relu(2 * 2 - 1) = 3 (channel 0), relu(-1 * 2 - 1) = 0 (channel 5), relu(-1) = 0 elsewhere
    sc, sh = torch.full((32,), 2.0), torch.full((32,), -1.0)
    got = X.pre_ref64(X._pre(1, 32, 64, 1, 1), x, sc, sh, w, bias, None, False)  # noqa: SLF001
    assert float(got[0, 7, 0, 0]) == 3 * 3 + 0.5 and float(got[0, 1, 0, 0]) == 0.5  # noqa: PLR2004
    # stride 2 keeps pixels (0, 0) and (0, 2) of a 1 x 3 map
    x3 = torch.zeros((1, 32, 1, 3))
    x3[0, 0, 0] = torch.tensor([1.0, 5.0, 2.0])
    got = X.pre_ref64(X._pre(1, 32, 64, 1, 3, stride=2), x3, sc, sh, w, None, None, False)  # noqa: SLF001
    assert got[0, 7, 0].tolist() == [3.0 * 1, 3.0 * 3]
    # head: one pixel, channels 1 and 63: 0.5 * 4 + 2 * (-3) = -4, plus bias 1 = -3; with pre (sc 2, sh 1): relu(9) * 0.5 + relu(-5) * 2 = 4.5
    xh = torch.zeros((1, 64, 1, 1))
    xh[0, 1], xh[0, 63] = 4.0, -3.0
    wh = torch.zeros((2, 64))
    wh[1, 1], wh[1, 63] = 0.5, 2.0
    assert X.head_ref64(xh, wh, torch.tensor([0.0, 1.0])).flatten().tolist() == [0.0, -3.0]
    with_pre = X.head_ref64(xh, wh, None, torch.full((64,), 2.0), torch.cat([torch.zeros(1), torch.ones(63)]))
    assert with_pre.flatten().tolist() == [0.0, 4.5 + 0.0]
    # upsample-add: a 1 x 2 map becomes 2 x 4; out[Y][X] = x[Y / 2][X / 2] + y[Y][X]
    xu = torch.tensor([[[[10.0, 20.0]]]])
    yu = torch.arange(8.0).view(1, 1, 2, 4)
    assert X.upsample_add_ref(xu, yu).tolist() == [[[[10.0, 11.0, 22.0, 23.0], [14.0, 15.0, 26.0, 27.0]]]]
    act = X.upsample_add_ref(xu, yu, torch.tensor([-1.0]), torch.tensor([12.0]))  # relu(12 - .)
    assert act.tolist() == [[[[2.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]]]
    assert X.upsample_add_ref(xu, yu, source_offset=1).tolist() == [[[[10.0, 21.0, 22.0, 23.0], [14.0, 25.0, 26.0, 27.0]]]]
    # pool: 3 x 3 map, bias 1: out (0, 0) sees rows 0..1 x columns 0..1, (0, 1) columns 1..2, (1, 0) rows 1..2, (1, 1) rows 1..2 x columns 1..2
    xp = torch.tensor([[[[-9.0, 2.0, -5.0], [1.0, -3.0, -7.0], [-8.0, -6.0, -4.0]]]])
    assert X.pool_ref(xp, torch.tensor([1.0])).tolist() == [[[[3.0, 3.0], [2.0, 0.0]]]]
    assert X.pool_ref(xp, torch.tensor([1.0]), first_row=0).tolist() == [[[[3.0, 3.0], [0.0, 0.0]]]]  # rows 0..2, then row 2 only
    assert X.pool_ref(-xp.abs(), torch.tensor([0.5])).abs().max() == 0  # all-negative input: every pooled value is 0
    # bias_act in bf16 (8 significant bits: even integers only from 256 on): 256 + 1 + 2 = 259 is a tie between 258 and 260 and goes
    # to even, 260; rounding 257 first gives 256 (a tie again) and then 258, which is representable: the wrong form differs
    xb = torch.tensor([[[[256.0]]]], dtype=torch.bfloat16)
    one, two = torch.tensor([1.0], dtype=torch.bfloat16), torch.tensor([[[[2.0]]]], dtype=torch.bfloat16)
    assert float(X.bias_act_ref(xb, one, two, relu=True)) == 260.0  # noqa: PLR2004
    assert float(X.bias_act_ref(xb, one, two, relu=True, round_before_residual=True)) == 258.0  # noqa: PLR2004
    assert float(X.bias_act_ref(-xb, one, None, relu=True)) == 0.0 and float(X.bias_act_ref(-xb, one, None, relu=False)) == -255.0  # noqa: PLR2004
    # the operand / post arithmetic rounds the product and the sum separately: 3 * (1 + 2^-23) = 3 + 1.5 * 2^-22 is a tie and rounds
    # to 3 + 2^-21; - 2^-23 is a tie again and stays there.  A fused multiply-add gives 3 + 1.5 * 2^-22 - 0.5 * 2^-22 = 3 + 2^-22.
    a = torch.tensor([1.0 + 2.0 ** -23]).view(1, 1, 1, 1)
    got = X.scale_shift_ref(a, torch.tensor([3.0]), torch.tensor([-(2.0 ** -23)]))
    fused = float(torch.tensor(3.0 * (1.0 + 2.0 ** -23) - 2.0 ** -23, dtype=torch.float64).float())
    assert float(got) == 3.0 + 2.0 ** -21 and fused == 3.0 + 2.0 ** -22  # noqa: PLR2004


@pytest.mark.parametrize("kernel", X.CONV_KERNELS)
def test_cases_are_what_the_entry_points_serve(kernel):
    """Fixed, random and exact cases are inside what each entry point documents; the fixed lists hold the edges tier 1 is about; the
    random draw is reproducible."""
    fixed, rand = X.fixed_cases(kernel), X.random_cases(kernel)
    assert rand == X.random_cases(kernel) and len(rand) >= 24  # noqa: PLR2004
    for c in fixed + rand + X.exact_cases(kernel):
        assert c.kernel == kernel and X.served(c), c
    pixels = {c.n * c.ho * c.wo for c in fixed}
    if kernel in ("post", "pre"):
        for width in (64, 128):
            mine = [c for c in fixed if X.tile_width(c) == width]
            assert {1, 127, 128, 129} <= {c.n * c.ho * c.wo for c in mine}, width
            assert any(c.n * c.ho * c.wo % 128 == 0 and c.n * c.ho * c.wo > 128 for c in mine), width  # noqa: PLR2004
            assert any(c.h != c.w and c.stride == 2 for c in mine) and any(c.n > 1 for c in mine), width  # noqa: PLR2004
        assert sum(c.h != c.w for c in fixed) >= len(fixed) // 2
    if kernel == "post":
        w64 = {(c.cout, c.k) for c in fixed if X.tile_width(c) == 64}  # noqa: PLR2004
        assert {(64, 1), (192, 1), (128, 1), (64, 3), (192, 3)} <= w64
        assert all(c.cin <= 256 for c in fixed if c.cout % 128 == 0 and X.tile_width(c) == 64)  # noqa: PLR2004
        w128 = {(c.cout, c.k, c.cin) for c in fixed if X.tile_width(c) == 128}  # noqa: PLR2004
        assert {(128, 1, 288), (256, 1, 288), (128, 1, 512), (256, 1, 512)} <= w128 and any(k == 3 and co == 128 for co, k, _ in w128)  # noqa: PLR2004
        assert {c.k for c in fixed} == {1, 3} and {c.stride for c in fixed} == {1, 2}
        assert {(c.pad_lo, c.pad_hi) for c in fixed if c.k == 3} == {(0, 0), (1, 1), (0, 1)}  # noqa: PLR2004
        assert len(X.epilogues(fixed[0])) == 8  # noqa: PLR2004
    if kernel == "pre":
        assert {c.cin for c in fixed if X.tile_width(c) == 128} >= {288, 512, 1024}  # noqa: PLR2004
        assert {c.cout for c in fixed if c.cin > 256 and X.tile_width(c) == 64} >= {64, 192}  # noqa: PLR2004
        assert all(c.cin <= 256 or c.cout % 128 for c in fixed if X.tile_width(c) == 64)  # noqa: PLR2004
        assert {c.stride for c in fixed} == {1, 2, 3}
        assert sum(c.stride > 1 and c.h % c.stride != c.w % c.stride for c in fixed) >= 5  # noqa: PLR2004
    if kernel == "thin":
        assert {(c.cin, c.k) for c in fixed} == set(X.THIN_CK) and {c.n for c in fixed} == {1, 3} and {c.cout for c in fixed} == {64, 128, 192}
        for c_, k in X.THIN_CK:
            mine = [c for c in fixed if (c.cin, c.k) == (c_, k)]
            borders = {(k // 2, k // 2), (0, 0), (0, 1)} | ({(2, 3)} if k >= 5 else set())  # noqa: PLR2004
            assert {(c.stride, c.pad_lo, c.pad_hi) for c in mine} == {(s, lo, hi) for s in (1, 2, 3) for lo, hi in borders}, (c_, k)
        assert sorted({c.cin * c.k for c in fixed}) == [3, 16, 20, 21, 30, 32] and max(c.k for c in fixed) == 16  # noqa: PLR2004
        extra = [X.thin_extra(c) for c in fixed]
        assert sum(e > 0 for e in extra) >= 10 and sum(e == 0 for e in extra) >= 10  # noqa: PLR2004  (both occur)
    if kernel == "head":
        assert {c.cout for c in fixed} == set(range(1, 9)) and {c.n * c.h * c.w for c in fixed} == set(X.HEAD_PIXELS)
        assert set(X.HEAD_PIXELS) == {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257}
        assert all(n * h * w == npix and (h != w or npix in (1, 4)) for npix, (n, h, w) in X.HEAD_PIXELS.items())  # noqa: PLR2004
        assert {c.cout for c in X.exact_cases(kernel)} == set(range(1, 9))
    if kernel == "gvalid":
        assert {(c.groups, c.k) for c in fixed} == {(g, k) for g in X.GVALID_GROUPS for k in X.GVALID_K}
        assert {1, 255, 256, 257} <= pixels
        assert any((c.ho, c.wo) == (1, 1) for c in fixed) and any(c.ho == 1 and c.wo > 1 for c in fixed)
        assert any(c.wo == 1 and c.ho > 1 for c in fixed) and any(c.n > 1 for c in fixed)
        for k in X.GVALID_K:
            assert {(c.ho == 1, c.wo == 1) for c in fixed if c.k == k} >= {(True, True), (False, False)}, k


def test_elementwise_case_lists_hold_the_edges():
    assert {s[1] for s in X.SCALE_SHIFT_SHAPES} == {4, 8, 96, 2048} and sum(s[0] * s[2] * s[3] == 1 for s in X.SCALE_SHIFT_SHAPES) == 4  # noqa: PLR2004
    for (n, cw, hh, ww), c, y0, x0, h, w in X.SCALE_SHIFT_VIEWS:
        assert c % 4 == 0 and cw % 4 == 0 and c <= cw and y0 + h <= hh and x0 + w <= ww and n >= 1
    views = X.SCALE_SHIFT_VIEWS
    assert any(c < cw and (y0 or x0) and n > 1 for (n, cw, _, _), c, y0, x0, _, _ in views)  # prefix, base offset, n > 1, stride > c
    assert any(c == cw and (y0 or x0) for (_, cw, _, _), c, y0, x0, _, _ in views)
    shapes = X.UPSAMPLE_SHAPES
    assert any(h == 1 and w > 1 for _, _, h, w in shapes) and any(w == 1 and h > 1 for _, _, h, w in shapes)
    assert any((h, w) == (1, 1) for _, _, h, w in shapes) and any(c == 4 for _, c, _, _ in shapes) and any(n > 1 and h != w for n, _, h, w in shapes)  # noqa: PLR2004
    assert X.UPSAMPLE_CROP[0] != X.UPSAMPLE_CROP[1] and X.UPSAMPLE_CROP[2] - X.UPSAMPLE_CROP[0] != X.UPSAMPLE_CROP[3] - X.UPSAMPLE_CROP[1]
    assert {s[1] for s in X.BIAS_ACT_SHAPES} == {8, 24, 64} and any(s[0] > 1 for s in X.BIAS_ACT_SHAPES)
    assert len(X.POOL_HW) == 20 and set(X.POOL_CHANNELS) == {8, 24, 64}  # noqa: PLR2004


@pytest.mark.parametrize("kernel", sorted(X.BEYOND_CAP))
def test_beyond_cap_cases_exceed_twice_the_grid_cap(kernel):
    """Every thread of a capped grid runs its loop body more than once: the case has more than twice the cap's work items."""
    work, cap = X.work_items(kernel)
    assert work > 2 * cap, (kernel, work, cap)
    assert work < 3 * cap  # (no larger than the point needs)
    assert (X.CAP_BIAS_ACT, X.CAP_SCALE_SHIFT, X.CAP_HEAD) == (2097152, 4194304, 262144)
    if kernel == "head":  # the 262,144 pixels of one pass: 256 * 16 workgroups x 4 waves x 4 groups x 4 pixels
        assert cap == 256 * 16 * 4 * 4 * 4


def test_random_sweep_reaches_both_tile_widths_and_every_head_width():
    for kernel in ("post", "pre"):
        cases = X.random_cases(kernel)
        for width in (64, 128):
            assert sum(X.tile_width(c) == width and c.h != c.w for c in cases) >= X.TILE_FLOOR, (kernel, width)
    assert X.tile_width(X._post(1, 256, 128, 4, 4)) == 64 and X.tile_width(X._post(1, 288, 128, 4, 4)) == 128  # noqa: PLR2004, SLF001
    assert X.tile_width(X._post(1, 32, 128, 4, 4, k=3)) == 128 and X.tile_width(X._post(1, 512, 192, 4, 4, k=3)) == 64  # noqa: PLR2004, SLF001
    assert {c.cout for c in X.random_cases("head")} == set(range(1, 9))
    assert {c.stride for c in X.random_cases("pre")} == {1, 2, 3} and {c.k for c in X.random_cases("post")} == {1, 3}


@pytest.mark.parametrize("kernel", X.CONV_KERNELS)
def test_exact_tier_stays_below_2_to_24(kernel):
    """``fused_exact_bound`` from the value ranges; the data really lies inside them; at least half of the reference is non-zero."""
    for c in X.exact_cases(kernel) + [X.SPLIT_CASES.get(kernel, X.exact_cases(kernel)[0])]:
        assert X.fused_exact_bound(c) < 2 ** 24, (c, X.fused_exact_bound(c))
    case = X.exact_cases(kernel)[-1]
    d = X.make_exact_data(case, 11)
    assert float(d["x"].abs().max()) <= X.X_MAX and float(d["w"].abs().max()) <= X.W_MAX and float(d["bias"].abs().max()) <= X.B_MAX
    assert float(d["res"].abs().max()) <= X.R_MAX and 1 <= float(d["ps"].min()) and float(d["ps"].max()) <= X.PS_MAX
    assert float(d["pt"].abs().max()) <= X.PT_MAX and float(d["sc"].abs().max()) <= X.SC_MAX and float(d["sh"].abs().max()) <= X.SH_MAX
    ref = X.evaluate(case, d, X.epilogues(case)[-1])
    for r in ref if isinstance(ref, tuple) else (ref,):
        assert torch.equal(r, r.round()) and float(r.abs().max()) <= X.fused_exact_bound(case)
    assert X.fused_exact_bound(X._post(1, 512, 128, 8, 8, k=3)) == (9 * 512 * 2 + 64 + 64) * 3 + 8  # noqa: SLF001
    assert X.fused_exact_bound(X._pre(1, 1024, 128, 8, 8)) == 1024 * (2 * 3 + 4) + 128  # noqa: SLF001


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_half_integer_data_lies_where_a_second_rounding_shows(dtype):
    """fp16 / bf16 ``bias_act`` and ``bias_relu_maxpool`` on integer data: at least a quarter of the expected results are not
    representable before the one rounding, and a reference that rounds ``x + b`` to half before adding the residual differs from
    the right one in at least 5 % of the elements and is rejected."""
    dt = getattr(torch, dtype)
    for shape in X.BIAS_ACT_SHAPES:
        if shape[0] * shape[2] * shape[3] < 20:  # noqa: PLR2004  (shares of a handful of elements say nothing)
            continue
        x, bias, res = X.make_half_integer_data(shape, dtype, 21)
        exact = x.double() + bias.double().view(1, -1, 1, 1) + res.double()
        assert float((exact.float().to(dt).double() != exact).double().mean()) >= QUARTER, (dtype, shape)
        assert float(exact.abs().max()) < 65504 / 2  # noqa: PLR2004
        good = X.bias_act_ref(x, bias, res, relu=False)
        assert torch.equal(good, R.to_half_once(exact, dt))
        twice = X.bias_act_ref(x, bias, res, relu=False, round_before_residual=True)
        assert float((twice != good).double().mean()) >= 0.05, (dtype, shape)  # noqa: PLR2004
        with pytest.raises(AssertionError, match="image, channel, row, column"):
            X.check_equal("rounded twice", twice, good)
        pooled_exact = X.pool_ref(x.double(), bias.double())
        assert float((pooled_exact.float().to(dt).double() != pooled_exact).double().mean()) >= QUARTER, (dtype, shape)


def _rounded(ref64: torch.Tensor) -> torch.Tensor:
    return ref64.float()


@pytest.mark.parametrize("kernel", X.CONV_KERNELS)
def test_comparisons_fail_for_a_subtly_wrong_reference(kernel):
    """Without a kernel: the right float64 result rounded to float32 passes tier 1 and tier 3; what a kernel with each of the named
    faults would compute is rejected by both, with a message naming an element."""
    case = {"post": X._post(2, 96, 128, 9, 6, k=3, pad=(1, 1)), "pre": X._pre(2, 96, 128, 13, 20, stride=2),  # noqa: SLF001
            "thin": R.Case("thin", 2, 3, 64, 12, 17, k=7, stride=2, pad_lo=3, pad_hi=3),
            "head": R.Case("head", 1, 64, 5, 7, 9, k=1, pad_lo=0, pad_hi=0),
            "gvalid": R.Case("gvalid", 2, 96, 24, 9, 12, k=3, pad_lo=0, pad_hi=0, groups=3)}[kernel]
    assert X.served(case)
    for make, exact in ((X.make_data, False), (X.make_exact_data, True)):
        d = make(case, 5)
        wrong = {}
        if kernel == "pre":
            swapped = dict(d, sc=torch.cat([d["sc"][4:8], d["sc"][:4], d["sc"][8:]]), sh=torch.cat([d["sh"][4:8], d["sh"][:4], d["sh"][8:]]))
            wrong = {"operand without its ReLU": lambda e, d=d: R.epilogue64(
                         R.conv_ref64(case, X.scale_shift_ref(d["x"], d["sc"], d["sh"], relu=False), d["w"]),
                         d["bias"] if e[0] else None, d["res"] if e[1] else None, e[2]),
                     "scale / shift of two channel quads swapped": lambda e, s=swapped: X.evaluate(case, s, e)}
        elif kernel == "thin":
            shifted = dict(d, x=torch.nn.functional.pad(d["x"], (1, 0))[..., :-1])
            last = d["w"].clone()
            last[..., -1] = 0
            wrong = {"taps shifted by one column": lambda e, s=shifted: X.evaluate(case, s, e),
                     "last tap column zeroed": lambda e, s=dict(d, w=last): X.evaluate(case, s, e)}
        elif kernel == "head":
            dropped = d["w"].clone()
            dropped[:, 4:8] = 0
            wrong = {"one channel quad dropped": lambda e, s=dict(d, w=dropped): X.evaluate(case, s, e),
                     "outputs o and o + 1 swapped": lambda e: X.evaluate(case, d, e)[:, [0, 2, 1, 3, 4]]}
        elif kernel == "gvalid":
            w = d["w"]
            wrong = {"weights of two groups swapped": lambda e, s=dict(d, w=torch.cat([w[8:16], w[:8], w[16:]])): X.evaluate(case, s, e)}
        for epilogue in X.epilogues(case):
            ref = X.evaluate(case, d, epilogue)
            label = f"{case} {epilogue}"
            if kernel == "post":
                v, y2 = ref
                use_bias, use_res, relu = epilogue
                ps, pt = d["ps"].double().view(1, -1, 1, 1), d["pt"].double().view(1, -1, 1, 1)
                v_nores = R.epilogue64(R.conv_ref64(case, d["x"], d["w"]), d["bias"] if use_bias else None, None, relu)
                bad = {"ReLU before the scale and shift": torch.relu(v) * ps + pt, "shift dropped": torch.relu(v * ps)}
                if use_res:
                    bad["y2 from the sum without the residual"] = torch.relu(v_nores * ps + pt)
                checks = [(lambda g, r=v: X.check_exact(label, g, r)), (lambda g, r=y2: X.check_exact(label, g, r))] if exact else [
                    (lambda g, r=v: X.check_close(label, "post", g, r)), (lambda g, r=y2: X.check_close(label, "post", g, r, **X.y2_gate(d["ps"])))]
                checks[0](_rounded(v))
                checks[1](_rounded(y2))
                if exact:  # (in the tolerance tier the float32 sequence rounds differently from float64: the GPU test's check)
                    X.check_equal(label, X.scale_shift_ref(_rounded(v), d["ps"], d["pt"]), _rounded(y2))
                for name, y2_bad in bad.items():
                    with pytest.raises(AssertionError, match="image, channel, row, column"):
                        checks[1](_rounded(y2_bad))
                        pytest.fail(f"accepted '{name}' for {label}")
                continue
            check = (lambda g, r=ref: X.check_exact(label, g, r)) if exact else (lambda g, r=ref: X.check_close(label, kernel, g, r))
            check(_rounded(ref))
            for name, make_bad in wrong.items():
                with pytest.raises(AssertionError, match="image, channel, row, column"):
                    check(_rounded(make_bad(epilogue)))
                    pytest.fail(f"accepted '{name}' for {label}")


def test_elementwise_comparisons_fail_for_a_wrong_window_or_source_pixel():
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn((2, 8, 3, 5), generator=g), torch.randn((2, 8, 6, 10), generator=g)
    s, t = torch.randn(8, generator=g), torch.randn(8, generator=g)
    for args in ((), (s, t)):
        good = X.upsample_add_ref(x, y, *args)
        X.check_equal("upsample", good.clone(), good)
        with pytest.raises(AssertionError, match="image, channel, row, column"):
            X.check_equal("upsample from (Y + 1) / 2", X.upsample_add_ref(x, y, *args, source_offset=1), good)
    for dtype in X.DTYPES:
        xp = torch.randn((2, 8, 5, 7), generator=g).to(getattr(torch, dtype))
        b = torch.randn(8, generator=g).to(xp.dtype)
        good = X.pool_ref(xp, b)
        assert good.dtype == xp.dtype and torch.equal(good.float(), torch.nn.functional.max_pool2d(torch.relu(xp.float() + b.float().view(1, -1, 1, 1)), 3, 2, 1)
                                                      .to(xp.dtype).float())
        with pytest.raises(AssertionError, match="image, channel, row, column"):
            X.check_equal("pool rows 2 oy .. 2 oy + 2", X.pool_ref(xp, b, first_row=0), good)
    pos, clamped = X.relu_fractions(torch.tensor([1.0, 0.0, 2.0, 0.0]))
    assert (pos, clamped) == (0.5, 0.5)


ONE_HOT_CASES = [X._pre(2, 64, 64, 9, 7), X._pre(3, 320, 128, 5, 11, stride=2),  # noqa: SLF001  (<64, PRE> and <128, PRE>)
                 *[R.Case("head", 2, 64, cout, 9, 7, k=1, pad_lo=0, pad_hi=0) for cout in (3, 8)]]


def test_one_hot_weights_pin_the_rounding_of_the_operand():
    """With one-hot weights the float64 reference of a PRE / head case IS the float32 operand ``relu(fl32(fl32(x * sc) + sh))`` of
    the picked channels, so equality with it checks the two roundings; an operand formed by a fused multiply-add differs from it in
    at least 5 % of the elements and is rejected."""
    for case in ONE_HOT_CASES:
        data = X.make_data(case, 41)
        data["w"], picked = X.one_hot_weights(case.cout, case.cin)
        assert len(set(picked.tolist())) == case.cout and {int(p) // 4 for p in picked} != {0}
        ref = X.evaluate(case, data, (False, False, False))
        s = case.stride
        operand = X.scale_shift_ref(data["x"], data["sc"], data["sh"])[:, picked, ::s, ::s]
        assert torch.equal(ref, operand.double())
        X.check_equal(f"{case}", ref.float(), operand)
        fused = X.fused_scale_shift(data["x"], data["sc"], data["sh"])[:, picked, ::s, ::s]
        assert float((fused != operand).double().mean()) >= 0.05, case  # noqa: PLR2004
        with pytest.raises(AssertionError, match="image, channel, row, column"):
            X.check_equal(f"{case} fused operand", fused.contiguous(), operand)


def test_split_cases_run_in_two_groups_of_65_and_64():
    """``conv2d_impl`` splits a batch of more than 2 GiB of input into equal groups: restated here (``even_group``) and asserted
    for the two cases of tier 4, whose sub-batches need no split."""
    for kernel, case in X.SPLIT_CASES.items():
        assert case.n * case.h * case.w * case.cin * 4 > 2 ** 31, kernel
        assert (2 ** 31 - 1) // (case.h * case.w * case.cin * 4) == 127  # noqa: PLR2004
        assert X.conv_group(case) == 65 and case.n - 65 == 64  # noqa: PLR2004
        assert X.conv_group(case._replace(n=X.SPLIT_CHUNK)) == X.SPLIT_CHUNK and case.n % X.SPLIT_CHUNK == 0
        assert X.served(case) and X.tile_width(case) == {"post": 128, "pre": 64}[kernel]
    assert X.even_group(4096, 2047) == 1366 and X.even_group(127, 127) == 127  # noqa: PLR2004  (the header's example: 1366 + 1366 + 1364)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """An NCHW host tensor as a channels-last device tensor (dense NHWC memory whatever the extents)."""
    return t.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)


SENTINEL = 12345.0


class _Device:
    """A convolution case's operands on the device, packed for its kernel; the ``run_*`` methods return host tensors."""

    def __init__(self, case, data):
        from tiatoolbox_amd.models.architecture import fused

        self.case, self.fused = case, fused
        self.d = {k: v.cuda() for k, v in data.items() if k not in ("x", "res", "w")}
        self.x, self.res = _nhwc(data["x"]), _nhwc(data["res"])
        if case.kernel in ("post", "pre"):
            conv = torch.nn.Conv2d(case.cin, case.cout, case.k, bias=False)
            with torch.no_grad():
                conv.weight.copy_(data["w"])
            self.w = fused.pack_conv_weights(conv.cuda())
        elif case.kernel == "thin":
            self.w = fused.pack_thin_conv_weights(data["w"].cuda())
            self.x_nchw = data["x"].cuda()
        elif case.kernel == "head":
            self.w = data["w"].cuda()
        else:  # [groups][ky][kx][32][8] from OIHW [groups * 8, 32, k, k]
            self.w = data["w"].view(case.groups, 8, 32, case.k, case.k).permute(0, 3, 4, 2, 1).contiguous().cuda()

    def _args(self, epilogue):
        use_bias, use_res, relu = epilogue
        return (self.d["bias"] if use_bias else None), (self.res if use_res else None), relu

    def post(self, epilogue, want_raw):
        c = self.case
        bias, res, relu = self._args(epilogue)
        y, y2 = self.fused.hip_conv2d_post(self.x, self.w, bias, res, kernel=c.k, stride=c.stride, pad_lo=c.pad_lo, pad_hi=c.pad_hi,
                                           relu=relu, post_scale=self.d["ps"], post_shift=self.d["pt"], want_raw=want_raw)
        assert (y is not None) == want_raw and y2.shape == (c.n, c.cout, c.ho, c.wo)
        return (y.cpu() if want_raw else None), y2.cpu()

    def pre(self, epilogue):
        bias, res, relu = self._args(epilogue)
        return self.fused.hip_conv1x1_pre(self.x, self.d["sc"], self.d["sh"], self.w, bias, res, stride=self.case.stride, relu=relu).cpu()

    def thin(self, epilogue, channels_last=True):
        c = self.case
        bias, _, relu = self._args(epilogue)
        return self.fused.hip_conv2d_thin(self.x if channels_last else self.x_nchw, self.w, bias, kernel=c.k, stride=c.stride,
                                          pad_lo=c.pad_lo, pad_hi=c.pad_hi, relu=relu).cpu()

    def head(self, epilogue, pre):
        bias, _, _ = self._args(epilogue)
        sc, sh = (self.d["sc"], self.d["sh"]) if pre else (None, None)
        return self.fused.hip_conv1x1_head(self.x, self.w, bias, pre_scale=sc, pre_shift=sh).cpu()

    def gvalid(self, view):
        """Dense output, or into a channel slice (not at 0) and a row / column crop of a wider buffer filled with a sentinel: returns
        the result and whether everything outside the view still holds the sentinel."""
        c = self.case
        if not view:
            return self.fused.hip_grouped_conv_valid(self.x, self.w, groups=c.groups, kernel=c.k).cpu(), True
        wide = torch.full((c.n, c.ho + 3, c.wo + 5, c.cout + 12), SENTINEL, device="cuda").permute(0, 3, 1, 2)
        out = wide[:, 4:4 + c.cout, 1:1 + c.ho, 2:2 + c.wo]
        self.fused.hip_grouped_conv_valid(self.x, self.w, groups=c.groups, kernel=c.k, out=out)
        got = out.cpu().contiguous(memory_format=torch.channels_last)
        wide[:, 4:4 + c.cout, 1:1 + c.ho, 2:2 + c.wo] = SENTINEL
        return got, bool((wide == SENTINEL).all())


def _conv_sweep(kernel, cases, make, seed, exact):  # noqa: C901, PLR0912
    """Every epilogue (and form) of every case against its reference.  Returns the worst error relative to the gate per form."""
    worst = {}

    def note(form, ratio):
        worst[form] = max(worst.get(form, 0.0), ratio or 0.0)

    def compare(label, form, got, ref, **gate):
        if exact:
            X.check_exact(label, got, ref)
        else:
            note(form, X.check_close(label, kernel, got, ref, **gate))

    for i, case in enumerate(cases):
        data = make(case, seed + i)
        dev = _Device(case, data)
        if exact:
            assert X.fused_exact_bound(case) < 2 ** 24, case
            plain = X.evaluate(case, data, (False, False, False))
            plain = plain[0] if isinstance(plain, tuple) else plain
            assert float((plain != 0).double().mean()) >= HALF, case
        for epilogue in X.epilogues(case):
            label = f"{case} epilogue (bias, residual, relu) {epilogue}"
            relu = epilogue[2]
            if kernel == "head":
                for pre in (False, True):
                    compare(f"{label} pre {pre}", "head + pre" if pre else "head", dev.head(epilogue, pre), X.evaluate(case, data, epilogue, pre=pre))
                continue
            ref = X.evaluate(case, data, epilogue)
            if relu and case.n * case.ho * case.wo * case.cout >= 64:  # noqa: PLR2004
                pos, clamped = X.relu_fractions(ref[0] if kernel == "post" else ref)
                assert pos >= QUARTER and clamped >= QUARTER, (label, pos, clamped)
            if kernel == "post":
                tw = X.tile_width(case)
                v, y2_ref = ref
                y, y2 = dev.post(epilogue, want_raw=True)
                compare(label + " y", f"<{tw}, POST> y", y, v)
                compare(label + " y2", f"<{tw}, POST> y2", y2, y2_ref, **X.y2_gate(data["ps"]))
                if not relu and case.n * case.ho * case.wo * case.cout >= 64:  # noqa: PLR2004  (after a ReLU v >= 0 skews y2 by construction)
                    pos, clamped = X.relu_fractions(y2_ref)
                    assert pos >= QUARTER and clamped >= QUARTER, (label, "y2", pos, clamped)
                # the header's contract, bit for bit: y2 is relu(fl32(fl32(y * ps) + pt)) of the y the kernel returned
                X.check_equal(label + " y2 from y", y2, X.scale_shift_ref(y, data["ps"], data["pt"]))
                X.check_equal(label + " y2 without y", dev.post(epilogue, want_raw=False)[1], y2)
            elif kernel == "pre":
                compare(label, f"<{X.tile_width(case)}, PRE>", dev.pre(epilogue), ref)
            elif kernel == "thin":
                got = dev.thin(epilogue)
                compare(label, "thin", got, ref)
                X.check_equal(label + " NCHW-contiguous input", dev.thin(epilogue, channels_last=False), got)
            else:
                for view in (False, True):
                    got, untouched = dev.gvalid(view)
                    compare(f"{label} view {view}", "view" if view else "dense", got, ref)
                    assert untouched, f"{label}: the kernel wrote outside its output view"
    return worst


def _report(tier, kernel, worst):
    print(f"\ntier {tier} {kernel}: worst error relative to the gate per form: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert worst and 0.0 < max(worst.values()) and all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", X.CONV_KERNELS)
def test_fixed_edge_cases_match_float64(kernel):
    """Tier 1: post (``y``), pre and thin within 1e-4 (He-scaled weights), post ``y2`` within ``1e-4 * max(1, max |ps|) + 2^-23 |ref|``
    and equal, bit for bit, to ``relu(fl32(fl32(y * ps) + pt))`` of the returned ``y`` with and without ``want_raw``; head and grouped
    valid within 1e-5 of the largest reference magnitude, the latter also into a view whose surroundings must stay untouched."""
    _report(1, kernel, _conv_sweep(kernel, X.fixed_cases(kernel), X.make_data, 1000, exact=False))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", X.CONV_KERNELS)
def test_random_shapes_match_float64(kernel):
    """Tier 2: the seeded sweep at the gates of tier 1."""
    _report(2, kernel, _conv_sweep(kernel, X.random_cases(kernel), X.make_data, 2000, exact=False))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", X.CONV_KERNELS)
def test_integer_data_is_reproduced_bit_for_bit(kernel):
    """Tier 3: integer inputs, weights and per-channel vectors, every product and partial sum below 2^24 (asserted): the kernel must
    equal the float64 reference exactly, so a dropped, doubled or misplaced term shows at the element it belongs to."""
    _conv_sweep(kernel, X.exact_cases(kernel), X.make_exact_data, 3000, exact=True)


@pytest.mark.gpu
def test_pre_and_head_round_the_product_and_the_sum_of_their_operand_separately():
    """``tia_conv1x1_pre_nhwc_f32`` (both tile widths) and ``tia_conv1x1_head_nhwc_f32`` with one-hot weights return their operand
    exactly, so it must equal ``relu(fl32(fl32(x * sc) + sh))`` bit for bit: "product and sum rounded separately, like batch_norm +
    relu", interchangeable with the POST output and ``scale_shift_act``.  (A fused multiply-add -- one rounding -- differs in some
    10 % of the elements; the host test asserts at least 5 %.)"""
    for case in ONE_HOT_CASES:
        data = X.make_data(case, 41)
        data["w"], picked = X.one_hot_weights(case.cout, case.cin)
        dev = _Device(case, data)
        got = dev.pre((False, False, False)) if case.kernel == "pre" else dev.head((False, False, False), pre=True)
        s = case.stride
        X.check_equal(f"{case} one-hot weights", got, X.scale_shift_ref(data["x"], data["sc"], data["sh"])[:, picked, ::s, ::s])


def _randn(shape, seed, dtype=torch.float32):
    """Normal values of ``dtype`` on the host, [n, c, h, w] (drawn in NHWC order so that views of it are cheap to cut)."""
    n, c, h, w = shape
    return torch.randn((n, h, w, c), generator=torch.Generator().manual_seed(seed)).to(dtype).permute(0, 3, 1, 2)


def _scale_shift_case(fused, x, s, t, label):
    xd, sd, td = x.contiguous(memory_format=torch.channels_last).cuda(), s.cuda(), t.cuda()
    for relu in (True, False):
        exp = X.scale_shift_ref(x, s, t, relu)
        got = fused.hip_scale_shift_act(xd, sd, td, relu=relu)
        X.check_equal(f"scale_shift_act {label} relu {relu}", got.cpu(), exp)
        same = xd.clone()
        assert fused.hip_scale_shift_act(same, sd, td, relu=relu, inplace=True) is same
        X.check_equal(f"scale_shift_act in place {label} relu {relu}", same.cpu(), exp)


def _view_case(fused, buffer_shape, c, y0, x0, h, w, seed):
    wide = _randn(buffer_shape, seed)
    s, t = torch.randn(c, generator=torch.Generator().manual_seed(seed + 1)), torch.randn(c, generator=torch.Generator().manual_seed(seed + 2))
    dev = wide.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
    view = dev[:, :c, y0:y0 + h, x0:x0 + w]
    for relu in (True, False):
        exp = X.scale_shift_ref(wide[:, :c, y0:y0 + h, x0:x0 + w], s, t, relu).contiguous(memory_format=torch.channels_last)
        got = fused.hip_scale_shift_act_view(view, s.cuda(), t.cuda(), relu=relu)
        X.check_equal(f"scale_shift_act_view {buffer_shape} {(c, y0, x0, h, w)} relu {relu}", got.cpu(), exp)
    assert torch.equal(dev.cpu(), wide)  # the source is read only


def _upsample_case(fused, shape, seed, crop, act):
    n, c, h, w = shape
    x = _randn(shape, seed)
    y0, x0, eh, ew = X.UPSAMPLE_CROP if crop else (0, 0, 0, 0)
    skip = _randn((n, c, 2 * h + eh, 2 * w + ew), seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    s, t = (torch.randn(c, generator=g), torch.randn(c, generator=g)) if act else (None, None)
    skip_dev = skip.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)[:, :, y0:y0 + 2 * h, x0:x0 + 2 * w]
    got = fused.hip_upsample2x_add(_nhwc(x), skip_dev, s.cuda() if act else None, t.cuda() if act else None)
    exp = X.upsample_add_ref(x, skip[:, :, y0:y0 + 2 * h, x0:x0 + 2 * w], s, t)
    X.check_equal(f"upsample2x_add {shape} crop {crop} act {act}", got.cpu(), exp)
    if act:
        pos, clamped = X.relu_fractions(exp)
        assert n * c * h * w < 64 or (pos >= QUARTER and clamped >= QUARTER), (shape, pos, clamped)  # noqa: PLR2004


@pytest.mark.gpu
def test_scale_shift_and_upsample_equal_the_float32_sequence():
    """Tier 1 of ``scale_shift_act``, its view form and ``upsample2x_add(_act)``: ``x * s`` then ``+ t`` then ``max(., 0)``, each
    rounded once, by equality; in place equals out of place; views with a channel prefix, a crop with a base offset, n > 1 and a
    pixel stride above c; dense and cropped skips."""
    from tiatoolbox_amd.models.architecture import fused

    for i, shape in enumerate(X.SCALE_SHIFT_SHAPES):
        g = torch.Generator().manual_seed(40 + i)
        _scale_shift_case(fused, _randn(shape, 400 + i), torch.randn(shape[1], generator=g), torch.randn(shape[1], generator=g), shape)
    for i, (buffer_shape, c, y0, x0, h, w) in enumerate(X.SCALE_SHIFT_VIEWS):
        _view_case(fused, buffer_shape, c, y0, x0, h, w, 500 + 3 * i)
    for i, shape in enumerate(X.UPSAMPLE_SHAPES):
        for crop in (False, True):
            for act in (False, True):
                _upsample_case(fused, shape, 600 + 3 * i, crop, act)


def _bias_act_case(fused, x, bias, res, label):
    xd, bd, rd = x.contiguous(memory_format=torch.channels_last).cuda(), bias.cuda(), res.contiguous(memory_format=torch.channels_last).cuda()
    for use_res in (False, True):
        for relu in (False, True):
            got = fused.hip_bias_act_(xd.clone(), bd, rd if use_res else None, relu=relu)
            X.check_equal(f"bias_act {label} residual {use_res} relu {relu}", got.cpu(), X.bias_act_ref(x, bias, res if use_res else None, relu))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", X.DTYPES)
def test_bias_act_and_pool_round_once(dtype):
    """Tiers 1 and 3 of ``bias_act`` and ``bias_relu_maxpool``: ``(x + b) + r``, ``max(., 0)`` (and the 3 x 3 / 2 maximum with windows
    cut on every side) in float32 and ONE rounding to the tensor's type, by equality -- on normal data, on all-negative data (every
    pooled value exactly 0), and for fp16 / bf16 on integer data whose sums lie beyond the integers the type holds exactly, where a
    tie or a second rounding shows (the share of such sums is asserted on the host)."""
    from tiatoolbox_amd.models.architecture import fused

    dt = getattr(torch, dtype)
    for i, shape in enumerate(X.BIAS_ACT_SHAPES):
        b = torch.randn(shape[1], generator=torch.Generator().manual_seed(70 + i)).to(dt)
        _bias_act_case(fused, _randn(shape, 700 + i, dt), b, _randn(shape, 750 + i, dt), f"{dtype} {shape}")
        if dtype != "float32":
            _bias_act_case(fused, *X.make_half_integer_data(shape, dtype, 800 + i), f"{dtype} integers {shape}")
    for i, (h, w) in enumerate(X.POOL_HW):
        shape = (2 + i % 2, X.POOL_CHANNELS[i % 3], h, w)
        b = torch.randn(shape[1], generator=torch.Generator().manual_seed(90 + i)).to(dt)
        inputs = [("normal", _randn(shape, 900 + i, dt), b), ("all negative", -_randn(shape, 950 + i, dt).abs() - 1, -b.abs())]
        if dtype != "float32":
            xi, bi, _ = X.make_half_integer_data(shape, dtype, 980 + i)
            inputs.append(("integers", xi, bi))
        for name, x, bias in inputs:
            got = fused.hip_bias_relu_maxpool(x.contiguous(memory_format=torch.channels_last).cuda(), bias.cuda()).cpu()
            X.check_equal(f"bias_relu_maxpool {dtype} {name} {shape}", got, X.pool_ref(x, bias))
            assert name != "all negative" or float(got.float().abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(X.BEYOND_CAP))
def test_grid_stride_loops_beyond_the_grid_cap(kernel):
    """One case per capped kernel with more than twice the cap's work (asserted on the host): every thread runs its loop body more
    than once, the head's waves their lane exchanges in a second and third pass.  Same references and comparisons as tier 1."""
    from tiatoolbox_amd.models.architecture import fused

    shape, dtype = X.BEYOND_CAP[kernel]
    dt = getattr(torch, dtype)
    n, c, h, w = shape
    g = torch.Generator().manual_seed(11)
    if kernel == "bias_act":
        x, res, b = _randn(shape, 12, dt), _randn(shape, 13, dt), torch.randn(c, generator=g).to(dt)
        got = fused.hip_bias_act_(x.contiguous(memory_format=torch.channels_last).cuda(), b.cuda(), res.contiguous(memory_format=torch.channels_last).cuda())
        X.check_equal(f"bias_act {shape}", got.cpu(), X.bias_act_ref(x, b, res, relu=True))
    elif kernel == "pool":
        x, b = _randn(shape, 14, dt), torch.randn(c, generator=g).to(dt)
        got = fused.hip_bias_relu_maxpool(x.contiguous(memory_format=torch.channels_last).cuda(), b.cuda())
        X.check_equal(f"bias_relu_maxpool {shape}", got.cpu(), X.pool_ref(x, b))
    elif kernel == "scale_shift":
        x, s, t = _randn(shape, 15), torch.randn(c, generator=g), torch.randn(c, generator=g)
        got = fused.hip_scale_shift_act(x.contiguous(memory_format=torch.channels_last).cuda(), s.cuda(), t.cuda())
        X.check_equal(f"scale_shift_act {shape}", got.cpu(), X.scale_shift_ref(x, s, t))
    elif kernel == "scale_shift_view":
        _view_case(fused, (n, c + 8, h + 2, w), c, 1, 0, h, w, 16)
    elif kernel == "upsample":
        _upsample_case(fused, shape, 17, crop=True, act=True)
    else:
        case = R.Case("head", n, 64, 3, h, w, k=1, pad_lo=0, pad_hi=0)
        data = X.make_data(case, 18)
        dev = _Device(case, data)
        ratio = X.check_close(f"{case}", "head", dev.head((True, False, False), pre=True), X.evaluate(case, data, (True, False, False)))
        print(f"\nhead beyond the grid cap: {ratio:.3f} of the gate")
        assert ratio > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(X.SPLIT_CASES))
def test_batches_beyond_2gib_run_in_groups_bit_identically_and_match_float64(kernel):
    """Tier 4: a 1x1 POST (``<128, true>``) and a PRE (``<64, false, true>``) convolution of 129 maps of 64 x 64 x 1024 -- just over
    2 GiB of input, launched as 65 + 64 images -- with a residual: (a) bit-identical to the same call over three sub-batches of 43
    that need no split, every output; (b) the first image, the images on both sides of the group boundary and the last image within
    the tier-1 gates of the float64 reference."""
    from tiatoolbox_amd.models.architecture import fused

    case = X.SPLIT_CASES[kernel]
    group, chunk, n = X.conv_group(case), X.SPLIT_CHUNK, case.n
    assert group == 65 and n * case.h * case.w * case.cin * 4 > 2 ** 31 > chunk * case.h * case.w * case.cin * 4  # noqa: PLR2004
    small = X.make_data(case._replace(n=1, h=1, w=1), 31)  # weights, bias and the per-channel vectors
    conv = torch.nn.Conv2d(case.cin, case.cout, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(small["w"])
    packed = fused.pack_conv_weights(conv.cuda())
    dev = {k: small[k].cuda() for k in ("bias", "ps", "pt", "sc", "sh")}
    g = torch.Generator(device="cuda").manual_seed(32)
    x = torch.randn((n, case.h, case.w, case.cin), device="cuda", generator=g).permute(0, 3, 1, 2)
    res = torch.randn((n, case.ho, case.wo, case.cout), device="cuda", generator=g).permute(0, 3, 1, 2)

    def run(a, b):
        if kernel == "post":
            return fused.hip_conv2d_post(x[a:b], packed, dev["bias"], res[a:b], kernel=1, stride=1, pad_lo=0, pad_hi=0, relu=False,
                                         post_scale=dev["ps"], post_shift=dev["pt"])
        return (fused.hip_conv1x1_pre(x[a:b], dev["sc"], dev["sh"], packed, dev["bias"], res[a:b], relu=True),)

    whole = run(0, n)
    parts = [run(a, a + chunk) for a in range(0, n, chunk)]
    same = [torch.equal(whole[j], torch.cat([p[j] for p in parts])) for j in range(len(whole))]
    del parts
    images = sorted({0, group - 1, group, n - 1})
    idx = torch.tensor(images, device="cuda")
    x_cpu, res_cpu, got = x[idx].cpu(), res[idx].cpu(), [t[idx].cpu() for t in whole]
    del x, res, whole
    gc.collect()
    torch.cuda.empty_cache()
    assert all(same), (kernel, same, "the split batch differs from its unsplit sub-batches")
    sub = case._replace(n=len(images))
    data = dict(small, x=x_cpu, res=res_cpu)
    ref = X.evaluate(sub, data, (True, True, kernel == "pre"))
    for j, image in enumerate(images):
        label = f"{kernel} split, image {image}"
        if kernel == "post":
            r_y = X.check_close(label + " y", "post", got[0][j:j + 1], ref[0][j:j + 1])
            r_y2 = X.check_close(label + " y2", "post", got[1][j:j + 1], ref[1][j:j + 1], **X.y2_gate(small["ps"]))
            X.check_equal(label + " y2 from y", got[1][j:j + 1], X.scale_shift_ref(got[0][j:j + 1], small["ps"], small["pt"]))
            print(f"\n{label}: y {r_y:.3f}, y2 {r_y2:.3f} of the gate")
        else:
            print(f"\n{label}: {X.check_close(label, 'pre', got[0][j:j + 1], ref[j:j + 1]):.3f} of the gate")

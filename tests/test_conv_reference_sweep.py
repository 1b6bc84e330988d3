"""Every hand-written convolution kernel -- float32 direct (``tia_conv2d_nhwc_f32_ex``: tap-reuse blocks, bands, slice kernel, ring),
Winograd F(2x2) and F(4x2), fp16 / bf16 (``tia_conv2d_nhwc_h``) and the grouped 3x3 -- against ``torch.nn.functional.conv2d`` on the
CPU in FLOAT64 on exactly the values the kernel is given, followed by bias, residual and ReLU in float64; never against another
kernel of this library.  Four tiers:

1. fixed rectangular and edge cases per kernel at the gate the project holds that kernel to, every epilogue combination;
2. a seeded random sweep (``h`` and ``w`` drawn independently) at the same gates, which proves through the library's host-only
   route queries that it reached every form of every kernel with maps that are not square;
3. integer data, where float32 accumulation is exact in any order and the kernel must equal the reference bit for bit (for the
   half kernel: one rounding of the exact value) -- independent of any tolerance;
4. the > 2 GiB batch split of F(4x2), bit-identical to unsplit sub-batches and tied to the float64 reference at the group boundaries.

Helpers, case lists and bounds are in ``tests/_conv_ref.py``; the tests without the ``gpu`` mark check them on the host, including that
the comparisons fail for a reference that is wrong in the ways a kernel can be (``h`` / ``w`` swapped, a tap or a channel dropped,
a second rounding to half)."""

from __future__ import annotations

import gc
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _conv_ref as R  # noqa: E402, N812

KERNELS = ("direct", "half", "wino22", "wino42", "grouped")


def _lib_or_skip():
    from tiatoolbox_amd import _lib, build

    if not build.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------------------------
# host only: reference helpers, case generation, bounds, coverage, and the comparisons' own sensitivity
# ------------------------------------------------------------------------------------------------------------------------------------
def test_reference_matches_a_hand_computed_3x3_example():
    """One channel, 2 x 3 map, border 1 in front and 0 behind, written out by hand; then bias / residual / ReLU; then stride 2."""
    x = torch.tensor([[[[1., 2., 3.], [4., 5., 6.]]]])
    w = torch.tensor([[[[1., 0., -1.], [2., 0., -2.], [0., 3., 0.]]]])
    case = R.Case("direct", 1, 1, 1, 2, 3, pad_lo=1, pad_hi=0)
    assert (case.ho, case.wo) == (1, 2)
    # output (0, 0): window rows {-1, 0, 1} x columns {-1, 0, 1}: 2 * 0 - 2 * 2 (row 0) + 3 * 4 (row 1, centre) = 8
    # output (0, 1): columns {0, 1, 2}: 2 * 1 - 2 * 3 (row 0) + 3 * 5 (row 1, centre) = 11
    lin = R.conv_ref64(case, x, w)
    assert lin.dtype == torch.float64 and lin.tolist() == [[[[8.0, 11.0]]]]
    res = torch.tensor([[[[-10.0, 0.5]]]])
    assert R.epilogue64(lin, torch.tensor([1.0]), res, relu=False).tolist() == [[[[-1.0, 12.5]]]]
    assert R.epilogue64(lin, torch.tensor([1.0]), res, relu=True).tolist() == [[[[0.0, 12.5]]]]
    assert R.epilogue64(lin, None, None, relu=False) is lin
    # stride 2, "same": outputs at rows {0}, columns {0, 2}; (0, 0) = 2*0 - 2*2 + 3*4 = 8; (0, 1): columns {1, 2, 3}: 2*2 - 0 + 3*6 = 22
    case = R.Case("direct", 1, 1, 1, 2, 3, stride=2)
    assert R.conv_ref64(case, x, w).tolist() == [[[[8.0, 22.0]]]]
    # grouped: two groups of one channel are two independent convolutions
    case = R.Case("grouped", 1, 2, 2, 2, 3, groups=2)
    both = R.conv_ref64(case, torch.cat([x, 2 * x], 1), torch.cat([w, w]))
    assert torch.equal(both[:, 1], 2 * both[:, 0])
    assert R.worst_element(torch.tensor([[[[0.0, 1.0], [5.0, 2.0]]]])) == (0, 0, 1, 0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_cases_are_what_the_entry_points_serve(kernel):
    """Fixed, random and exact cases: channel multiples, borders, strides and output sizes inside what each entry point documents;
    the lists hold the shapes the tiers are about; the random draw is reproducible."""
    assert R.random_cases(kernel) == R.random_cases(kernel)
    for c in R.fixed_cases(kernel) + R.random_cases(kernel) + R.exact_cases(kernel):
        assert c.kernel == kernel and 1 <= c.n <= 9 and c.ho >= 1 and c.wo >= 1 and c.h >= 1 and c.w >= 1, c  # noqa: PLR2004
        if kernel in ("wino22", "wino42"):
            assert c.cin % 16 == 0 and c.cout % 64 == 0 and (c.k, c.stride) == (3, 1) and 0 <= c.pad_lo <= 2 and 0 <= c.pad_hi <= 2, c  # noqa: PLR2004
            assert c.ho - 1 - c.pad_lo < c.h and c.wo - 1 - c.pad_lo < c.w, c
        elif kernel == "grouped":
            assert c.cin == c.cout and c.cin % c.groups == 0 and c.cin // c.groups in R.GROUPED_P and c.stride in (1, 2), c
            assert (c.k, c.pad_lo, c.pad_hi) == (3, 1, 1), c
        else:
            assert c.cin % 32 == 0 and c.cout % 64 == 0 and c.pad_lo < c.k, c
            assert (c.ho - 1) * c.stride - c.pad_lo < c.h and (c.wo - 1) * c.stride - c.pad_lo < c.w, c
            assert kernel == "direct" or (c.pad_lo == c.pad_hi and c.dtype in R.HALF_EPS), c
    fixed = R.fixed_cases(kernel)
    shapes = {(c.h, c.w) for c in fixed}
    assert sum(c.h != c.w for c in fixed) >= len(fixed) // 2
    if kernel in ("wino22", "wino42"):
        assert {(32, 16), (16, 32), (16, 48), (8, 3), (3, 8), (1, 8), (8, 1), (5, 7), (1, 1), (30, 18), (18, 30), (17, 33), (36, 20),
                (13, 40)} <= shapes
        assert {(c.pad_lo, c.pad_hi) for c in fixed} == {(1, 1), (0, 0), (2, 2), (0, 1), (1, 0), (2, 1)}
        assert {c.n for c in fixed if c.ho <= 8 and c.wo <= 8} >= {1, 3, 4, 5, 9}  # noqa: PLR2004
        assert {c.cin for c in fixed} >= {16, 48, 512} and {c.cout for c in fixed} >= {64, 192}
        assert any(c.ho % 4 and c.wo % 2 for c in fixed) and any(c.ho % 4 == 0 and c.wo % 2 for c in fixed)
        assert any(c.ho % 4 and c.wo % 2 == 0 for c in fixed)
    if kernel == "wino22":
        assert {(14, 28), (28, 14), (21, 56), (56, 7), (9, 42), (37, 12), (44, 30)} <= shapes
    if kernel == "direct":
        assert {c.w for c in fixed} >= {7, 14, 21, 28, 42, 56} and {c.h for c in fixed} >= {7, 14, 21, 28, 42, 56}
        assert {(c.pad_lo, c.pad_hi) for c in fixed if c.k == 3 and c.stride == 1} >= {(0, 1), (1, 0), (2, 2)}  # noqa: PLR2004
        assert any(c.k == 1 and c.stride == 2 and c.h != c.w for c in fixed)  # noqa: PLR2004
        assert any(c.k == 3 and c.stride == 2 and c.h % 2 != c.w % 2 for c in fixed)  # noqa: PLR2004
    if kernel == "half":
        for dtype in R.HALF_EPS:
            assert {(33, 55), (55, 33), (28, 42), (15, 64)} <= {(c.h, c.w) for c in fixed if c.dtype == dtype}
            assert any(c.stride == 2 and c.h % 2 and c.w % 2 for c in fixed if c.dtype == dtype)  # noqa: PLR2004
    if kernel == "grouped":
        assert {(c.groups, c.cin // c.groups) for c in fixed} == {(g, cg) for g in (1, 3, 5, 32, 33, 64) for cg in (4, 8, 16, 32, 64)}
        assert {c.n for c in fixed} >= {1, 3, 7}
        for cg, p in R.GROUPED_P.items():
            pixels = {c.n * c.ho * c.wo for c in fixed if c.cin // c.groups == cg}
            assert {64 * p - 1, 64 * p, 64 * p + 1, 1} <= pixels, (cg, sorted(pixels))
            mine = [c for c in fixed if c.cin // c.groups == cg]
            assert any(c.h == 1 and c.w > 1 for c in mine) and any(c.w == 1 and c.h > 1 for c in mine)
            assert any((c.h, c.w, c.stride) == (2, 2, 2) for c in mine)


def test_window_cases_take_windows_with_a_partial_last_block():
    import ctypes

    lib = _lib_or_skip()
    for c in R.WINDOW_CASES:
        geom = (ctypes.c_int32 * 4)()
        assert lib.tia_conv3x3_wino_geometry(c.n, c.ho, c.wo, geom) == 2, c  # noqa: PLR2004
        wg, _, _, windows = geom
        assert (c.n * windows) % wg != 0, (c, list(geom))
        assert c.h != c.w


@pytest.mark.parametrize("kernel", ["direct", "wino22", "wino42"])
def test_random_sweep_reaches_every_form_with_maps_that_are_not_square(kernel):
    """Through the host-only queries (``tia_conv2d_route_f32``, ``tia_conv3x3_geometry``, ``tia_conv3x3_wino_geometry``; a host without
    a device answers for the MI355X's 256 CUs): at least four cases with ``h != w`` on every form; the fixed and the exact tier reach
    every form as well.  F(4x2) has two geometries, chosen by the output size alone (at most 8 x 8: four images per block)."""
    lib = _lib_or_skip()
    counts = R.non_square_form_counts(lib, R.random_cases(kernel))
    for form in R.REQUIRED_FORMS[kernel]:
        assert counts.get(form, 0) >= R.FORM_FLOOR, (kernel, counts)
    for cases in (R.fixed_cases(kernel), R.exact_cases(kernel)):
        counts = R.non_square_form_counts(lib, cases)
        assert all(counts.get(form, 0) >= 1 for form in R.REQUIRED_FORMS[kernel]), (kernel, counts)
    if kernel == "wino42":  # the shapes the fused resnet blocks really route to F(4x2)
        for h, w in ((32, 16), (16, 32), (8, 3), (3, 8), (1, 8), (5, 7)):
            assert lib.tia_conv3x3_wino_form(8, h, w, 64, 64, 1) == 1, (h, w)


@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_tier_stays_below_2_to_24(kernel):
    """The bound behind "float32 accumulation is exact": derived from the transform matrices' absolute row sums, the value ranges and
    the channel count, asserted for every exact case; Winograd weights of the tier transform to integers; F(4x2)'s limit on the
    channel count is what the bound gives, not an estimate."""
    for c in R.exact_cases(kernel):
        assert R.exact_bound(c) < 2 ** 24, (c, R.exact_bound(c))
        if kernel in ("wino22", "wino42"):
            assert R.wino_weights_are_integral(c, R.make_exact_data(c._replace(n=1, h=3, w=3), 1)[1]), c
    if kernel == "wino42":
        assert R.exact_bound(R.Case("wino42", 1, 192, 64, 8, 8)) < 2 ** 24 <= R.exact_bound(R.Case("wino42", 1, 208, 64, 8, 8))
        odd = torch.full((64, 16, 3, 3), 4.0)  # multiples of 4 are enough for F(2x2), not for F(4x2)
        assert R.wino_weights_are_integral(R.Case("wino22", 1, 16, 64, 8, 8), odd)
        assert not R.wino_weights_are_integral(R.Case("wino42", 1, 16, 64, 8, 8), odd)
    if kernel == "direct":
        assert R.exact_bound(R.Case("direct", 1, 64, 64, 8, 8)) == 9 * 64 * 2 + 64 + 64


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_exact_half_results_lie_where_a_second_rounding_shows(dtype):
    """The half cases of the exact tier with bias and residual: at least half of the results beyond the integers half holds exactly
    (256 for bf16, 2048 for fp16), at least a quarter of them not representable before the one rounding -- and a reference that rounds
    to half BEFORE adding the residual differs, so ``check_exact`` pins "float32 sum of convolution, bias and residual, ReLU, ONE
    rounding".  Without bias and residual the results are small integers (exact in half): that combination checks the sums only."""
    dt = getattr(torch, dtype)
    for case in [c for c in R.exact_cases("half") if c.dtype == dtype]:
        x, w, bias, res = R.make_exact_data(case, 5)
        lin = R.conv_ref64(case, x, w)
        exact = R.epilogue64(lin, bias, res, relu=False)
        assert float((exact.abs() > R.HALF_INTEGER_LIMIT[dtype]).double().mean()) >= 0.5, case  # noqa: PLR2004
        assert float((R.to_half_once(exact, dt).double() != exact).double().mean()) >= 0.25, case  # noqa: PLR2004
        assert float(exact.abs().max()) < 65504 / 2
        good = R.to_half_once(exact, dt)
        R.check_exact(case, (True, True, False), good, exact)
        twice = (R.to_half_once(R.epilogue64(lin, bias, None, relu=False), dt).float() + res).to(dt)  # conv + bias rounded, then + residual
        assert float((twice != good).double().mean()) >= 0.05  # noqa: PLR2004
        with pytest.raises(AssertionError, match="elements differ"):
            R.check_exact(case, (True, True, False), twice, exact)
        bias_in_half = (R.to_half_once(lin, dt).float() + bias.to(dt).float().view(1, -1, 1, 1)).to(dt)  # bias added to a rounded sum
        with pytest.raises(AssertionError, match="elements differ"):
            R.check_exact(case, (True, False, False), bias_in_half, R.epilogue64(lin, bias, None, relu=False))
        relu_first = (torch.relu(lin + bias.view(1, -1, 1, 1)) + res).float().to(dt)  # ReLU before the residual
        with pytest.raises(AssertionError, match="elements differ"):
            R.check_exact(case, (True, True, True), relu_first, R.epilogue64(lin, bias, res, relu=True))


def _wrong_references(case, x, w):
    """What a kernel with a row / column mix-up, a dropped tap or a dropped input channel would compute."""
    swapped = R.conv_ref64(case._replace(h=case.w, w=case.h), x.transpose(2, 3), w).transpose(2, 3)  # the filter applied transposed
    w_tap = w.clone()
    w_tap[:, :, 0, 2] = 0
    x_ch = x.clone()
    x_ch[:, case.cin // case.groups - 1] = 0
    return {"h and w swapped": swapped, "one tap zeroed": R.conv_ref64(case, x, w_tap), "one channel dropped": R.conv_ref64(case, x_ch, w)}


@pytest.mark.parametrize("kernel", KERNELS)
def test_comparisons_fail_for_a_subtly_wrong_reference(kernel):
    """The sanity check of the tests themselves, without a kernel: the true float64 result rounded to the kernel's output type passes
    tier 1 and tier 3 for a rectangular case; the result with ``h`` and ``w`` swapped, with one tap zeroed, with one input channel
    dropped fails both."""
    case = next(c for c in R.fixed_cases(kernel) if c.h != c.w and c.h > 4 and c.w > 4 and c.cin // c.groups >= 16)  # noqa: PLR2004
    out_dt = getattr(torch, case.dtype)
    for tier, make, check in (("tolerance", R.make_data, R.check_tolerance), ("exact", R.make_exact_data, R.check_exact)):
        x, w, bias, res = make(case, 3)
        lin = R.conv_ref64(case, x, w)
        for epilogue in R.epilogues(case):
            use_bias, use_res, relu = epilogue
            args = (bias if use_bias else None, res if use_res else None, relu)
            ref = R.epilogue64(lin, *args)
            check(case, epilogue, ref.float().to(out_dt), ref)
            for name, wrong in _wrong_references(case, x, w).items():
                with pytest.raises(AssertionError, match="image, channel, row, column"):
                    check(case, epilogue, R.epilogue64(wrong, *args).float().to(out_dt), ref)
                    pytest.fail(f"{tier} tier accepted '{name}' for {case} {epilogue}")
        assert float((lin != 0).double().mean()) > 0.5  # noqa: PLR2004


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def _nhwc(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """An NCHW host tensor as a channels-last device tensor (dense NHWC memory whatever the extents)."""
    return t.to(dtype).permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)


class _Device:
    """A case's operands on the device, packed for its kernel; ``run`` returns the kernel's output on the host."""

    def __init__(self, case, x, weight, bias, res):
        from tiatoolbox_amd.models.architecture import fused

        self.case, self.fused = case, fused
        self.dt = getattr(torch, case.dtype)
        conv = torch.nn.Conv2d(case.cin, case.cout, case.k, stride=case.stride, groups=case.groups, bias=False)
        with torch.no_grad():
            conv.weight.copy_(weight)
        conv = conv.cuda()
        pack = {"direct": fused.pack_conv_weights, "wino22": fused.pack_conv_weights_wino, "wino42": fused.pack_conv_weights_wino42,
                "grouped": fused.pack_grouped_conv_weights, "half": lambda m: fused.pack_conv_weights_h(m, self.dt)}[case.kernel]
        self.packed = pack(conv)
        self.x, self.res, self.bias = _nhwc(x, self.dt), _nhwc(res, self.dt), bias.cuda()

    def run(self, epilogue) -> torch.Tensor:
        c, f = self.case, self.fused
        use_bias, use_res, relu = epilogue
        bias, res = self.bias if use_bias else None, self.res if use_res else None
        if c.kernel == "direct":
            y = f.hip_conv2d_ex(self.x, self.packed, bias, res, kernel=c.k, stride=c.stride, pad_lo=c.pad_lo, pad_hi=c.pad_hi, relu=relu)
        elif c.kernel == "half":
            y = f.hip_conv2d_h(self.x, self.packed, bias, res, cout=c.cout, kernel=c.k, stride=c.stride, padding=c.pad_lo, relu=relu)
        elif c.kernel == "grouped":
            y = f.hip_conv3x3_grouped(self.x, self.packed, bias, stride=c.stride, relu=relu)
        else:
            y = f.hip_conv3x3_wino(self.x, self.packed, bias, res, padding=c.pad_lo, pad_hi=c.pad_hi, relu=relu)
        assert y.shape == (c.n, c.cout, c.ho, c.wo) and y.dtype == self.dt, (c, tuple(y.shape), y.dtype)
        return y.cpu()


def _sweep(cases, make, check, seed, on_reference=None):
    """Every epilogue of every case against the float64 reference (computed once per case; ``on_reference(case, lin)`` may assert on
    it).  Returns the worst figure ``check`` reports per form."""
    from tiatoolbox_amd import _lib

    lib, worst = _lib.load(), {}
    for i, case in enumerate(cases):
        x, w, bias, res = make(case, seed + i)
        lin = R.conv_ref64(case, x, w)
        if on_reference is not None:
            on_reference(case, lin)
        dev = _Device(case, x, w, bias, res)
        for epilogue in R.epilogues(case):
            use_bias, use_res, relu = epilogue
            ref = R.epilogue64(lin, bias if use_bias else None, res if use_res else None, relu)
            ratio = check(case, epilogue, dev.run(epilogue), ref)
            form = (case.dtype + " " if case.kernel == "half" else "") + R.form_of(lib, case)
            worst[form] = max(worst.get(form, 0.0), ratio or 0.0)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_fixed_rectangular_cases_match_float64(kernel):
    """Tier 1: max |delta| <= 1e-5 of the largest reference magnitude for F(2x2), F(4x2) and the grouped kernel, |delta| <= 1e-4 for the
    float32 direct kernel (He-scaled weights), ``eps * |ref| + 1e-4 * max |ref|`` per element for fp16 / bf16; every epilogue
    combination on every case.  A failure names the case and the element."""
    worst = _sweep(R.fixed_cases(kernel), R.make_data, R.check_tolerance, seed=1000)
    print(f"\ntier 1 {kernel}: worst error relative to the gate per form: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert 0.0 < max(worst.values()) <= 1.0  # (a kernel that equalled float64 exactly would not be a float32 kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_random_shapes_match_float64(kernel):
    """Tier 2: the seeded sweep at the gates of tier 1; no case is skipped, a non-zero return code raises."""
    worst = _sweep(R.random_cases(kernel), R.make_data, R.check_tolerance, seed=2000)
    print(f"\ntier 2 {kernel}: worst error relative to the gate per form: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert 0.0 < max(worst.values()) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_integer_data_is_reproduced_bit_for_bit(kernel):
    """Tier 3: small integer inputs and weights (``_conv_ref.EXACT_RANGES``), every partial sum below 2^24 (asserted), so the kernel
    must equal the float64 reference exactly: any dropped, doubled or misplaced term shows, at the element it belongs to.  The half
    kernel must return ONE rounding of the exact float32 sum of convolution, bias and residual after the ReLU."""
    def not_trivial(case, lin):
        assert R.exact_bound(case) < 2 ** 24, case
        assert float((lin != 0).double().mean()) >= 0.5, case  # noqa: PLR2004  (the reference is not trivially zero)
        assert torch.equal(lin, lin.round()) and float(lin.abs().max()) < 2 ** 24

    _sweep(R.exact_cases(kernel), R.make_exact_data, R.check_exact, seed=3000, on_reference=not_trivial)


def _f42_group(n: int, h: int, w: int, cin: int) -> int:
    """Images per launch of ``tia_conv3x3_wino42_nhwc_f32`` as its header documents the split: groups of < 2 GiB of input, equal
    (``ceil(n / k)`` for the smallest ``k`` that fits), whole blocks of four images for maps of at most 8 x 8."""
    limit = (2 ** 31 - 1) // (h * w * cin * 4)
    small = h <= 8 and w <= 8  # noqa: PLR2004
    if small:
        limit -= limit % 4
    if n <= limit:
        return n
    k = -(-n // limit)
    even = -(-n // k)
    return -(-even // 4) * 4 if small else even


@pytest.mark.gpu
@pytest.mark.parametrize(("n", "hw", "chunk"), [(17001, 8, 5668), (4101, 16, 1368)])
def test_f42_batches_beyond_2gib_run_in_groups_bit_identically_and_match_float64(n, hw, chunk):
    """Tier 4: ``tia_conv3x3_wino42_nhwc_f32`` over a batch of 512-channel maps just beyond 2 GiB of input (8 x 8: four-image blocks,
    groups rounded to whole blocks, a batch size that is no multiple of 4; 16 x 16: blocks of 16 x 16) is (a) bit-identical to the same
    call over sub-batches that need no split and whose sizes are multiples of 4, and (b) within the 1e-5 gate of the float64 reference
    for the first image, the images on both sides of every internal group boundary and the last image."""
    from tiatoolbox_amd.models.architecture.fused import hip_conv3x3_wino, pack_conv_weights_wino42

    cin, cout = 512, 64
    assert n * hw * hw * cin * 4 > 2 ** 31 and chunk % 4 == 0 and chunk * hw * hw * cin * 4 < 2 ** 31 and (hw > 8 or n % 4)  # noqa: PLR2004
    group = _f42_group(n, hw, hw, cin)
    assert group < n and (hw > 8 or group % 4 == 0)  # noqa: PLR2004
    g = torch.Generator(device="cuda").manual_seed(17)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=torch.Generator().manual_seed(18)) * (2.0 / (9 * cin)) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=torch.Generator().manual_seed(19)) * 0.1)
    w_cpu, b_cpu = conv.weight.detach().clone(), conv.bias.detach().clone()
    conv = conv.cuda()
    up = pack_conv_weights_wino42(conv)
    x = torch.randn((n, hw, hw, cin), device="cuda", generator=g).permute(0, 3, 1, 2)
    res = torch.randn((n, hw, hw, cout), device="cuda", generator=g).permute(0, 3, 1, 2)
    whole = hip_conv3x3_wino(x, up, conv.bias, res, padding=1, relu=True)
    parts = torch.cat([hip_conv3x3_wino(x[a:a + chunk], up, conv.bias, res[a:a + chunk], padding=1, relu=True) for a in range(0, n, chunk)])
    same = torch.equal(whole, parts)
    del parts
    images = sorted({0, n - 1} | {i for b in range(group, n, group) for i in (b - 1, b)})
    assert len(images) >= 4  # noqa: PLR2004
    idx = torch.tensor(images, device="cuda")
    x_cpu, res_cpu, got = x[idx].cpu(), res[idx].cpu(), whole[idx].cpu()
    del x, res, whole
    gc.collect()
    torch.cuda.empty_cache()
    assert same, (n, hw, "the split batch differs from its unsplit sub-batches")
    case = R.Case("wino42", len(images), cin, cout, hw, hw)
    ref = R.epilogue64(R.conv_ref64(case, x_cpu, w_cpu), b_cpu, res_cpu, relu=True)
    for j, image in enumerate(images):
        one = case._replace(n=1)
        ratio, where = R.tolerance_ratio(one, got[j:j + 1], ref[j:j + 1])
        assert ratio <= 1.0, (n, hw, group, f"image {image}", where, ratio)

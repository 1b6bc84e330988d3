"""Every kernel ``ReinhardNormalizer.transform`` / ``lab_statistics`` can reach (csrc/lab.hip: the eight register-resident forms, the
scratch-slot kernel, the three-launch form wide and scalar; each in its statistics-only variant too) against the oracle
(``oracle.stain`` Reinhard on ``oracle.cvref``), bit for bit -- the chain is integer Lab and byte tables.  Beyond the shapes: more
patches than persistent workgroups (the LDS union is re-used from patch to patch), a zero standard deviation on every route, bases
that are not 16-byte aligned, batches beyond the 65535-image launch limit, and guard bytes around the output of the direct calls.

The single tolerance is ``atol=1e-9`` on the statistics against the oracle (inherited from test_reinhard.py: the oracle sums pixels,
the kernels sum 256 weighted bins).  The host-only tests prove that the shape table reaches every kernel and that the oracle alone
meets every precondition the GPU tests lean on."""

from __future__ import annotations

import ctypes as C

import _reinhard_ref as R
import numpy as np
import pytest

GUARD = 4096   # bytes of canary on either side of a direct call's output, and of slack behind its workspace
CANARY = 0xA5
NCHUNK = 65535 + 7


def _id(shape) -> str:
    return f"{shape[0]}x{shape[1]}"


# ------------------------------------------------------------------------------------------------------------------------------------
# host only
# ------------------------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_kernel():
    assert {k for k in R.SHAPES if k[0] == "resident"} == {("resident", g) for g in R.LADDER}
    assert {("fused", None), ("three_scalar", None), ("three_wide", None)} <= set(R.SHAPES)
    for key, shapes in R.SHAPES.items():
        for h, w in shapes:
            assert R.route(h, w) == key, (h, w)
    assert len(set(R.ALL_SHAPES)) == len(R.ALL_SHAPES)
    # the limits and their neighbours; what alignment changes
    assert R.route(256, 256) == ("resident", 16) and R.route(257, 256) == ("fused", None)
    assert R.route(512, 512) == ("fused", None) and R.route(1025, 256) == ("three_scalar", None)
    assert R.route(1024, 1536) == ("three_wide", None)
    assert R.route(256, 256, align=4) == ("resident", 16) and R.route(320, 320, align=4) == ("fused", None)
    assert R.route(257, 1024, align=4) == ("three_scalar", None)
    for h, w in ((256, 256), (320, 320), (257, 1024)):
        assert R.route(h, w, aligned=False) == ("three_scalar", None)
    assert all(R.route(*s)[0] != "resident" or (s[0] * s[1]) % 4 == 0 for s in R.ALL_SHAPES)
    assert sorted(R.route(*s)[0] for s in R.ZERO_STD_SHAPES) == ["fused", "resident", "resident", "three_scalar", "three_wide"]
    assert R.route(*R.FLAT_SHAPE) == ("fused", None) and R.route(3, 3) == ("three_scalar", None)


def test_table_has_full_and_ragged_shapes_of_every_form():
    """Per NG above 1: a shape that needs every group of the form, and one that leaves the last group ragged or wholly idle.  The
    scratch-slot kernel: every remainder of the wave steps modulo its four waves."""
    for ng in R.LADDER[1:]:
        shapes = R.SHAPES[("resident", ng)]
        assert any(R.need(h, w) == ng for h, w in shapes), ng
        assert any(R.need(h, w) < ng or ((h * w) >> 2) % R.RESIDENT_THREADS for h, w in shapes), ng
    ng1 = R.SHAPES[("resident", 1)]
    assert (1, 4) in ng1 and any(h * w == 4 * R.RESIDENT_THREADS for h, w in ng1)
    steps = [h * w // R.FUSED_STEP_PIXELS for h, w in R.SHAPES[("fused", None)]]
    assert {s % R.FUSED_WAVES for s in steps} == {0, 1, 2, 3}
    assert min(steps) == R.RESIDENT_MAX_PIXELS // R.FUSED_STEP_PIXELS + 1 and max(steps) == R.FUSED_MAX_PIXELS // R.FUSED_STEP_PIXELS


def test_oracle_accepts_every_healthy_input(target_image):
    """No ZeroDivisionError, every std non-zero: the table's batches, the eight distinct images of the persistence and chunking tests."""
    cases = [(h, w, 3) for h, w in R.ALL_SHAPES] + [(16, 16, 8), (72, 72, 8), (257, 256, 8), (3, 3, 8)]
    for h, w, n in cases:
        out, ms = R.expected(target_image, h, w, n)
        assert out.shape == (n, h, w, 3) and np.isfinite(ms).all() and (ms[:, 3:] > 0).all(), (h, w, n)
    # the inputs are what they are named for
    imgs = R.batch(96, 96)
    assert (imgs[0, :32] == 255).all() and imgs[0, 32:44].max() < 12  # noqa: PLR2004
    assert {tuple(p) for p in imgs[1].reshape(-1, 3)[-96 * 24:]} == {tuple(p) for p in R.SATURATED}
    assert len({im.tobytes() for im in R.batch(16, 16, 8)}) == 8 and len({im.tobytes() for im in R.batch(3, 3, 8)}) == 8  # noqa: PLR2004


def test_oracle_raises_on_every_degenerate_input(target_image):
    ref = R.oracle(target_image)
    for h, w in R.ZERO_STD_SHAPES:
        ramp = R.grey_ramp(h, w)
        _, std = ref.get_mean_std(ramp.copy())
        assert std[0] > 0 and std[1] == 0 and std[2] == 0, (h, w, std)
        with pytest.raises(ZeroDivisionError):
            ref.transform(ramp.copy())
    flat = R.flat_image(*R.FLAT_SHAPE)
    _, std = ref.get_mean_std(flat.copy())
    assert std[1] == 0 and std[2] == 0
    with pytest.raises(ZeroDivisionError):
        ref.transform(flat.copy())


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def norm(target_image):
    from tiatoolbox_amd.tools.stainnorm import get_normalizer

    nm = get_normalizer("reinhard")
    nm.fit(target_image)
    return nm


def _moments_rc(batch) -> int:
    """tia_lab_moments_u8 itself on the batch's pointer: 0 = a one-launch kernel took it, TIA_ESIZE = the caller's three launches."""
    import torch

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import reinhard as rh

    n, h, w, _ = batch.shape
    ms = torch.empty((n, 6), dtype=torch.float64, device=batch.device)
    rc = _lib.load().tia_lab_moments_u8(batch.data_ptr(), n, h, w, rh.lab_tables(batch.device).data_ptr(),
                                        rh._channel_values_device(batch.device).data_ptr(), ms.data_ptr(), 0,  # noqa: SLF001
                                        _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def _direct_transform(norm, batch, *, want_meanstd: bool = False):
    """tia_reinhard_transform_u8 itself (for a shape it returns TIA_ESIZE for: the three launches, called one by one), with what
    ``ReinhardNormalizer.transform`` never passes or shows: ``d_meanstd``, the flags, an output between two runs of canary bytes and a
    workspace of exactly the size the library asks for (with slack behind it that it must not need).  n <= 65535."""
    import torch

    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools import reinhard as rh

    lib = _lib.load()
    n, h, w, _ = batch.shape
    dev, nbytes = batch.device, batch.numel()
    held = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    out = held[GUARD:GUARD + nbytes].view(n, h, w, 3)
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    ms = torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev) if want_meanstd else None
    ms_ptr = ms.data_ptr() if ms is not None else 0
    ws_bytes = int(lib.tia_reinhard_workspace_bytes(n, h, w))
    ws = torch.empty(ws_bytes + GUARD, dtype=torch.uint8, device=dev) if ws_bytes else None
    tabs, chan = rh.lab_tables(dev).data_ptr(), rh._channel_values_device(dev).data_ptr()  # noqa: SLF001
    tm, ts = (C.c_double * 3)(*norm.target_means), (C.c_double * 3)(*norm.target_stds)
    stream = _lib.current_stream()
    rc = lib.tia_reinhard_transform_u8(batch.data_ptr(), n, h, w, tabs, chan, tm, ts, out.data_ptr(), ms_ptr, flags.data_ptr(),
                                       ws.data_ptr() if ws is not None else 0, ws_bytes, stream)
    if rc == _lib.TIA_ESIZE:
        hist = torch.zeros((n, 3, 256), dtype=torch.int32, device=dev)
        luts = torch.empty((n, 3, 256), dtype=torch.uint8, device=dev)
        _lib.check(lib.tia_lab_hist_u8(batch.data_ptr(), n, h, w, tabs, hist.data_ptr(), stream), "tia_lab_hist_u8")
        _lib.check(lib.tia_reinhard_luts(hist.data_ptr(), n, chan, tm, ts, luts.data_ptr(), ms_ptr, flags.data_ptr(), stream),
                   "tia_reinhard_luts")
        _lib.check(lib.tia_reinhard_apply_u8(batch.data_ptr(), n, h, w, tabs, luts.data_ptr(), out.data_ptr(), stream),
                   "tia_reinhard_apply_u8")
    else:
        _lib.check(rc, "tia_reinhard_transform_u8")
    torch.cuda.synchronize()
    assert bool((held[:GUARD] == CANARY).all()) and bool((held[GUARD + nbytes:] == CANARY).all()), "bytes written outside d_out"
    return rc, out, flags.cpu().numpy(), ms


def _assert_stats(ms: np.ndarray, exp_ms: np.ndarray) -> None:
    np.testing.assert_allclose(ms, exp_ms, rtol=0, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=_id)
def test_every_route_matches_oracle(shape, norm, target_image):
    """transform bit for bit; lab_statistics within 1e-9 of the oracle and EQUAL to get_mean_std (two different kernels: the
    one-launch moments, the many-workgroup histogram + host arithmetic); the route is the one ``R.route`` predicts."""
    import torch

    from tiatoolbox_amd import _lib

    h, w = shape
    imgs = R.batch(h, w)
    exp_out, exp_ms = R.expected(target_image, h, w)
    dev = torch.from_numpy(imgs).cuda()
    kind, _ = R.route(h, w)
    one_launch = kind in ("resident", "fused")
    assert (int(_lib.load().tia_reinhard_workspace_bytes(len(imgs), h, w)) > 0) == (kind == "fused")
    assert _moments_rc(dev) == (0 if one_launch else _lib.TIA_ESIZE)
    got = norm.transform(dev).cpu().numpy()
    for i in range(len(imgs)):
        assert np.array_equal(got[i], exp_out[i]), (shape, i, int((got[i] != exp_out[i]).sum()))
    ms = norm.lab_statistics(dev).cpu().numpy()
    _assert_stats(ms, exp_ms)
    for i in range(len(imgs)):
        mean, std = norm.get_mean_std(imgs[i])
        assert np.array_equal(ms[i], np.concatenate([mean, std])), (shape, i)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(256, 256), (320, 320)], ids=_id)
def test_direct_call_writes_meanstd_and_nothing_outside_out(shape, norm, target_image):
    """tia_reinhard_transform_u8 with ``d_meanstd`` (Python passes 0): the same six doubles as lab_statistics, the same image, no
    flag, the canaries around ``d_out`` intact (a wave step too many in pass 2 would land there)."""
    import torch

    h, w = shape
    dev = torch.from_numpy(R.batch(h, w)).cuda()
    exp_out, exp_ms = R.expected(target_image, h, w)
    rc, out, flags, ms = _direct_transform(norm, dev, want_meanstd=True)
    assert rc == 0 and not flags.any()
    assert np.array_equal(out.cpu().numpy(), exp_out)
    assert torch.equal(ms, norm.lab_statistics(dev))
    _assert_stats(ms.cpu().numpy(), exp_ms)


def _persistent(norm, target_image, h: int, w: int, n: int) -> None:
    """n patches drawn in seeded random order from 8 distinct images: consecutive patches of one workgroup differ, so a stale
    histogram, stale tables or a clear that comes too early shows."""
    import torch

    exp_out, exp_ms = R.expected(target_image, h, w, 8)
    idx = torch.from_numpy(np.random.default_rng(n).integers(0, 8, n)).cuda()
    assert len(torch.unique(idx)) == 8  # noqa: PLR2004
    distinct = torch.from_numpy(R.batch(h, w, 8)).cuda()
    batch = distinct[idx]
    assert torch.equal(norm.transform(batch), torch.tensor(exp_out).cuda()[idx])
    ms = norm.lab_statistics(batch)
    assert float((ms - torch.tensor(exp_ms).cuda()[idx]).abs().max()) <= 1e-9  # noqa: PLR2004
    assert torch.equal(ms, norm.lab_statistics(distinct)[idx])   # each patch's statistics as if it were its workgroup's first


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 16), (72, 72)], ids=_id)
def test_resident_workgroups_take_several_patches(shape, norm, target_image):
    """One workgroup per CU: 2 CUs + 5 patches give every workgroup two or three."""
    import torch

    assert R.route(*shape)[0] == "resident"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _persistent(norm, target_image, *shape, 2 * cus + 5)


@pytest.mark.gpu
def test_fused_workgroups_take_several_patches(norm, target_image):
    """The grid is the library's own answer (CUs x resident workgroups); half of the workgroups take a second patch."""
    from tiatoolbox_amd import _lib

    h, w = 257, 256
    assert R.route(h, w) == ("fused", None)
    grid = int(_lib.load().tia_reinhard_workspace_bytes(10**6, h, w)) // (h * w * 4)
    n = grid + grid // 2 + 1
    assert grid >= 1 and n <= 4096, (grid, n)  # noqa: PLR2004 -- a larger grid: rethink this test, do not shrink it
    _persistent(norm, target_image, h, w, n)


def _assert_flags_middle(norm, imgs: np.ndarray, exp_out: np.ndarray) -> None:
    import torch

    dev = torch.from_numpy(imgs).cuda()
    with pytest.raises(ZeroDivisionError):
        norm.transform(dev)
    _, out, flags, _ = _direct_transform(norm, dev)
    assert flags.tolist() == [0, 1, 0]
    got = out.cpu().numpy()
    assert np.array_equal(got[0], exp_out[0]) and np.array_equal(got[2], exp_out[2])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.ZERO_STD_SHAPES, ids=_id)
def test_zero_std_is_flagged_on_every_route(shape, norm, target_image):
    """A grey ramp (a == b == 128: only the integer a / b sums can raise the flag) in the middle of a batch: transform raises, the flag
    lands on that image alone, its neighbours are untouched by it."""
    h, w = shape
    _assert_flags_middle(norm, R.zero_std_batch(h, w, R.grey_ramp(h, w)), R.expected(target_image, h, w)[0])


@pytest.mark.gpu
def test_flat_image_is_flagged_on_the_fused_route(norm, target_image):
    h, w = R.FLAT_SHAPE
    _assert_flags_middle(norm, R.zero_std_batch(h, w, R.flat_image(h, w)), R.expected(target_image, h, w)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [4, 1])
@pytest.mark.parametrize("shape", [(256, 256), (320, 320), (257, 1024)], ids=_id)
def test_misaligned_bases(shape, offset, norm, target_image):
    """A batch that starts 4 bytes (the one-launch kernels still take it: they need dword alignment; the 16-byte streaming path does
    not) or 1 byte (nothing but the scalar three-launch form does) into its allocation."""
    import torch

    from tiatoolbox_amd import _lib

    h, w = shape
    imgs = R.batch(h, w)
    exp_out, exp_ms = R.expected(target_image, h, w)
    buf = torch.zeros(imgs.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + imgs.size].view(imgs.shape)
    view.copy_(torch.from_numpy(imgs))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + offset
    kind, _ = R.route(h, w, align=offset)
    assert kind == ("three_scalar" if offset == 1 or shape == (257, 1024) else R.route(h, w)[0])
    assert _moments_rc(view) == (0 if kind in ("resident", "fused") else _lib.TIA_ESIZE)
    assert np.array_equal(norm.transform(view).cpu().numpy(), exp_out)
    _assert_stats(norm.lab_statistics(view).cpu().numpy(), exp_ms)


@pytest.mark.gpu
def test_batches_beyond_the_launch_limit_are_chunked(norm, target_image):
    """65535 + 7 images of 3 x 3: the 65535-image loops of transform, lab_statistics and _lab_hist go round twice."""
    import torch

    exp_out, exp_ms = R.expected(target_image, 3, 3, 8)
    imgs8 = R.batch(3, 3, 8)
    idx_h = np.random.default_rng(NCHUNK).integers(0, 8, NCHUNK)
    idx = torch.from_numpy(idx_h).cuda()
    batch = torch.from_numpy(imgs8).cuda()[idx]
    assert torch.equal(norm.transform(batch), torch.tensor(exp_out).cuda()[idx])
    ms = norm.lab_statistics(batch)
    assert float((ms - torch.tensor(exp_ms).cuda()[idx]).abs().max()) <= 1e-9  # noqa: PLR2004
    assert np.array_equal(norm._lab_hist(batch), R.lab_hist(imgs8)[idx_h])  # noqa: SLF001

"""The canvas stitching kernels (``block_flags_kernel``, ``row_merge_kernel``, ``finalize_kernel`` of ``csrc/canvas.hip``) and the
two engines that drive them, against the NumPy statement in ``_canvas_ref`` on the case lists ``test_canvas_stitch.py`` checks on
the host: sums, counts, probabilities and labels element for element (a NaN equal to a NaN), no tolerance anywhere."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import semantic as osem

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _canvas_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PRED_FILL, PROB_FILL = 0xA5, -7.5  # sentinels: what a kernel must leave alone
TIA_OK = 0  # include/tiatoolbox_amd.h


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def differing(a, b) -> int:
    a, b = np.asarray(a), np.asarray(b)
    return int((~((a == b) | ((a != a) & (b != b)))).sum())


def _ss():
    from tiatoolbox_amd.models.engine import semantic_segmentor as ss

    return ss


def _dev_row_merge(blocks, xs, width):
    row, cnt = _ss()._row_merge(torch.from_numpy(np.ascontiguousarray(blocks)).cuda(), np.asarray(xs), width)  # noqa: SLF001
    return row.cpu().numpy(), cnt.cpu().numpy()


def _check_row_merge(blocks, xs, width):
    row, cnt = _dev_row_merge(blocks, xs, width)
    exp_row, exp_cnt = ref.row_merge_ref(blocks, xs, width)
    assert same(cnt, exp_cnt), differing(cnt, exp_cnt)
    assert same(row, exp_row), differing(row, exp_row)
    return exp_row, exp_cnt


# ------------------------------------------------------------------------------------------------ row merge
@pytest.mark.parametrize("name", list(ref.channel_cases()))
def test_row_merge_channel_sweep(name):
    _check_row_merge(*ref.channel_cases()[name])


def test_row_merge_deep_and_unordered():
    """Six shuffled blocks, four deep: the kernel adds in the order given, and so does the public wrapper."""
    blocks, xs, width = ref.deep_case()
    exp_row, exp_cnt = _check_row_merge(blocks, xs, width)
    locs = ref.row_locs(xs, 4, 16)
    canvas, count = _ss().merge_batch_to_canvas(blocks, locs, (4, width, 3))
    ora_canvas, ora_count = osem.merge_batch_to_canvas(blocks, locs, (4, width, 3))
    assert same(canvas, ora_canvas), differing(canvas, ora_canvas)
    assert same(count, ora_count) and same(canvas, exp_row) and same(count[..., 0], exp_cnt)


@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("kind", ref.ZERO_KINDS)
def test_row_merge_zero_block_rule(kind, c):
    """``np.any(block)`` false means skip, for sum and count alike: ``+0.0`` and ``-0.0`` blocks are skipped, a block whose only
    non-zero is ``2^-149`` or a NaN counts."""
    blocks, xs, width = ref.zero_case(kind, c)
    _, exp_cnt = _check_row_merge(blocks, xs, width)
    assert exp_cnt[0, 2] == (4 if kind in ("plus_zero", "minus_zero") else 5)


@pytest.mark.parametrize(("n", "wrapped"), [(300, 44), (256, 0)])
def test_row_merge_count_wraps_like_uint8(n, wrapped):
    _, exp_cnt = _check_row_merge(*ref.wrap_case(n))
    assert (exp_cnt[:, :3] == wrapped).all()


def test_row_merge_grid_stride_loop():
    """2 x 2,100,000 canvas elements: more than the 16384 workgroups of 256 threads the launcher caps the grid at."""
    blocks, xs, width = ref.grid_stride_case()
    assert blocks.shape[1] * width > 16384 * 256
    row, cnt = _ss()._row_merge(torch.from_numpy(blocks).cuda(), xs, width)  # noqa: SLF001
    exp_row, exp_cnt = ref.row_merge_ref(blocks, xs, width)
    assert torch.equal(row.cpu(), torch.from_numpy(exp_row)) and torch.equal(cnt.cpu(), torch.from_numpy(exp_cnt))
    assert exp_cnt[:, -30:].all() and exp_cnt.sum() == 2 * (64 + 64 + 30)


# ------------------------------------------------------------------------------------------------ finalize
def _dev_finalize(case, *, with_probs: bool = True, y_base: int = 0, rows: int | None = None):
    """``_finalize`` of one case into sentinel-filled maps of ``rows`` rows whose row 0 is canvas row ``y_base``."""
    row_a, cnt_a, ys_a, row_b, cnt_b, ys_b, _, y0, y1 = ref.finalize_args(case)
    width, c = row_a.shape[1:]
    rows = max(y1, ys_a, ys_b) - y_base + 2 if rows is None else rows
    pred = torch.full((rows, width), PRED_FILL, dtype=torch.uint8, device="cuda")
    probs = torch.full((rows, width, c), PROB_FILL, dtype=torch.float32, device="cuda") if with_probs else None
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    _ss()._finalize(up(row_a), up(cnt_a), ys_a, up(row_b), up(cnt_b), ys_b, y0, y1, probs, pred, y_base=y_base)  # noqa: SLF001
    torch.cuda.synchronize()
    return (probs.cpu().numpy() if with_probs else None), pred.cpu().numpy()


def _check_finalize(case):
    y0, y1 = case["y0"], case["y1"]
    exp_probs, exp_pred = ref.finalize_ref(*ref.finalize_args(case))
    probs, pred = _dev_finalize(case)
    assert same(probs[y0:y1], exp_probs), (case["name"], differing(probs[y0:y1], exp_probs))
    assert same(pred[y0:y1], exp_pred), (case["name"], differing(pred[y0:y1], exp_pred))
    outside = np.ones(len(pred), dtype=bool)
    outside[y0:y1] = False
    assert (pred[outside] == PRED_FILL).all() and (probs[outside] == PROB_FILL).all(), case["name"]
    _, pred_only = _dev_finalize(case, with_probs=False)  # probs == NULL: the same labels
    assert same(pred_only, pred), case["name"]
    return exp_probs, exp_pred


@pytest.mark.parametrize("c", range(1, 9))
def test_finalize_geometry(c):
    """Overlaps of 5, 3 and 1 rows, none, a gap; the engine's ranges, a sub-range, the span of both rows, a range that ends
    where ``b`` begins, no ``b``; with and without ``probs``."""
    for case in ref.finalize_geometry_cases(c):
        _check_finalize(case)


@pytest.mark.parametrize("case", ref.finalize_count_cases(), ids=lambda case: case["name"])
def test_finalize_counts_wrap_like_uint8(case):
    exp_probs, _ = _check_finalize(case)
    count = case["cnt_a"] + case["cnt_b"]
    assert same(exp_probs, (case["row_a"] + case["row_b"]) / np.float32(44 if case["name"] == "count_wrap44" else 1))
    assert count.dtype == np.uint8 and (count == (44 if case["name"] == "count_wrap44" else 0)).all()


@pytest.mark.parametrize("case", ref.finalize_label_cases(), ids=lambda case: case["name"])
def test_finalize_labels_are_numpy_argmax(case):
    """Exact ties, signed zeros, all-negative channels, infinities and NaNs: the first NaN wins, else the first maximum."""
    exp_probs, exp_pred = _check_finalize(case)
    assert same(exp_pred, np.argmax(exp_probs, -1).astype(np.uint8)) and (exp_pred != ref.gt_scan_argmax(exp_probs)).any()


def test_finalize_y_base_shifts_the_rows_and_touches_nothing_else():
    case = next(k for k in ref.finalize_geometry_cases(3) if k["name"] == "c3_off5_last")
    y0, y1 = case["y0"], case["y1"]
    assert y0 - 7 == 2
    probs, pred = _dev_finalize(case)
    band_probs, band_pred = _dev_finalize(case, y_base=7, rows=y1 - 7 + 1)
    assert same(band_probs[y0 - 7:y1 - 7], probs[y0:y1]) and same(band_pred[y0 - 7:y1 - 7], pred[y0:y1])
    assert same(band_probs[y0 - 7:y1 - 7], ref.finalize_ref(*ref.finalize_args(case))[0])
    for rows in (slice(0, y0 - 7), slice(y1 - 7, None)):
        assert (band_pred[rows] == PRED_FILL).all() and (band_probs[rows] == PROB_FILL).all() and len(band_pred[rows]) >= 1


def test_finalize_grid_stride_loop():
    rng = np.random.default_rng(47)
    width = ref.GRID_STRIDE_WIDTH
    case = {"name": "grid_stride", "row_a": rng.standard_normal((3, width, 1)).astype(np.float32),
            "cnt_a": rng.integers(0, 4, (3, width)).astype(np.uint8), "ys_a": 0,
            "row_b": rng.standard_normal((3, width, 1)).astype(np.float32), "cnt_b": rng.integers(0, 4, (3, width)).astype(np.uint8),
            "ys_b": 2, "oh": 3, "y0": 2, "y1": 4}
    assert (case["y1"] - case["y0"]) * width > 16384 * 256
    exp_probs, exp_pred = ref.finalize_ref(*ref.finalize_args(case))
    probs, pred = _dev_finalize(case)
    assert torch.equal(torch.from_numpy(probs[2:4]), torch.from_numpy(exp_probs)) and not pred[2:4].any() and not exp_pred.any()
    assert (pred[[0, 1, 4, 5]] == PRED_FILL).all() and (probs[[0, 1, 4, 5]] == PROB_FILL).all()


# ------------------------------------------------------------------------------------------------ refusals
def _filled(shape, dtype, value):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def test_row_merge_refuses_bad_arguments_and_writes_nothing():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    n, oh, ow, c, width = 3, 2, 4, 2, 9
    blocks = torch.ones((n, oh, ow, c), dtype=torch.float32, device="cuda")
    xs = torch.tensor([0, 2, 5], dtype=torch.int32, device="cuda")
    row, cnt, flags = _filled((oh, width, c), torch.float32, PROB_FILL), _filled((oh, width), torch.uint8, PRED_FILL), _filled((n,), torch.int32, -3)

    def call(**kw):
        a = {"blocks": blocks.data_ptr(), "xs": xs.data_ptr(), "n": n, "oh": oh, "ow": ow, "c": c, "width": width, "row": row.data_ptr(),
             "cnt": cnt.data_ptr(), "flags": flags.data_ptr(), **kw}
        rc = lib.tia_canvas_row_merge_f32(a["blocks"], a["xs"], a["n"], a["oh"], a["ow"], a["c"], a["width"], a["row"], a["cnt"], a["flags"],
                                          _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    bad = [{"blocks": 0}, {"xs": 0}, {"row": 0}, {"cnt": 0}, {"flags": 0}, {"n": 0}, {"n": -1}, {"n": 65536}, {"c": 0}, {"c": 9}, {"oh": 0},
           {"ow": 0}, {"width": 0}]
    for kw in bad:
        assert call(**kw) == _lib.TIA_EINVAL, kw
        assert (row == PROB_FILL).all() and (cnt == PRED_FILL).all() and (flags == -3).all(), kw
    assert call() == TIA_OK and same(cnt.cpu().numpy(), ref.row_merge_ref(blocks.cpu().numpy(), [0, 2, 5], width)[1])
    # n = 65535 is the largest accepted count.  Only the argument check is exercised: the blocks are single float32 ones (256 KB in
    # all, every buffer sized for them), not blocks of a real patch size -- 65535 of those would be gigabytes for nothing.
    many = torch.ones((65535, 1, 1, 1), dtype=torch.float32, device="cuda")
    xs_many = torch.zeros(65535, dtype=torch.int32, device="cuda")
    row1, cnt1, flags1 = _filled((1, 1, 1), torch.float32, PROB_FILL), _filled((1, 1), torch.uint8, PRED_FILL), _filled((65535,), torch.int32, -3)
    rc = lib.tia_canvas_row_merge_f32(many.data_ptr(), xs_many.data_ptr(), 65535, 1, 1, 1, 1, row1.data_ptr(), cnt1.data_ptr(),
                                      flags1.data_ptr(), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == TIA_OK and float(row1) == 65535.0 and int(cnt1) == 65535 % 256


def test_finalize_refuses_bad_arguments_and_writes_nothing():
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    oh, width, c = 3, 5, 2
    row_a = torch.ones((oh, width, c), dtype=torch.float32, device="cuda")
    cnt_a = torch.ones((oh, width), dtype=torch.uint8, device="cuda")
    row_b, cnt_b = row_a.clone(), cnt_a.clone()
    probs, pred = _filled((oh, width, c), torch.float32, PROB_FILL), _filled((oh, width), torch.uint8, PRED_FILL)

    def call(**kw):
        a = {"row_a": row_a.data_ptr(), "cnt_a": cnt_a.data_ptr(), "row_b": row_b.data_ptr(), "cnt_b": cnt_b.data_ptr(), "c": c, "y0": 0,
             "y1": oh, "pred": pred.data_ptr(), **kw}
        rc = lib.tia_canvas_finalize_f32(a["row_a"], a["cnt_a"], 0, a["row_b"], a["cnt_b"], 0, oh, width, a["c"], a["y0"], a["y1"],
                                         probs.data_ptr(), a["pred"], _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    for kw in ({"row_a": 0}, {"cnt_a": 0}, {"pred": 0}, {"cnt_b": 0}, {"c": 0}, {"c": 256}, {"y0": 2, "y1": 1}):
        assert call(**kw) == _lib.TIA_EINVAL, kw
        assert (probs == PROB_FILL).all() and (pred == PRED_FILL).all(), kw
    assert call(y0=2, y1=2) == TIA_OK  # an empty range: accepted, nothing written
    assert (probs == PROB_FILL).all() and (pred == PRED_FILL).all()
    assert call() == TIA_OK and (probs == 1.0).all() and (pred == 0).all()


# ------------------------------------------------------------------------------------------------ engines
def _stub_values(patch_u8, xp, pin: int, pout: int, nch: int):
    """Deterministic head output ``[n, pin, pin, 3]`` uint8 -> ``[n, pout, pout, nch]`` float32 in [0, 1): 24-bit fractions built
    from the centre crop's bytes and the position inside the patch (integer arithmetic, one exact int -> float conversion, one
    exact scaling: identical in torch and NumPy), so overlapping patches disagree and their float32 sums round."""
    off = (pin - pout) // 2
    if xp is torch:
        t = patch_u8[:, off:off + pout, off:off + pout, :].to(torch.int32)
        yy = torch.arange(pout, device=t.device, dtype=torch.int32).view(1, pout, 1)
        xx = torch.arange(pout, device=t.device, dtype=torch.int32).view(1, 1, pout)
    else:
        t = patch_u8[:, off:off + pout, off:off + pout, :].astype(np.int32)
        yy = np.arange(pout, dtype=np.int32).reshape(1, pout, 1)
        xx = np.arange(pout, dtype=np.int32).reshape(1, 1, pout)
    chans = []
    for c in range(nch):
        b0 = (t[..., c % 3] * (c + 3) + yy * 7 + xx * 13) & 255
        b1 = (t[..., (c + 1) % 3] * 5 + xx * 3 + c) & 255
        b2 = (t[..., (c + 2) % 3] + yy) & 255
        word = b0 * 65536 + b1 * 256 + b2
        chans.append(word.to(torch.float32) * (2.0 ** -24) if xp is torch else word.astype(np.float32) * np.float32(2.0 ** -24))
    return torch.stack(chans, dim=-1) if xp is torch else np.stack(chans, axis=-1)


PIN, POUT, NCH = 32, 16, 5


class _StubHead(torch.nn.Module):
    """Stands in for the UNet (the ``infer_batch`` contract of ``architecture/unet.py``) and counts its calls."""

    calls = 0

    def __init__(self) -> None:
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    preproc_func = staticmethod(lambda img: img)
    postproc_func = staticmethod(lambda img: img)

    @staticmethod
    def infer_batch(model, batch_data, *, device):  # noqa: ARG004
        _StubHead.calls += 1
        return _stub_values(batch_data, torch, PIN, POUT, NCH)


def _stub_hovernet(pin: int, pout: int):
    """The deterministic-head HoVer-Net of ``test_tile_mode.py`` at any patch size: np = darkness of the centre crop, hv = signed
    patch-local ramps modulated by it, tp = 1 + (darkness > 0.8).  Counts its calls."""
    from tiatoolbox_amd.models.architecture.hovernet import HoVerNet

    off = (pin - pout) // 2

    class _Stub(HoVerNet):
        calls = 0

        @staticmethod
        def infer_batch(model, batch_data, *, device):  # noqa: ARG004
            _Stub.calls += 1
            x = torch.as_tensor(batch_data).to(device).float()
            dark = (1.0 - x.mean(-1) / 255.0)[:, off:off + pout, off:off + pout]
            ramp = torch.linspace(-1, 1, pout, device=dark.device)
            hv = torch.stack([ramp[None, None, :] * dark, ramp[None, :, None] * dark], dim=-1)
            return dark[..., None].contiguous(), hv.contiguous(), (1.0 + (dark > 0.8).float())[..., None].contiguous()

    return _Stub(num_types=6, mode="fast")


class _Mask:
    def __init__(self, img) -> None:
        self.img = img


def _semantic_engine(stride, batch_size: int = 3):
    from tiatoolbox_amd.models.engine.io_config import IOSegmentorConfig
    from tiatoolbox_amd.models.engine.semantic_segmentor import SemanticSegmentor

    res = {"units": "mpp", "resolution": 0.25}
    cfg = IOSegmentorConfig(input_resolutions=[res], output_resolutions=[res], patch_input_shape=[PIN, PIN],
                            patch_output_shape=[POUT, POUT], stride_shape=list(stride), save_resolution=res)
    eng = SemanticSegmentor(_StubHead(), batch_size=batch_size, device="cuda", verbose=False)
    eng._ioconfig = eng.ioconfig = cfg  # noqa: SLF001
    return eng


def _multitask_engine(stride, pin: int, pout: int, batch_size: int = 4):
    from tiatoolbox_amd.models.engine.io_config import IOInstanceSegmentorConfig
    from tiatoolbox_amd.models.engine.multi_task_segmentor import MultiTaskSegmentor

    res = {"units": "mpp", "resolution": 0.25}
    cfg = IOInstanceSegmentorConfig(input_resolutions=[res], output_resolutions=[res, res, res], patch_input_shape=[pin, pin],
                                    patch_output_shape=[pout, pout], stride_shape=list(stride), margin=4, tile_shape=[4 * pout, 4 * pout])
    eng = MultiTaskSegmentor(_stub_hovernet(pin, pout), batch_size=batch_size, device="cuda", verbose=False)
    eng._ioconfig = eng.ioconfig = cfg  # noqa: SLF001
    return eng


def _slide(h: int, w: int, seed: int):
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    return ArrayWSIReader(np.random.default_rng(seed).integers(20, 200, (h, w, 3), dtype=np.uint8), mpp=0.25, power=40.0)


def test_semantic_segmentor_wsi_maps_equal_the_statement():
    """96 x 70 slide, 32 in / 16 out, rows two deep and columns four deep, batches of 3 that straddle the patch rows, a mask that
    drops the whole first patch row, a middle row and patches inside rows: the whole maps, resident and streamed."""
    h, w = 70, 96
    reader = _slide(h, w, 48)
    mask = np.ones((h, w), dtype=np.uint8)
    mask[:16] = 0       # the first patch row (canvas rows 0 .. 15) sees no tissue; the second (8 .. 23) does
    mask[32:48] = 0     # the patch row at y = 32
    mask[:28, 30:47] = 0     # the patch at x = 30 of the row at y = 8
    mask[50:70, 60:80] = 0   # the patch at x = 60 of the rows at y = 56 and y = 64
    eng = _semantic_engine([8, 5])
    out = eng.infer_wsi(reader, _Mask(mask), return_probabilities=True)
    in_b, out_b, keep = eng.get_coordinates(reader, _Mask(mask))
    row_ys = np.unique(out_b[:, 1])
    per_row = np.array([(keep & (out_b[:, 1] == y)).sum() for y in row_ys])
    assert list(np.diff(row_ys)) == [8] * (len(row_ys) - 1) and per_row[0] == 0 and per_row[4] == 0 and 0 < per_row[1] < (out_b[:, 1] == 8).sum()
    assert keep.sum() % 3 != 0 and (per_row[per_row > 0] % 3 != 0).any()
    blocks = _stub_values(reader.read_bounds_batch(in_b).cpu().numpy(), np, PIN, POUT, NCH)
    blocks[~keep] = 0.0  # patches the mask dropped are never inferred: all-zero blocks are skipped
    exp_probs, exp_pred = ref.stitch_ref(blocks, out_b, (h, w))
    assert ref.wide_ref(blocks, out_b, (h, w))[3].max() == 8
    probs, pred = out["probabilities"].cpu().numpy(), out["predictions"].cpu().numpy()
    assert same(probs, exp_probs), differing(probs, exp_probs)
    assert same(pred, exp_pred), differing(pred, exp_pred)
    eng.device_band_rows = 2
    streamed = eng.infer_wsi(reader, _Mask(mask), return_probabilities=True)
    assert eng.last_band_streamed and not streamed["probabilities"].is_cuda
    assert same(streamed["probabilities"].numpy(), exp_probs) and same(streamed["predictions"].numpy(), exp_pred)


def test_multi_task_segmentor_wsi_maps_equal_the_statement():
    """HoVer-Net's three heads (np, signed hv, tp) at a stride with four-deep column overlap under a mask that moves the region's
    origin: every stitched head map equals the statement on that head's blocks."""
    from tiatoolbox_amd.models.engine.multi_task_segmentor import get_full_output_locs_inside_mask
    from tiatoolbox_amd.tools.patchextraction import PatchExtractor

    h, w, pin, pout = 130, 170, 48, 32
    reader = _slide(h, w, 49)
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[70:125, 90:165] = 1   # tissue far enough from the top-left corner that the region's origin moves
    mask[70:125, 110:150] = 0  # a hole wide enough to drop patches inside the region
    eng = _multitask_engine([16, 8], pin, pout)
    out = eng.infer_wsi(reader, _Mask(mask))
    in_b, out_b = PatchExtractor.get_coordinates(patch_output_shape=(pout, pout), image_shape=(w, h), patch_input_shape=(pin, pin),
                                                 stride_shape=(8, 16))
    keep = PatchExtractor.filter_coordinates(_Mask(mask), out_b, (w, h), min_mask_ratio=0)
    kept = out_b[keep]
    bounds = (kept[:, 0].min(), kept[:, 1].min(), kept[:, 2].max(), kept[:, 3].max())
    inside, padding, (rh, rw) = get_full_output_locs_inside_mask(out_b, bounds, (h, w))
    meets = ~((out_b[:, 2] < bounds[0]) | (out_b[:, 0] > bounds[2]) | (out_b[:, 3] < bounds[1]) | (out_b[:, 1] > bounds[3]))
    assert padding[0] > 0 and padding[1] > 0 and 0 < keep[meets].sum() < meets.sum() and np.array_equal(out["coordinates"], kept)
    heads = eng.model.infer_batch(eng.model, reader.read_bounds_batch(in_b[meets]), device="cuda")
    assert len(out["probabilities"]) == 3
    for j, got in enumerate(out["probabilities"]):
        blocks = heads[j].float().cpu().numpy()
        blocks[~keep[meets]] = 0.0
        exp, _ = ref.stitch_ref(blocks, inside, (rh, rw))
        assert got.shape == exp.shape == (rh, rw, (1, 2, 1)[j])
        assert same(got.cpu().numpy(), exp), (j, differing(got.cpu().numpy(), exp))
        if j == 1:
            assert (exp < 0).any() and (exp > 0).any() and ref.wide_ref(blocks, inside, (rh, rw))[3].max() == 8


@pytest.mark.parametrize("engine", ["semantic", "multitask"])
def test_engines_refuse_three_patch_rows_over_a_canvas_row(engine):
    """Output 16 at a vertical stride of 5 or 7: a ``ValueError`` that names both settings, before anything is inferred; 8 and 16 run."""
    reader = _slide(40, 36, 50)
    for stride in (5, 7, 8, 16):
        eng = _semantic_engine([stride, 8]) if engine == "semantic" else _multitask_engine([stride, 8], PIN, POUT)
        stub = type(eng.model)
        stub.calls = 0
        if stride < 8:
            with pytest.raises(ValueError, match=r"`patch_output_shape`.*`stride_shape`"):
                eng.infer_wsi(reader, None)
            assert stub.calls == 0
        else:
            out = eng.infer_wsi(reader, None)
            assert stub.calls > 0 and (out["predictions"].shape == (40, 36) if engine == "semantic" else len(out["probabilities"]) == 3)

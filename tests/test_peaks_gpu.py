"""``utils.peaks.peak_local_max`` on the device (``csrc/peaks.hip``) against the NumPy statement (``utils/_peaks.py``):
``np.array_equal`` on every case of ``_peaks_ref.device_cases`` -- planes smaller than the window, sides around the kernel's tile
(read out of the source), batches, every ``min_distance`` route, corners and edges, ``exclude_border``, thresholds equal to a peak,
signed zeros and infinities, constant and two-valued planes, ``num_peaks``, plateaus -- then the refusals.  No tolerance anywhere."""

from __future__ import annotations

import functools
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _peaks_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SOURCE = Path(__file__).resolve().parent.parent / "tiatoolbox_amd" / "csrc" / "peaks.hip"
TILE = int(re.findall(r"constexpr int PEAK_TILE = (\d+);", SOURCE.read_text())[0])
CASES = ref.device_cases(TILE)
OK, EINVAL, ESIZE = 0, -1, -3


def _statement():
    from tiatoolbox_amd.utils import _peaks

    return _peaks


def _peaks():
    from tiatoolbox_amd.utils import peaks

    return peaks


@functools.lru_cache(maxsize=None)
def _expected(name: str):
    planes, kw = CASES[name]
    batch = planes if planes.ndim == 3 else planes[None]  # noqa: PLR2004
    out = [_statement().peak_local_max_ref(p, **kw) for p in batch]
    for o in out:
        o.setflags(write=False)
    return out


def test_cases_cover_what_they_claim():
    assert TILE >= 8 and {f"side_{s}" for s in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)} <= set(CASES)  # noqa: PLR2004
    st = _statement()
    img, kw = CASES["quantised_257x300"]
    cand = st.candidates_ref(img, kw["min_distance"])
    contested = st.contested_ref(cand, kw["min_distance"], img.shape)
    assert contested.sum() > len(cand) / 2 and len(cand) > 2000  # noqa: PLR2004  (the contested path is really exercised)
    img, kw = CASES["row_of_300_d3"]
    assert len(_expected("row_of_300_d3")[0]) == 100 and len(st.candidates_ref(img, 3)) == 300  # noqa: PLR2004
    for name in ("saturated_discs", "checkerboard_d2", "d64_quantised", "two_valued", "zeros_and_infinities_d2"):
        img, kw = CASES[name]
        cand = st.candidates_ref(img, kw["min_distance"])
        assert st.contested_ref(cand, kw["min_distance"], img.shape).any(), name
    assert not st.contested_ref(st.candidates_ref(CASES["d7_random"][0], 7), 7, (70, 90)).any()
    # strict thresholds: the peak whose value equals the threshold is gone, its neighbours in value stay
    spikes = CASES["threshold_abs_at_a_peak"][0]
    got = _expected("threshold_abs_at_a_peak")[0]
    values = spikes[got[:, 0], got[:, 1]]
    assert 5.0 not in values and 6.0 in values and 5.0 in spikes  # noqa: PLR2004
    values = spikes[tuple(_expected("threshold_rel_at_a_peak")[0].T)]
    assert 9.0 not in values and 10.0 in values  # noqa: PLR2004
    assert len(_expected("border_30")[0]) == 0 and len(_expected("border_0")[0]) > len(_expected("border_1")[0]) > len(_expected("border_19")[0])
    assert any(len(e) for e in _expected("batch_of_three")[:2]) and len(_expected("batch_of_three")[2]) == 0
    corners = {tuple(c) for c in _expected("corners_edges")[0]}
    assert {(0, 0), (0, 44), (36, 0), (36, 44)} <= corners


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_statement(name):
    planes, kw = CASES[name]
    got = _peaks().peak_local_max(torch.from_numpy(np.array(planes)).cuda(), **kw)
    got = got if isinstance(got, list) else [got]
    exp = _expected(name)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.is_cuda and g.dtype == torch.int64
        assert ref.same_peaks(g.cpu().numpy(), e), (name, len(g), len(e))


@pytest.mark.parametrize("name", ["d2_quantised", "saturated_discs", "corners_edges", "batch_of_three"])
def test_num_peaks_of_one_all_and_more(name):
    planes, kw = CASES[name]
    full = _expected(name)
    dev = torch.from_numpy(np.array(planes)).cuda()
    k_all = max(len(e) for e in full)
    assert k_all > 1
    for k in (1, k_all, k_all + 5, 0):
        got = _peaks().peak_local_max(dev, num_peaks=k, **kw)
        got = got if isinstance(got, list) else [got]
        for g, e in zip(got, full):
            assert ref.same_peaks(g.cpu().numpy(), e[:k]), (name, k)
    one = _statement().peak_local_max_ref(planes if planes.ndim == 2 else planes[0], num_peaks=1, **kw)  # noqa: PLR2004
    assert ref.same_peaks(one, full[0][:1])


def test_flat_form_carries_values_and_counts():
    planes, kw = CASES["batch_of_three"]
    dev = torch.from_numpy(np.array(planes)).cuda()
    coords, values, counts = _peaks().peak_local_max_planes(dev, **kw)
    exp = _expected("batch_of_three")
    assert counts == [len(e) for e in exp] and coords.is_cuda and values.is_cuda and values.dtype == torch.float32
    assert ref.same_peaks(coords.cpu().numpy(), np.concatenate(exp))
    flat = np.concatenate([p[e[:, 0], e[:, 1]] for p, e in zip(planes, exp)])
    assert np.array_equal(values.cpu().numpy(), flat)
    # a view that is not contiguous is taken as it is
    wide = torch.from_numpy(np.array(planes)).cuda().repeat(1, 1, 2)[:, :, :planes.shape[2]]
    assert not wide.is_contiguous()
    for g, e in zip(_peaks().peak_local_max(wide, **kw), exp):
        assert ref.same_peaks(g.cpu().numpy(), e)


def test_refusals():
    peaks = _peaks()
    img = torch.from_numpy(ref.random_plane(12, 13, 0)).cuda()
    for bad in (img.double(), img.half(), img.to(torch.int32), img[0], img[None, None]):
        with pytest.raises(ValueError, match="image"):
            peaks.peak_local_max(bad)
    for d in (0, -3, 65, 2.0):
        with pytest.raises(ValueError, match="min_distance"):
            peaks.peak_local_max(img, min_distance=d)
    with pytest.raises(ValueError, match="exclude_border"):
        peaks.peak_local_max(img, exclude_border=-1)
    with pytest.raises(ValueError, match="num_peaks"):
        peaks.peak_local_max(img, num_peaks=-1)
    # the entry points themselves: min_distance 65 and 0 are TIA_ESIZE, nothing is launched on an error
    from tiatoolbox_amd import _lib

    lib = _lib.load()
    n, h, w = 1, 12, 13
    chunks = int(lib.tia_peak_chunks(h, w))
    assert chunks == 1 and lib.tia_peak_chunks(0, 5) == 0 and lib.tia_peak_chunks(1 << 16, 1 << 15) == 0
    minmax = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    flags = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
    state = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros((n, chunks), dtype=torch.int32, device="cuda")
    totals = torch.full((n,), -5, dtype=torch.int64, device="cuda")

    def scan(d, *, image=img.data_ptr(), border=0, hh=h, ww=w, nn=n):
        return lib.tia_peak_scan_f32(image, nn, hh, ww, d, 0, 0.0, 0, 0.0, border, minmax.data_ptr(), flags.data_ptr(), state.data_ptr(),
                                     offsets.data_ptr(), totals.data_ptr(), _lib.current_stream())

    assert scan(65) == ESIZE and scan(0) == ESIZE and scan(2, hh=1 << 16, ww=1 << 15) == ESIZE
    assert scan(2, image=None) == EINVAL and scan(2, border=-1) == EINVAL and scan(2, nn=0) == EINVAL and scan(2, hh=0) == EINVAL
    torch.cuda.synchronize()
    assert int(totals[0]) == -5 and int(state.min()) == 9  # noqa: PLR2004  (untouched)
    assert scan(64) == OK and scan(2) == OK
    torch.cuda.synchronize()
    exp = _statement().peak_local_max_ref(img.cpu().numpy(), 2)
    assert int(totals[0]) == len(exp)
    # write: a capacity below the total leaves the rows beyond it unwritten
    k = len(exp)
    assert k >= 2  # noqa: PLR2004
    yx = torch.full((k, 2), -7, dtype=torch.int32, device="cuda")
    value = torch.zeros(k, dtype=torch.float32, device="cuda")
    contested = torch.full((k,), 5, dtype=torch.uint8, device="cuda")
    bases = torch.zeros(n, dtype=torch.int64, device="cuda")

    def write(cap, *, st=state.data_ptr(), out=yx.data_ptr()):
        return lib.tia_peak_write_f32(img.data_ptr(), st, n, h, w, offsets.data_ptr(), bases.data_ptr(), cap, out, value.data_ptr(),
                                      contested.data_ptr(), _lib.current_stream())

    assert write(-1) == EINVAL and write(k, st=None) == EINVAL and write(k, out=None) == EINVAL and write(0, out=None) == OK
    assert write(k - 1) == OK
    torch.cuda.synchronize()
    raster = exp[np.lexsort((exp[:, 1], exp[:, 0]))]
    assert np.array_equal(yx[:k - 1].cpu().numpy(), raster[:k - 1]) and yx[k - 1].tolist() == [-7, -7] and int(contested[k - 1]) == 5  # noqa: PLR2004
    assert write(k) == OK
    torch.cuda.synchronize()
    assert np.array_equal(yx.cpu().numpy(), raster) and not contested.any()

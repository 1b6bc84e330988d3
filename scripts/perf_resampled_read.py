"""Area-resampled WSI reads on the GPU: ``tia_gather_area_patches_u8`` against the two-step form it replaces, and
``PatchPredictor`` WSI mode through ``VirtualWSIReader`` against the same slide pre-downsampled in an ``ArrayWSIReader``.

Workload: a 20,000 x 20,000 x 3 synthetic slide at 0.25 mpp (1.2 GB, above the 256 MiB Infinity Cache), read entirely as
224 x 224 patches at 0.5 mpp (45 x 45 = 2,025 patches, the right / bottom ones padded with 255).

    python scripts/perf_resampled_read.py --out DIR [--kernels-only] [--reps N] [--mpp MPP]

``--kernels-only`` runs the two read forms alone (for ``rocprofv3 --kernel-trace --stats``); without it the script also
times them with device events and runs the end-to-end comparison.  Prints one JSON line and writes it to
``DIR/perf_resampled_read.json``.  Algorithmic bytes of the fused read: ``k^2 * out`` read + ``out`` written; HBM peak 8 TB/s.

``--mpp`` sets the slide's baseline mpp (default 0.25, the run above).  At a non-integer scale ``s = 0.5 / mpp`` (0.2425:
``s = 2.0619``, 44 x 44 = 1,936 patches, baseline regions of ``Wb = 462``) the read goes through a ``fractional=True``
reader (``tia_gather_area_resize_u8``), and is compared with the integer read (``k = 2``) of the same 1,936 view patches,
the slide taken as 0.25 mpp.  Algorithmic bytes ``M * Wb * Hb * c`` read + ``M * pw * ph * c`` written.  The end-to-end part
times PatchPredictor WSI mode through the fractional reader, through the integer reader at 0.25 mpp (2,025 patches) and on
the slide pre-resampled into an ``ArrayWSIReader`` (1,936 patches), and compares them per patch.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12
SIDE, PATCH, K = 20000, 224, 2


def _event_ms(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mpp", type=float, default=0.25, help="the slide's baseline mpp (read at 0.5 mpp)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        msg = "perf_resampled_read needs a GPU"
        raise SystemExit(msg)
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools.patchextraction import PatchExtractor
    from tiatoolbox_amd.wsicore import ArrayWSIReader, VirtualWSIReader, resolution_scale

    s = resolution_scale(0.5, "mpp", mpp=args.mpp)
    if s != K:
        _write(args, _fractional(args, s))
        return
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    slide = torch.randint(0, 256, (SIDE, SIDE, 3), dtype=torch.uint8, device=dev, generator=gen)
    virt = VirtualWSIReader(slide, mpp=0.25, power=40.0)
    view = virt.at_resolution(0.5, "mpp")
    grid = PatchExtractor.get_coordinates(image_shape=view.slide_dimensions, patch_input_shape=(PATCH, PATCH),
                                          stride_shape=(PATCH, PATCH))
    m = len(grid)
    b_view = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.int32)).to(dev)
    b_base = b_view * K
    out_bytes = m * PATCH * PATCH * 3
    base_reader = ArrayWSIReader(slide, mpp=0.25, power=40.0)
    lib = _lib.load()
    mid = PATCH * K

    def fused():
        return view.read_bounds_batch(b_view, size=(PATCH, PATCH))

    def two_step():
        big = base_reader.read_bounds_batch(b_base, size=(mid, mid))  # [m, 448, 448, 3]
        out = torch.empty((m * PATCH, PATCH, 3), dtype=torch.uint8, device=dev)
        rc = lib.tia_box_downsample_u8(big.data_ptr(), m * mid, mid, 3, K, out.data_ptr(), _lib.current_stream())
        _lib.check(rc, "tia_box_downsample_u8")
        return out.view(m, PATCH, PATCH, 3)

    # same bytes except where tia_box_downsample_u8's half-to-even differs from INTER_AREA's k = 2 half-up rule
    a, b = fused(), two_step()
    differ = int((a != b).sum())
    max_diff = int((a.int() - b.int()).abs().max())
    res = {"slide": [SIDE, SIDE, 3], "patches": m, "patch": PATCH, "factor": K, "out_bytes": out_bytes,
           "fused_vs_two_step_differing_bytes": differ, "fused_vs_two_step_max_abs_diff": max_diff}
    if args.kernels_only:
        for _ in range(args.reps):
            fused()
            two_step()
        torch.cuda.synchronize()
    else:
        t_f = _event_ms(fused, args.reps)
        t_2 = _event_ms(two_step, args.reps)
        alg = (K * K + 1) * out_bytes
        res.update({
            "fused_ms": round(t_f, 4), "fused_alg_GBps": round(alg / t_f / 1e6, 1),
            "fused_frac_hbm_peak": round(alg / (t_f * 1e-3) / HBM_PEAK, 4),
            "two_step_ms": round(t_2, 4), "two_step_alg_GBps": round(alg / t_2 / 1e6, 1),
            "two_step_frac_hbm_peak_alg": round(alg / (t_2 * 1e-3) / HBM_PEAK, 4),
            # traffic the two-step form really moves: gather k^2*out read + k^2*out written, box k^2*out read + out written
            "two_step_moved_bytes": (3 * K * K + 1) * out_bytes,
        })
        # end to end: PatchPredictor WSI mode, every patch kept (mask of ones), resampled reads vs a pre-downsampled slide
        import tempfile

        from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor

        down = view.read_bounds_batch(np.array([[0, 0, SIDE // K, SIDE // K]], np.int32))[0].contiguous()
        arr = ArrayWSIReader(down, mpp=0.5, power=20.0)
        mask = np.ones((SIDE // 64, SIDE // 64), np.uint8)
        eng = PatchPredictor("resnet18-kather100k", batch_size=128, device="cuda")
        times: dict[str, list[float]] = {"virtual": [], "array": []}
        outs = {}
        with tempfile.TemporaryDirectory() as tmp:
            for rep in range(4):  # rep 0 warms up; the two forms alternate
                for name, reader in (("virtual", virt), ("array", arr)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    path = eng.run([reader], masks=[mask], patch_mode=False, save_dir=Path(tmp) / f"{name}{rep}",
                                   return_probabilities=True)[0]
                    torch.cuda.synchronize()
                    if rep:
                        times[name].append(time.perf_counter() - t0)
                    with np.load(path) as z:
                        outs[name] = {k: z[k] for k in z.files}
        res.update({
            "e2e_patches": int(len(outs["virtual"]["coordinates"])),
            "e2e_virtual_s": [round(t, 4) for t in times["virtual"]], "e2e_array_s": [round(t, 4) for t in times["array"]],
            "e2e_virtual_median_s": round(float(np.median(times["virtual"])), 4),
            "e2e_array_median_s": round(float(np.median(times["array"])), 4),
            "e2e_same_coordinates": bool(np.array_equal(outs["virtual"]["coordinates"], outs["array"]["coordinates"])),
            "e2e_same_predictions": bool(np.array_equal(outs["virtual"]["predictions"], outs["array"]["predictions"])),
            "e2e_max_abs_prob_diff": float(np.abs(outs["virtual"]["probabilities"] - outs["array"]["probabilities"]).max()),
        })
    _write(args, res)


def _write(args, res: dict) -> None:
    line = json.dumps(res)
    print(line)
    args.out.mkdir(parents=True, exist_ok=True)
    tag = "" if args.mpp == 0.25 else f"_mpp{args.mpp:g}"  # noqa: PLR2004
    name = "perf_resampled_read_kernels" if args.kernels_only else "perf_resampled_read"
    (args.out / f"{name}{tag}.json").write_text(line + "\n")


def _fractional(args, s: float) -> dict:
    """The read at a non-integer scale ``s``: the fractional reader against the integer (k = 2) read of the same view
    patches, then PatchPredictor WSI mode end to end."""
    from tiatoolbox_amd.tools.patchextraction import PatchExtractor
    from tiatoolbox_amd.wsicore import ArrayWSIReader, VirtualWSIReader

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    slide = torch.randint(0, 256, (SIDE, SIDE, 3), dtype=torch.uint8, device=dev, generator=gen)
    frac = VirtualWSIReader(slide, mpp=args.mpp, power=40.0, fractional=True)
    view = frac.at_resolution(0.5, "mpp")
    integer = VirtualWSIReader(slide, mpp=0.25, power=40.0)
    int_view = integer.at_resolution(0.5, "mpp")
    grid = PatchExtractor.get_coordinates(image_shape=view.slide_dimensions, patch_input_shape=(PATCH, PATCH),
                                          stride_shape=(PATCH, PATCH))
    m = len(grid)
    b_view = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.int32)).to(dev)
    wb = int(np.round(PATCH * s))
    out_bytes = m * PATCH * PATCH * 3
    alg = m * wb * wb * 3 + out_bytes
    alg_int = (K * K + 1) * out_bytes

    def fractional():
        return view.read_bounds_batch(b_view, size=(PATCH, PATCH))

    def integer_read():
        return int_view.read_bounds_batch(b_view, size=(PATCH, PATCH))

    res = {"slide": [SIDE, SIDE, 3], "mpp": args.mpp, "scale": s, "patches": m, "patch": PATCH, "region": wb,
           "out_bytes": out_bytes, "alg_bytes": alg, "integer_alg_bytes": alg_int}
    if args.kernels_only:
        for _ in range(args.reps):
            fractional()
            integer_read()
        torch.cuda.synchronize()
        return res
    t_f = _event_ms(fractional, args.reps)
    t_i = _event_ms(integer_read, args.reps)
    res.update({
        "fractional_ms": round(t_f, 4), "fractional_alg_GBps": round(alg / t_f / 1e6, 1),
        "fractional_frac_hbm_peak": round(alg / (t_f * 1e-3) / HBM_PEAK, 4),
        "integer_ms": round(t_i, 4), "integer_alg_GBps": round(alg_int / t_i / 1e6, 1),
        "fractional_over_integer": round(t_f / t_i, 3),
    })
    import tempfile

    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor

    side = view.slide_dimensions[0]
    down = view.read_bounds_batch(np.array([[0, 0, side, side]], np.int32))[0].contiguous()  # the slide pre-resampled
    arr = ArrayWSIReader(down, mpp=0.5, power=40.0 / s)
    mask = np.ones((SIDE // 64, SIDE // 64), np.uint8)
    eng = PatchPredictor("resnet18-kather100k", batch_size=128, device="cuda")
    times: dict[str, list[float]] = {"fractional": [], "integer": [], "array": []}
    counts = {}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(4):  # rep 0 warms up; the three forms alternate
            for name, reader in (("fractional", frac), ("integer", integer), ("array", arr)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                path = eng.run([reader], masks=[mask], patch_mode=False, save_dir=Path(tmp) / f"{name}{rep}")[0]
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                with np.load(path) as z:
                    counts[name] = len(z["coordinates"])
    for name, ts in times.items():
        med = float(np.median(ts))
        res.update({f"e2e_{name}_patches": int(counts[name]), f"e2e_{name}_s": [round(t, 4) for t in ts],
                    f"e2e_{name}_median_s": round(med, 4), f"e2e_{name}_ms_per_patch": round(1e3 * med / counts[name], 5)})
    res["e2e_fractional_over_integer_per_patch"] = round(res["e2e_fractional_ms_per_patch"] / res["e2e_integer_ms_per_patch"], 4)
    res["e2e_fractional_over_array_per_patch"] = round(res["e2e_fractional_ms_per_patch"] / res["e2e_array_ms_per_patch"], 4)
    return res


if __name__ == "__main__":
    main()

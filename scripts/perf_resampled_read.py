"""Area-resampled WSI reads on the GPU: ``tia_gather_area_patches_u8`` against the two-step form it replaces, and
``PatchPredictor`` WSI mode through ``VirtualWSIReader`` against the same slide pre-downsampled in an ``ArrayWSIReader``.

Workload: a 20,000 x 20,000 x 3 synthetic slide at 0.25 mpp (1.2 GB, above the 256 MiB Infinity Cache), read entirely as
224 x 224 patches at 0.5 mpp (45 x 45 = 2,025 patches, the right / bottom ones padded with 255).

    python scripts/perf_resampled_read.py --out DIR [--kernels-only] [--reps N]

``--kernels-only`` runs the two read forms alone (for ``rocprofv3 --kernel-trace --stats``); without it the script also
times them with device events and runs the end-to-end comparison.  Prints one JSON line and writes it to
``DIR/perf_resampled_read.json``.  Algorithmic bytes of the fused read: ``k^2 * out`` read + ``out`` written; HBM peak 8 TB/s.
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        msg = "perf_resampled_read needs a GPU"
        raise SystemExit(msg)
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.tools.patchextraction import PatchExtractor
    from tiatoolbox_amd.wsicore import ArrayWSIReader, VirtualWSIReader

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
    line = json.dumps(res)
    print(line)
    args.out.mkdir(parents=True, exist_ok=True)
    (args.out / ("perf_resampled_read_kernels.json" if args.kernels_only else "perf_resampled_read.json")).write_text(line + "\n")


if __name__ == "__main__":
    main()

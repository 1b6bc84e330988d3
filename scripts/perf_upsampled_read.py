"""Bicubic up-sampling WSI reads on the GPU: ``tia_gather_cubic_resize_u8`` through ``VirtualWSIReader(..., upsample=True)``, and
the engines' WSI mode through that view.

Workload: a 10,000 x 10,000 x 3 synthetic slide at 0.5 mpp (300 MB), read entirely at 0.25 mpp as 256 x 256 patches: the
view is 20,000 x 20,000, 79 x 79 = 6,241 patches (the right / bottom ones padded with 255), 1.2 GB written, beyond the 256 MiB
Infinity Cache.  Each patch reads a 128 x 128 baseline region.

    python scripts/perf_upsampled_read.py --out DIR [--kernels-only] [--reps N] [--no-hovernet]

``--kernels-only`` runs the read alone (for ``rocprofv3 --kernel-trace --stats``); without it the script also times it with
device events, runs PatchPredictor (resnet18-kather100k at 0.25 mpp, 256 x 256 patches) in WSI mode through the view against
the same run on the slide pre-up-sampled into an ``ArrayWSIReader`` at 0.25 mpp (alternating, median of 3), and times
MultiTaskSegmentor (hovernet_fast-pannuke, seeded random weights) in WSI mode through the view of a 2,048^2 crop of the slide.
Algorithmic bytes: ``M * Wb * Hb * c`` read + ``M * pw * ph * c`` written; HBM peak 8 TB/s.  Prints one JSON line and writes it
to ``DIR/perf_upsampled_read[_kernels].json``.
"""

from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12
SIDE, PATCH, MPP, READ_MPP = 10000, 256, 0.5, 0.25
HOVER_SIDE = 2048


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


def _timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-hovernet", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        msg = "perf_upsampled_read needs a GPU"
        raise SystemExit(msg)
    from tiatoolbox_amd.tools.patchextraction import PatchExtractor
    from tiatoolbox_amd.wsicore import ArrayWSIReader, VirtualWSIReader

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    slide = torch.randint(0, 256, (SIDE, SIDE, 3), dtype=torch.uint8, device=dev, generator=gen)
    virt = VirtualWSIReader(slide, mpp=MPP, power=20.0, upsample=True)
    view = virt.at_resolution(READ_MPP, "mpp")
    s = view.factor
    grid = PatchExtractor.get_coordinates(image_shape=view.slide_dimensions, patch_input_shape=(PATCH, PATCH),
                                          stride_shape=(PATCH, PATCH))
    m = len(grid)
    b_view = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.int32)).to(dev)
    wb = int(np.round(PATCH * s))
    out_bytes = m * PATCH * PATCH * 3
    alg = m * wb * wb * 3 + out_bytes

    def read():
        return view.read_bounds_batch(b_view, size=(PATCH, PATCH))

    res = {"slide": [SIDE, SIDE, 3], "mpp": MPP, "read_mpp": READ_MPP, "scale": s, "view": list(view.slide_dimensions),
           "patches": m, "patch": PATCH, "region": wb, "out_bytes": out_bytes, "alg_bytes": alg}
    if args.kernels_only:
        for _ in range(args.reps):
            read()
        torch.cuda.synchronize()
        _write(args, res)
        return
    t = _event_ms(read, args.reps)
    res.update({"read_ms": round(t, 4), "read_alg_GBps": round(alg / t / 1e6, 1),
                "read_frac_hbm_peak": round(alg / (t * 1e-3) / HBM_PEAK, 4)})

    # end to end: PatchPredictor WSI mode at 0.25 mpp through the view against the slide pre-up-sampled (the same bytes)
    from tiatoolbox_amd.models.engine.io_config import ModelIOConfigABC
    from tiatoolbox_amd.models.engine.patch_predictor import PatchPredictor

    vw, vh = view.slide_dimensions
    up = view.read_bounds_batch(np.array([[0, 0, vw, vh]], np.int32))[0].contiguous()  # 1.2 GB
    arr = ArrayWSIReader(up, mpp=READ_MPP, power=40.0)
    cfg = ModelIOConfigABC(input_resolutions=[{"units": "mpp", "resolution": READ_MPP}], patch_input_shape=(PATCH, PATCH),
                           stride_shape=(PATCH, PATCH), output_resolutions=[])
    mask = np.ones((SIDE // 32, SIDE // 32), np.uint8)
    eng = PatchPredictor("resnet18-kather100k", batch_size=128, device="cuda")
    times: dict[str, list[float]] = {"view": [], "array": []}
    outs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(4):  # rep 0 warms up; the two forms alternate
            for name, reader in (("view", virt), ("array", arr)):
                box = {}

                def run(name=name, reader=reader, rep=rep, box=box):
                    box["path"] = eng.run([reader], masks=[mask], patch_mode=False, ioconfig=cfg, return_probabilities=True,
                                          save_dir=Path(tmp) / f"{name}{rep}")[0]

                dt = _timed(run)
                if rep:
                    times[name].append(dt)
                with np.load(box["path"]) as z:
                    outs[name] = {k: z[k] for k in z.files}
    del arr, up
    for name, ts in times.items():
        med = float(np.median(ts))
        n = len(outs[name]["coordinates"])
        res.update({f"e2e_{name}_patches": n, f"e2e_{name}_s": [round(x, 4) for x in ts], f"e2e_{name}_median_s": round(med, 4),
                    f"e2e_{name}_ms_per_patch": round(1e3 * med / n, 5)})
    res["e2e_view_over_array_per_patch"] = round(res["e2e_view_ms_per_patch"] / res["e2e_array_ms_per_patch"], 4)
    res["e2e_same_coordinates"] = bool(np.array_equal(outs["view"]["coordinates"], outs["array"]["coordinates"]))
    res["e2e_same_predictions"] = bool(np.array_equal(outs["view"]["predictions"], outs["array"]["predictions"]))
    res["e2e_max_abs_prob_diff"] = float(np.abs(outs["view"]["probabilities"] - outs["array"]["probabilities"]).max())

    if not args.no_hovernet:
        res.update(_hovernet(slide))
    _write(args, res)


def _hovernet(slide: torch.Tensor) -> dict:
    """MultiTaskSegmentor (hovernet_fast-pannuke, 0.25 mpp) WSI mode through the view of a HOVER_SIDE^2 crop at 0.5 mpp."""
    from tiatoolbox_amd.models.engine.multi_task_segmentor import MultiTaskSegmentor
    from tiatoolbox_amd.wsicore import VirtualWSIReader

    torch.manual_seed(0)
    crop = slide[:HOVER_SIDE, :HOVER_SIDE].contiguous()
    virt = VirtualWSIReader(crop, mpp=MPP, power=20.0, upsample=True)
    mask = np.ones((HOVER_SIDE // 16, HOVER_SIDE // 16), np.uint8)
    eng = MultiTaskSegmentor("hovernet_fast-pannuke", batch_size=32, device="cuda")
    ts = []
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(4):  # rep 0 warms up
            dt = _timed(lambda rep=rep: eng.run([virt], masks=[mask], patch_mode=False, save_dir=Path(tmp) / f"h{rep}"))
            if rep:
                ts.append(dt)
    return {"hovernet_view": [2 * HOVER_SIDE, 2 * HOVER_SIDE], "hovernet_s": [round(x, 3) for x in ts],
            "hovernet_median_s": round(float(np.median(ts)), 3)}


def _write(args, res: dict) -> None:
    line = json.dumps(res)
    print(line)
    args.out.mkdir(parents=True, exist_ok=True)
    name = "perf_upsampled_read_kernels" if args.kernels_only else "perf_upsampled_read"
    (args.out / f"{name}.json").write_text(line + "\n")


if __name__ == "__main__":
    main()

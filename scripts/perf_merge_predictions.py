"""``merge_predictions`` on the GPU: list building and ``tia_merge_patch_rects_f32`` timed apart, against the host NumPy loop.

Workload: C = 9 softmax rows for the patch grid of a 100,000 x 100,000 slide at 20x (every grid patch kept):
  (a) 224 / 224 grid (447 x 447 = 199,809 patches) to a 1.25x map (6,250 x 6,250);
  (b) 224 / 112 grid (893 x 893 = 797,449 patches) to the same map;
  (c) 224 / 224 grid to a 5x map (25,000 x 25,000).

    python scripts/perf_merge_predictions.py --out FILE [--reps N] [--cases abc] [--no-host]

Timing: one device-event pair per repetition, 3 warm-ups, ``--reps`` (>= 20) repetitions, the median.  The kernel
is timed in the engine's two forms: labels alone, and labels + the raw probability map (``return_probabilities``).  Algorithmic
bytes: every output written once, values and rectangles read once, the lists (offsets and items) read once; HBM peak 8 TB/s.
The host NumPy form (``device="cpu"``, labels) runs once on the same inputs.  Prints one JSON line per case and appends it to
FILE.
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
SLIDE, PATCH, C = 100_000, 224, 9
CASES = {"a": (224, 16), "b": (112, 16), "c": (224, 4)}  # stride, down-sampling ratio of the map from the 20x patch space
WARMUP = 3


def _median_ms(fn, reps: int) -> float:
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times))


def _case(name: str, reps: int, host: bool) -> dict:
    from tiatoolbox_amd.models.engine import _patch_merge as pm

    stride, ratio = CASES[name]
    dev = torch.device("cuda")
    pos = np.arange(0, SLIDE, stride, dtype=np.int64)
    gx, gy = np.meshgrid(pos, pos)
    coords = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + PATCH, gy.ravel() + PATCH], axis=1)
    n = len(coords)
    w, h = pm.canvas_size((SLIDE, SLIDE), float(ratio))
    rects = pm.patch_rects(coords, (SLIDE, SLIDE), (h, w))
    gen = torch.Generator(device=dev).manual_seed(0)
    probs = torch.softmax(2.0 * torch.randn((n, C), device=dev, generator=gen), dim=1).contiguous()
    rects_dev = torch.from_numpy(rects).to(dev)
    tile = pm.choose_tile(rects)
    offsets, items = pm.build_tile_lists(rects_dev, h, w, tile, tile)
    pairs = int(offsets[-1])
    res = {"case": name, "patches": n, "stride": stride, "canvas": [h, w], "classes": C, "tile": tile, "tiles": len(offsets) - 1,
           "pairs": pairs, "pairs_per_patch": round(pairs / n, 3)}
    res["lists_ms"] = round(_median_ms(lambda: pm.build_tile_lists(rects_dev, h, w, tile, tile), reps), 4)
    inputs = 4 * (n * C + n * 4 + len(offsets) + pairs)
    for tag, want, per_pixel in (("labels", ("labels",), 1), ("labels_raw", ("labels", "raw"), 1 + 4 * C)):
        ms = _median_ms(lambda want=want: pm.launch_merge(rects_dev, probs, h, w, offsets, items, tile, tile, want), reps)
        alg = h * w * per_pixel + inputs
        res.update({f"kernel_{tag}_ms": round(ms, 4), f"kernel_{tag}_alg_bytes": alg,
                    f"kernel_{tag}_alg_GBps": round(alg / ms / 1e6, 1),
                    f"kernel_{tag}_frac_hbm_peak": round(alg / (ms * 1e-3) / HBM_PEAK, 4)})
    # end to end through the public low-level form (rectangles from the host, guard, lists, kernel), CUDA rows in and out
    res["merge_patch_rects_labels_ms"] = round(_median_ms(lambda: pm.merge_patch_rects(rects, probs, (h, w)), reps), 4)
    if host:
        print(json.dumps(res | {"host": "pending"}), flush=True)  # the device figures survive a host form that runs out of memory
        got = pm.merge_patch_rects(rects, probs, (h, w))["labels"].cpu().numpy()
        probs_np = probs.cpu().numpy()
        t0 = time.perf_counter()
        exp = pm.merge_patch_rects(rects, probs_np, (h, w), device="cpu")["labels"]
        res["host_numpy_labels_s"] = round(time.perf_counter() - t0, 3)
        res["device_equals_host"] = bool(np.array_equal(got, exp))
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--no-host", action="store_true", help="skip the host NumPy form")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        msg = "perf_merge_predictions needs a GPU"
        raise SystemExit(msg)
    if args.reps < 20:  # noqa: PLR2004
        msg = "at least 20 repetitions (SURVEY 8(d))"
        raise SystemExit(msg)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    for name in args.cases:
        line = json.dumps(_case(name, args.reps, not args.no_host))
        print(line, flush=True)
        with args.out.open("a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

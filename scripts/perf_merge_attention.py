"""``merge_attention`` on the GPU: ``tia_merge_patch_grids_f32`` alone against the host NumPy loop, and what the option
adds to a WSI-mode run.

Kernel cases: 20,000 patches (a grid of 200 x 100) of 224 x 224 pixels with a 16 x 16 map each, at stride 224 (no overlap) and 112 (every
pixel under four patches), C = 1 ("rollout") and 16 ("class" of a 16-head model), merged to a map 16 and 4 times coarser than the patch
space, nearest and bilinear: 16 cases.  Per case ``launch_merge`` (``raw`` + ``count``, what the engine asks for) is timed with one HIP
event pair per repetition after ``--warmup`` launches; the figure is the median of ``--reps`` (>= 20), the spread the inter-quartile
range, minimum and maximum kept.  Algorithmic bytes: every output written once; maps, rectangles, affines and the lists read once; over
the median as a share of the 8 TB/s HBM peak.  The list building (``build_tile_lists``) is timed apart.  The comparator is the same work
in the package's host NumPy loop (``device="cpu"``, timed once with a host clock on this machine's CPU) -- what a user does without the
kernel, the ``N x C x gh x gw`` copy to the host not counted -- and the two results are compared bit for bit.  Host runs whose output
exceeds ``--host-max-elems`` elements are skipped and say so.

End to end: ``DeepFeatureExtractor`` on a seeded ``UNI`` (random weights: no checkpoint is read), bfloat16, a synthetic slide of
``--slide`` pixels at stride 224, WSI mode, ``--e2e-reps`` runs with and without ``merge_attention="rollout"`` in turn after one warm-up
of each, host clock around ``run()`` (which ends with the device synchronised and the ``.npz`` written).  The run without the kwarg is
the parent's behaviour: the files hold the same keys and the loop launches the same kernels.

    python scripts/perf_merge_attention.py --out-prefix profiles/attention_merge_perf [--reps 20] [--no-host] [--no-e2e] [--no-kernel]

Writes ``<prefix>.json`` (every record) and ``<prefix>.txt`` (one line per figure).  Needs a GPU: there is no fall-back."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12
PATCH, GRID, COLS, ROWS = 224, 16, 200, 100


def _timed_ms(fn, warmup: int, reps: int) -> dict:
    for _ in range(warmup):
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
    q = statistics.quantiles(times, n=4)
    return {"ms": statistics.median(times), "iqr_ms": q[2] - q[0], "min_ms": min(times), "max_ms": max(times)}


def kernel_cases(args, emit) -> None:
    from tiatoolbox_amd.models.engine import _attention_merge as am
    from tiatoolbox_amd.models.engine import _patch_merge as pm

    dev = torch.device("cuda")
    for stride in (224, 112):
        xs, ys = np.arange(COLS, dtype=np.int64) * stride, np.arange(ROWS, dtype=np.int64) * stride
        gx, gy = np.meshgrid(xs, ys)
        coords = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + PATCH, gy.ravel() + PATCH], axis=1)
        space = (int(xs[-1]) + PATCH, int(ys[-1]) + PATCH)
        n = len(coords)
        for c in (1, 16):
            gen = torch.Generator(device=dev).manual_seed(c)
            maps = torch.rand((n, c, GRID, GRID), device=dev, generator=gen)
            maps = (maps / maps.sum((-2, -1), keepdim=True)).contiguous()
            for ratio in (16, 4):
                w, h = pm.canvas_size(space, float(ratio))
                rects = pm.patch_rects(coords, space, (h, w))
                affine = am.patch_affines(coords, rects, space, (h, w), (GRID, GRID))
                rects_dev, affine_dev = torch.from_numpy(rects).to(dev), torch.from_numpy(affine).to(dev)
                tile = pm.choose_tile(rects)
                offsets, items = pm.build_tile_lists(rects_dev, h, w, tile, tile)
                pairs = int(offsets[-1])
                lists = _timed_ms(lambda: pm.build_tile_lists(rects_dev, h, w, tile, tile), args.warmup, args.reps)  # noqa: B023
                written = 4 * h * w * (c + 1)
                read = 4 * (n * c * GRID * GRID + 8 * n + len(offsets) + pairs)
                for mode in am.INTERPOLATIONS:
                    def launch(mode=mode):
                        return am.launch_merge(rects_dev, affine_dev, maps, h, w, offsets, items, tile, tile, mode, ("raw", "count"))  # noqa: B023

                    t = _timed_ms(launch, args.warmup, args.reps)
                    rec = {"what": "kernel", "patches": n, "stride": stride, "channels": c, "ratio": ratio, "canvas": [h, w], "mode": mode,
                           "tile": tile, "tiles": len(offsets) - 1, "pairs": pairs, "lists_ms": round(lists["ms"], 4), **{k: round(v, 4) for k, v in t.items()},
                           "bytes_written": written, "bytes_read": read, "GBps": round((written + read) / t["ms"] / 1e6, 1),
                           "share_of_hbm_peak": round((written + read) / (t["ms"] * 1e-3) / HBM_PEAK, 4)}
                    if args.no_host:
                        rec["host"] = "not run"
                    elif c * h * w > args.host_max_elems:
                        rec["host"] = f"skipped: {c * h * w} output elements"
                    else:
                        got = launch()
                        maps_np = maps.cpu().numpy()
                        t0 = time.perf_counter()
                        exp = am.merge_patch_grids(coords, maps_np, space, (h, w), interpolation=mode, want=("raw", "count"), device="cpu")
                        rec["host_numpy_s"] = round(time.perf_counter() - t0, 3)
                        rec["host_over_kernel"] = round(rec["host_numpy_s"] * 1e3 / t["ms"], 1)
                        rec["device_equals_host"] = bool(np.array_equal(got["raw"].cpu().numpy(), exp["raw"])
                                                         and np.array_equal(got["count"].cpu().numpy(), exp["count"]))
                        del got, exp
                    emit(rec, f"kernel  stride {stride:3d}  C {c:2d}  1/{ratio:<2d} ({w} x {h})  {mode:8s}  {t['ms']:8.3f} ms  iqr {t['iqr_ms']:.3f}  "
                              f"[{t['min_ms']:.3f} .. {t['max_ms']:.3f}]  {rec['GBps']:7.1f} GB/s = {100 * rec['share_of_hbm_peak']:.1f} % of 8 TB/s  "
                              f"lists {lists['ms']:.3f} ms  host NumPy: {rec.get('host_numpy_s', rec.get('host'))}"
                              + (f" s = {rec['host_over_kernel']} x, equal bits: {rec['device_equals_host']}" if "host_numpy_s" in rec else ""))
            del maps
            torch.cuda.empty_cache()


def end_to_end(args, emit) -> None:
    from tiatoolbox_amd.models import DeepFeatureExtractor, IOPatchPredictorConfig
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func
    from tiatoolbox_amd.wsicore import ArrayWSIReader

    w, h = args.slide
    slide = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    reader = ArrayWSIReader(slide, mpp=0.5, power=20.0)
    torch.manual_seed(0)
    model = TimmBackbone("UNI")
    model.preproc_func = timm_preproc_func("UNI")
    eng = DeepFeatureExtractor(model.eval(), batch_size=args.batch, device="cuda")
    cfg = IOPatchPredictorConfig(input_resolutions=[{"units": "mpp", "resolution": 0.5}], patch_input_shape=(224, 224), stride_shape=(224, 224))
    variants = {"without": {}, "merge_attention=rollout": {"merge_attention": "rollout"}}
    times = {name: [] for name in variants}
    keys = {}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(args.e2e_reps + 1):  # (round 0: the warm-up of each variant)
            for name, kw in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = eng.run([reader], patch_mode=False, ioconfig=cfg, compute_dtype="bfloat16", auto_get_mask=False,
                              save_dir=Path(tmp) / f"{rep}-{len(kw)}", **kw)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                with np.load(out[0]) as data:
                    keys[name] = {k: list(data[k].shape) for k in data.files}
    rec = {"what": "end to end", "model": "UNI (seeded random weights)", "compute_dtype": "bfloat16", "slide": [w, h], "batch": args.batch,
           "reps": args.e2e_reps, "arrays": keys}
    for name, ts in times.items():
        rec[name] = {"s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "times": [round(t, 4) for t in ts]}
    rec["added_s"] = round(rec["merge_attention=rollout"]["s"] - rec["without"]["s"], 4)
    patches = keys["without"]["coordinates"][0]
    emit(rec, f"end to end  UNI bf16  slide {w} x {h}  {patches} patches  without {rec['without']['s']:.3f} s [{rec['without']['min_s']:.3f} .. "
              f"{rec['without']['max_s']:.3f}]  with rollout {rec['merge_attention=rollout']['s']:.3f} s [{rec['merge_attention=rollout']['min_s']:.3f} .. "
              f"{rec['merge_attention=rollout']['max_s']:.3f}]  added {rec['added_s']:+.3f} s  (maps in the forward, the merge and three more arrays in the file)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-prefix", type=Path, required=True)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-max-elems", type=int, default=1 << 28)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--slide", type=int, nargs=2, default=(8960, 6720), metavar=("W", "H"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--e2e-reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_merge_attention.py measures on a GPU; none is visible.")
    if args.reps < 20:  # noqa: PLR2004
        sys.exit("at least 20 repetitions")
    args.out_prefix.parent.mkdir(parents=True, exist_ok=True)
    records, lines = [], [f"{torch.cuda.get_device_name(0)}; warm-up {args.warmup}, {args.reps} repetitions, median, inter-quartile range, [min .. max]"]

    def emit(rec: dict, line: str) -> None:
        records.append(rec)
        lines.append(line)
        print(line, flush=True)
        args.out_prefix.with_suffix(".json").write_text(json.dumps(records, indent=1) + "\n")
        args.out_prefix.with_suffix(".txt").write_text("\n".join(lines) + "\n")

    if not args.no_kernel:
        kernel_cases(args, emit)
    if not args.no_e2e:
        end_to_end(args, emit)


if __name__ == "__main__":
    main()

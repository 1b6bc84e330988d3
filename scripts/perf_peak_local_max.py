"""What ``utils.peaks.peak_local_max`` takes on the device.

Maps of ``--sides`` (default 4096 and 16384) squared, float32, ``min_distance`` 4 and 8, of two kinds: ``random`` (uniform noise: no
two candidates within reach of each other, nothing contested) and ``plateau`` (box-filtered noise stretched to [0, 1] and rounded to
41 levels: every hill top is a plateau and most candidates are contested, so their coordinates go through the host walk).

Per case, ``--reps`` rounds after ``--warmup``, one HIP event pair each, medians:

* ``scan``: ``tia_peak_scan_f32`` alone -- minimum / maximum, window maximum, candidate flags, contested count, count pass.  The bytes
  are the map read once, ``h w 4``, over the median time, beside the 8 TB/s roof.
* ``call``: the whole ``peak_local_max`` -- scan, the read of the totals, write pass, the contested candidates' trip through
  ``tia_peak_resolve_host``, the stable sort -- ending with the coordinates on the device.

Maps under 512 MB are rotated over enough buffers that no call finds its map in the 256 MiB Infinity Cache.  On the smaller side the
same call on the SciPy statement (``utils/_peaks.peak_local_max_ref``) on the host is timed once with the wall clock and its result
compared with the device's.  One GPU.

usage: perf_peak_local_max.py [--sides 4096,16384] [--distances 4,8] [--warmup 2] [--reps 7] [--out FILE.json]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F  # noqa: N812

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

HBM_PEAK = 8e12  # bytes/s
L3_BYTES = 256 << 20


def make_map(side: int, kind: str, seed: int) -> torch.Tensor:
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((side, side), device="cuda", generator=g)
    if kind == "random":
        return x
    for _ in range(2):
        x = F.avg_pool2d(x[None, None], 9, stride=1, padding=4, count_include_pad=False)[0, 0]
    x = (x - x.min()) / (x.max() - x.min())
    return (torch.round(x * 40) / 40).contiguous()


def median_ms(fn, warmup: int, reps: int) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="4096,16384")
    ap.add_argument("--distances", default="4,8")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_peak_local_max.py measures on a GPU; none is visible.")
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.utils import _peaks, peaks

    lib = _lib.load()
    sides = [int(s) for s in args.sides.split(",")]
    report = {"device": torch.cuda.get_device_name(0), "cases": []}
    for side in sides:
        nbytes = side * side * 4
        count = 1 if nbytes >= 2 * L3_BYTES else -(-2 * L3_BYTES // nbytes) + 1
        for kind in ("random", "plateau"):
            maps = [make_map(side, kind, 100 + i) for i in range(count)]
            chunks = int(lib.tia_peak_chunks(side, side))
            ws = {"minmax": torch.empty((1, 2), dtype=torch.int32, device="cuda"),
                  "flags": torch.empty((side, side), dtype=torch.uint8, device="cuda"),
                  "state": torch.empty((side, side), dtype=torch.uint8, device="cuda"),
                  "offsets": torch.empty((1, chunks), dtype=torch.int32, device="cuda"),
                  "totals": torch.empty(1, dtype=torch.int64, device="cuda")}
            for d in (int(v) for v in args.distances.split(",")):
                turn = {"scan": 0, "call": 0}

                def scan(d=d, maps=maps, ws=ws, side=side, turn=turn):
                    turn["scan"] += 1
                    rc = lib.tia_peak_scan_f32(maps[turn["scan"] % len(maps)].data_ptr(), 1, side, side, d, 0, 0.0, 0, 0.0, 0,
                                               ws["minmax"].data_ptr(), ws["flags"].data_ptr(), ws["state"].data_ptr(),
                                               ws["offsets"].data_ptr(), ws["totals"].data_ptr(), _lib.current_stream())
                    _lib.check(rc, "tia_peak_scan_f32")

                def call(d=d, maps=maps, turn=turn):
                    turn["call"] += 1
                    return peaks.peak_local_max(maps[turn["call"] % len(maps)], min_distance=d)

                res = {"scan": median_ms(scan, args.warmup, args.reps), "call": median_ms(call, args.warmup, args.reps)}
                scan()
                torch.cuda.synchronize()
                candidates = int(ws["totals"][0])
                contested = int((ws["state"] == 2).sum())  # noqa: PLR2004
                found = call()
                case = {"side": side, "kind": kind, "min_distance": d, "buffers": len(maps), "bytes": nbytes, "candidates": candidates,
                        "contested": contested, "peaks": int(found.shape[0]), **res}
                for name in ("scan", "call"):
                    case[name]["tb_per_s"] = nbytes / (case[name]["ms"] * 1e-3) / 1e12
                    case[name]["share_of_8_tb_per_s"] = nbytes / (case[name]["ms"] * 1e-3) / HBM_PEAK
                line = (f"{side}^2 {kind:8s} d={d}: scan {res['scan']['ms']:8.3f} ms = {case['scan']['tb_per_s']:.3f} TB/s "
                        f"({100 * case['scan']['share_of_8_tb_per_s']:.1f} % of 8 TB/s)   call {res['call']['ms']:9.3f} ms "
                        f"[{res['call']['min_ms']:.3f} .. {res['call']['max_ms']:.3f}] = {case['call']['tb_per_s']:.3f} TB/s   "
                        f"candidates {candidates}, contested {contested}, peaks {case['peaks']}; {len(maps)} rotating map(s)")
                if side == min(sides):
                    host = maps[turn["call"] % len(maps)].cpu().numpy()
                    t0 = time.perf_counter()
                    exp = _peaks.peak_local_max_ref(host, d)
                    case["host_statement_s"] = time.perf_counter() - t0
                    case["equal_to_statement"] = bool(np.array_equal(found.cpu().numpy(), exp))
                    line += f"; SciPy statement on the host {case['host_statement_s']:.2f} s, equal: {case['equal_to_statement']}"
                print(line, flush=True)
                report["cases"].append(case)
            del maps, ws
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()

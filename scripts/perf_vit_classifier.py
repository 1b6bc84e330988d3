"""A Vision Transformer classifier from uint8 patches to probabilities (``TimmModel`` / ``FusedViTClassifier``): a seeded
``--model`` (default ``UNI``) plus a ``--classes``-way head on ``--batch`` x ``--side``^2 uint8 patches, in bfloat16 and float16, in ONE
session:

(a) the new path on a device-resident batch: ``FusedViTClassifier.forward_uint8`` -- the hook's table inside the im2col
    (``tia_vit_patchify_norm_u8_h``), the graph, the head kernel (``tia_linear_softmax_rows_f32``);
(b) the same commit with the deferral off: the hook's batched gather (a torch index kernel writing the normalised batch in the run's
    dtype), ``FusedViT.forward`` on it, ``classifier`` and ``softmax`` as torch operations on the float32 features -- what a user
    could assemble before;
(c) the host-fed engine run (``PatchPredictor.run`` on a NumPy array, upload included): the hook as the engine knows it (deferred)
    against the same hook wrapped in a plain Python callable, which the engine applies per patch on the host and uploads as float32.

(a) and (b) alternate inside a round and are timed with HIP events around ``--reps`` calls (median, min and max over ``--rounds``);
(c) is the host clock around whole ``run()`` calls, each ending in the copy of the results to the host, after one warm-up run of
each (the first builds the inference copy).  The outputs of (a) and (b) are compared before anything is timed.

usage: perf_vit_classifier.py [--model UNI] [--classes 9] [--batch 256] [--side 224] [--depth N] [--rounds 5] [--reps 3] [--host-runs 5]
                              [--out FILE.json]"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from perf_vit import HALVES, alternate, build  # noqa: E402


def classifier_of(vit, classes: int):
    """A ``TimmModel``-shaped module around the seeded ``vit`` (no second allocation of the trunk) with a classifier N(0, 4 / F)."""
    from tiatoolbox_amd.models.architecture.vanilla import TimmModel

    with torch.device("meta"):
        model = TimmModel("vit_small_patch16_224", classes)
    model.feat_extract = vit
    width = vit.embed_dim * (2 if vit.global_pool == "token_mean" else 1)
    model.classifier = torch.nn.Linear(width, classes, device="cuda")
    with torch.no_grad():
        model.classifier.weight.normal_(0.0, 2.0 / width ** 0.5)
        model.classifier.bias.normal_(0.0, 0.1)
    return model.eval()


def fused_of(model, dtype):
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViTClassifier

    fused = FusedViTClassifier(model)
    fused.feat_extract.prepare(dtype)
    return fused.to(dtype).eval()


def host_runs(model, patches: np.ndarray, dtype_name: str, runs: int, side: int) -> dict:
    """(c): whole ``PatchPredictor.run`` calls on the host array, seconds by the host clock (the results are on the host when it returns)."""
    from tiatoolbox_amd.models import IOPatchPredictorConfig, PatchPredictor
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    cfg = IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(side, side),
                                 stride_shape=(side, side))
    hook = timm_preproc_func("UNI")
    out, probs = {}, {}
    for name, func in (("host-fed, hook deferred", hook), ("host-fed, hook as a Python callable", lambda img: hook(img))):  # noqa: PLW0108
        eng_model = copy.deepcopy(model).float()
        eng_model.preproc_func = func
        eng = PatchPredictor(eng_model, batch_size=len(patches), device="cuda")
        times = []
        for i in range(runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = eng.run(patches, patch_mode=True, ioconfig=cfg, return_probabilities=True, compute_dtype=dtype_name)
            torch.cuda.synchronize()
            if i:  # (the first run builds and packs the inference copy)
                times.append((time.perf_counter() - t0) * 1e3)
        probs[name] = res["probabilities"]
        out[name] = {"ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}
        del eng, eng_model
        torch.cuda.empty_cache()
    a, b = probs.values()
    out["max_abs_difference"] = float(np.abs(a - b).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="UNI")
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--depth", type=int, default=0, help="override the number of blocks (0: the model's own)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=5, help="timed engine runs per host-fed variant (0: skip (c))")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perf_vit_classifier.py measures on a GPU; none is visible.")
    from tiatoolbox_amd.models.dataset.classification import timm_preproc_func

    cfg, vit = build(args)
    model = classifier_of(vit, args.classes)
    hook = timm_preproc_func("UNI")
    patches = np.random.default_rng(1).integers(0, 256, (args.batch, args.side, args.side, 3), dtype=np.uint8)
    x = torch.from_numpy(patches).cuda()
    variants, results = {}, {"model": args.model, "config": cfg, "classes": args.classes, "batch": args.batch, "side": args.side,
                             "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    for name, dtype in HALVES.items():
        fused = fused_of(copy.deepcopy(model), dtype)
        table = hook.device_table("cuda", dtype)
        w, b = fused._w32, fused._b32  # noqa: SLF001

        def new(m=fused, t=table):
            return m.forward_uint8(x, t)

        def old(m=fused, d=dtype, w=w, b=b):
            feat = m.feat_extract(hook.device_batch(x, d).permute(0, 3, 1, 2))
            return torch.softmax(torch.nn.functional.linear(feat, w, b), -1)

        with torch.inference_mode():
            diff = float((new() - old()).abs().max())
        print(f"{name}: max |p(a) - p(b)| = {diff:.3e}", flush=True)
        results[f"max_abs_difference {name}"] = diff
        variants[f"(a) forward_uint8 + head kernel {name}"] = new
        variants[f"(b) hook gather + forward + torch head {name}"] = old
    res = alternate(variants, args.rounds, args.reps)
    print(f"{args.model} depth {cfg['depth']} + {args.classes} classes  {args.batch} x {args.side}^2 uint8  on {results['device']}")
    for name, r in res.items():
        r["patches_per_s"] = args.batch / r["ms"] * 1e3
        print(f"{name:48s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  {r['patches_per_s']:8.1f} patches/s", flush=True)
    results["device_resident"] = res
    del variants
    torch.cuda.empty_cache()
    if args.host_runs:
        for name in HALVES:
            host = host_runs(model, patches, name, args.host_runs, args.side)
            results[f"host_fed {name}"] = host
            for what, r in host.items():
                if isinstance(r, dict):
                    print(f"(c) {what + ' ' + name:48s} {r['ms']:9.2f} ms  [{r['min_ms']:.2f} .. {r['max_ms']:.2f}]  "
                          f"{args.batch / r['ms'] * 1e3:8.1f} patches/s", flush=True)
            print(f"(c) {name}: max |p deferred - p callable| = {host['max_abs_difference']:.3e}", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()

"""Bit-level record of what the fused segmentation graphs compute, for comparing two checkouts that share one C library.

``run``: builds ``FusedHoVerNet`` (the seeded ``fast`` / ``original`` / ``plus`` networks of ``tests/_hovernet_half_ref.py``) and
``FusedUNet`` (the seeded network of ``tests/test_unet_half.py``) the way ``EngineABC._inference_model`` does -- device ->
``set_conv_algo`` -> ``prepare`` -> cast -> channels-last -- in float32 ``direct``, float32 ``winograd``, fp16 and bf16, runs one
forward at the networks' smallest inputs (batch 1; ``fast`` also batch 2) and writes every output head's raw bytes and one SHA-256
per case into an ``.npz``.  ``--tree`` names the checkout whose package and test helpers are imported (default: this one); point
``TIA_LIB_PATH`` at one library for both runs, then any difference is a difference in the Python graph layer.

``compare``: the per-case table of two such files (hash equal or not, differing bytes); exit status 1 on any difference.

    python scripts/fused_graph_parity.py run --out head.npz
    python scripts/fused_graph_parity.py run --tree ../parent --out parent.npz
    python scripts/fused_graph_parity.py compare parent.npz head.npz
"""
import argparse
import copy
import hashlib
import os
import sys

import numpy as np

MODES = (("f32-direct", "float32", "direct"), ("f32-winograd", "float32", "winograd"), ("fp16", "float16", "direct"),
         ("bf16", "bfloat16", "direct"))


def cases():
    """``(name, plain model, x float NCHW in 0 .. 255)``: 5 inputs."""
    import _hovernet_half_ref as H  # noqa: N812
    import _unet_half_ref as U  # noqa: N812
    import torch
    from tiatoolbox_amd.models.architecture.unet import UNetModel

    for kind in ("fast", "original", "plus"):
        model, x, _ = H.graph_case(kind)
        yield f"hovernet-{kind}-n1", model, x[:1]
        if kind == "fast":
            yield "hovernet-fast-n2", model, x
    torch.manual_seed(2)
    unet = UNetModel(3, 5, "resnet50", decoder_block=[3, 3]).eval()
    g = U.randomise_bn(unet, 9)
    yield "unet-n1", unet, torch.randint(0, 256, (1, 3, 96, 128), generator=g).float()


def run(tree: str, out: str) -> None:
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    import tiatoolbox_amd.models.architecture.hovernet_fused as hf
    import torch
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.hovernet import HoVerNet
    from tiatoolbox_amd.models.architecture.hovernet_fused import FusedHoVerNet, set_conv_algo
    from tiatoolbox_amd.models.architecture.unet_fused import FusedUNet

    print(f"graph layer: {os.path.dirname(hf.__file__)}\nlibrary:     {_lib.lib_path()}", flush=True)
    record = {}
    for name, model, x in cases():
        for mode, dtype_name, algo in MODES:
            dtype = getattr(torch, dtype_name)
            plain = copy.deepcopy(model).to("cuda")
            fused = (FusedHoVerNet if isinstance(model, HoVerNet) else FusedUNet)(plain)
            set_conv_algo(fused, algo)
            fused = fused.to("cuda")
            if dtype != torch.float32:
                fused.prepare(dtype)
                fused = fused.to(dtype)
            fused = fused.to(memory_format=torch.channels_last).eval()
            with torch.inference_mode():
                got = fused(x.to("cuda", dtype).contiguous(memory_format=torch.channels_last))
                torch.cuda.synchronize()
            heads = got if isinstance(got, dict) else {"logits": got}
            sha = hashlib.sha256()
            for head, y in heads.items():
                raw = np.frombuffer(y.float().contiguous().cpu().numpy().tobytes(), dtype=np.uint8)
                record[f"{name}/{mode}/{head}"] = raw
                sha.update(raw.tobytes())
            record[f"{name}/{mode}/sha256"] = np.array(sha.hexdigest())
            print(f"{name:20s} {mode:13s} {sha.hexdigest()}", flush=True)
    np.savez(out, **record)


def compare(a_path: str, b_path: str) -> int:
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    print(f"{'case':36s} {'bytes':>10s} {'differing':>10s}  sha256 ({a_path} | {b_path})")
    for key in sorted(k for k in a.files if k.endswith("/sha256") and k in b.files):
        case = key[:-len("/sha256")]
        heads = [k for k in a.files if k.startswith(case + "/") and k != key and k in b.files]
        total = sum(a[k].size for k in heads)
        diff = sum(int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else max(a[k].size, b[k].size) for k in heads)
        same = str(a[key]) == str(b[key]) and diff == 0
        bad += [] if same else [case]
        print(f"{case:36s} {total:10d} {diff:10d}  {str(a[key])[:16]} {'==' if same else '!='} {str(b[key])[:16]}")
    print(f"{'all equal' if not bad else 'DIFFERENT: ' + ', '.join(bad)}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "run":
        run(os.path.abspath(args.tree), args.out)
    else:
        sys.exit(compare(args.a, args.b))

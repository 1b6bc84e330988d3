"""The half-precision attention kernels of two revisions side by side: bits and time ("one copy").

    python scripts/compare_attention_libs.py build REV OUT.so            # REV: a git revision, or WORKTREE (needs hipcc; no GPU)
    python scripts/compare_attention_libs.py bits PARENT.so BRANCH.so [--out FILE]
    python scripts/compare_attention_libs.py time PARENT.so BRANCH.so [--out FILE] [--rounds 9] [--window-ms 30]

``build`` compiles ``vit_attention.hip`` and ``vit_attention_maps.hip`` of a revision with the product's flags into a small library
of its own.  ``bits`` loads two such libraries into one process and calls ``tia_mha_fwd_h``, ``tia_mha_probs_h`` (``q_rows`` 1 and
``s``, head mean off and on) and ``tia_mha_probs_fused_h`` (mean / max / min) of both on the same seeded inputs: every output must be
byte-identical, there is no tolerance.  ``time`` measures the forward kernel and the rollout form of the probabilities kernel
(all rows, head mean) on the attention shapes of three backbones with ``perf_vit.alternate``: device events, every variant warmed,
variants alternating inside a round, repetitions sized for a window of tens of milliseconds.  The parent library is loaded twice
(a copy of the file: a second handle) and fills two slots, so every round also measures the parent against itself; the margin the
branch has to keep is that A/A spread: the distance of the two parent medians or the parent's own min .. max over the rounds,
whichever is larger."""
from __future__ import annotations

import argparse
import ctypes as C
import math
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "scripts")]

SOURCES = ("vit_attention.hip", "vit_attention_maps.hip")
ENTRY_POINTS = ("tia_mha_fwd_h", "tia_mha_probs_h", "tia_mha_probs_fused_h")
WORKLOADS = {"UNI": (256, 197, 16, 64), "H-optimus-0": (64, 261, 24, 64), "Virchow2": (64, 261, 16, 80)}  # n, s, heads, head_dim


def build(rev: str, out: Path) -> None:
    from isa_compare import extract
    from tiatoolbox_amd.build import HIPCC_FLAGS

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        extract(rev, Path(tmp))
        csrc = Path(tmp) / "tiatoolbox_amd" / "csrc"
        subprocess.run([hipcc, *HIPCC_FLAGS, "-shared", f"-I{Path(tmp) / 'include'}", f"-I{csrc}", *[str(csrc / s) for s in SOURCES],
                        "-o", str(out)], check=True)


def load(path: Path) -> C.CDLL:
    from tiatoolbox_amd._lib import _SIGNATURES

    lib = C.CDLL(str(path))
    for name in ENTRY_POINTS:
        getattr(lib, name).argtypes, getattr(lib, name).restype = _SIGNATURES[name]
    return lib


def attention_data(kind: str, n: int, heads: int, s: int, hd: int, dtype):
    """``[n, s, 3, heads, hd]``: the ``gauss`` and ``late`` inputs of the kernel tests (tests/test_vit_kernels_gpu.py, and
    tests/test_vit_virchow_kernels_gpu.py for head_dim 80, whose shared component sits on dimension 72)."""
    import torch

    qkv = torch.randn((n, s, 3, heads, hd), generator=torch.Generator().manual_seed(s * 131 + heads * 7 + n + len(kind)))
    if kind == "late":
        d, t0 = (0 if hd == 64 else hd - 8), 64 * ((s - 1) // 64)
        qkv[:, :, 0, :, d] = 6.0
        qkv[:, :, 1, :, d] = 0.0
        qkv[:, t0:, 1, :, d] = 60.0
    return qkv.to(dtype).cuda()


def calls(lib: C.CDLL, qkv, forms):
    """{form: a function that launches it on ``qkv`` and returns its output}, outputs allocated once (poisoned with NaN)."""
    import torch
    from tiatoolbox_amd import _lib
    from tiatoolbox_amd.models.architecture.vit_fused import _DT
    from tiatoolbox_amd.models.engine._rollout_options import FUSION_CODES

    n, s, _, heads, hd = qkv.shape
    head = (qkv.data_ptr(),)
    dims, tail = (n, s, heads, hd, hd ** -0.5), (_DT[qkv.dtype], _lib.current_stream())
    made = {}

    def launch(name, out, *middle):
        _lib.check(getattr(lib, name)(*head, out.data_ptr(), *dims, *middle, *tail), name)
        return out

    for form in forms:
        kind, *opt = form.split(":")
        if kind == "fwd":
            out = torch.full((n, s, heads * hd), math.nan, dtype=qkv.dtype, device="cuda")
            made[form] = lambda out=out: launch("tia_mha_fwd_h", out)
        elif kind == "probs":
            q_rows, mean = (1 if opt[0] == "1" else s), int(opt[1])
            out = torch.full((n, q_rows, s) if mean else (n, heads, q_rows, s), math.nan, device="cuda")
            made[form] = lambda out=out, q_rows=q_rows, mean=mean: launch("tia_mha_probs_h", out, q_rows, mean)
        else:
            out = torch.full((n, s, s), math.nan, device="cuda")
            made[form] = lambda out=out, code=FUSION_CODES[opt[0]]: launch("tia_mha_probs_fused_h", out, code)
    return made


BIT_FORMS = ("fwd", "probs:1:0", "probs:1:1", "probs:s:0", "probs:s:1", "fused:mean", "fused:max", "fused:min")


def bits(parent: C.CDLL, branch: C.CDLL) -> tuple[list[str], int]:
    import torch

    cases = [("small", kind, 2, s, 3, hd) for hd in (64, 80) for s in (1, 17, 64, 65, 129, 261) for kind in ("gauss", "late")]
    cases += [(name, "gauss", n, s, heads, hd) for name, (n, s, heads, hd) in WORKLOADS.items()]
    lines, bad = [], 0
    for name, kind, n, s, heads, hd in cases:
        for dtype in (torch.float16, torch.bfloat16):
            qkv = attention_data(kind, n, heads, s, hd, dtype)
            differing = []
            for form in BIT_FORMS:  # one form at a time: a workload's per-head probabilities of all rows are its largest buffers
                a, b = (calls(lib, qkv, (form,))[form]() for lib in (parent, branch))
                torch.cuda.synchronize()
                word = torch.int16 if a.element_size() == 2 else torch.int32
                if not torch.equal(a.view(word), b.view(word)):
                    differing.append(f"{form} ({int((a.view(word) != b.view(word)).sum())} of {a.numel()} values)")
                del a, b
            bad += len(differing)
            lines.append(f"{name:12s} {kind:5s} n {n:3d} s {s:3d} heads {heads:2d} head_dim {hd} {str(dtype)[6:]:8s} "
                         + ("identical: " + " ".join(BIT_FORMS) if not differing else "DIFFERS: " + ", ".join(differing)))
    lines.append(f"outputs that differ: {bad}")
    return lines, bad


def time_(libs: dict[str, C.CDLL], rounds: int, window_ms: float) -> tuple[list[str], int]:
    import torch
    from perf_vit import alternate, ev

    lines, slower = [], 0
    for name, (n, s, heads, hd) in WORKLOADS.items():
        for dtype in (torch.bfloat16, torch.float16):
            qkv = attention_data("gauss", n, heads, s, hd, dtype)
            for form in ("fwd", "probs:s:1"):
                variants = {slot: calls(lib, qkv, (form,))[form] for slot, lib in libs.items()}
                variants["parent"]()
                torch.cuda.synchronize()
                reps = max(5, math.ceil(window_ms / ev(variants["parent"], 5)))
                alternate(variants, 1, reps)  # discarded: the first window after the calibration was 4 .. 8 % long in every slot it fell into
                res = alternate(variants, rounds, reps)
                p, again, br = (res[k] for k in ("parent", "parent again", "branch"))
                spread = max(abs(p["ms"] - again["ms"]), p["max_ms"] - p["min_ms"])
                verdict = "within" if abs(br["ms"] - p["ms"]) <= spread else ("FASTER than" if br["ms"] < p["ms"] else "SLOWER than")
                slower += verdict.startswith("SLOWER")
                lines.append(f"{name:12s} {str(dtype)[6:]:8s} {'forward' if form == 'fwd' else 'probabilities (rollout form)':28s} x{reps:4d}  "
                             + "  ".join(f"{k} {1e3 * r['ms']:8.2f} us [{1e3 * r['min_ms']:.2f} .. {1e3 * r['max_ms']:.2f}]" for k, r in res.items())
                             + f"  A/A spread {1e3 * spread:.2f} us: branch - parent {1e3 * (br['ms'] - p['ms']):+.2f} us, {verdict} the spread")
    lines.append(f"kernels slower than the parent beyond the A/A spread: {slower}")
    return lines, slower


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("build", "bits", "time"))
    ap.add_argument("first", help="build: the revision; bits / time: the parent's library")
    ap.add_argument("second", type=Path, help="build: the library to write; bits / time: the branch's library")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", type=Path)
    args = ap.parse_args()
    if args.mode == "build":
        build(args.first, args.second)
        return 0
    import torch

    head = [f"{args.mode}: parent {args.first}, branch {args.second}, on {torch.cuda.get_device_name(0)}"]
    if args.mode == "bits":
        lines, bad = bits(load(Path(args.first)), load(args.second))
    else:
        with tempfile.TemporaryDirectory() as tmp:  # (the same path again would return the first handle)
            twin = shutil.copy(args.first, Path(tmp) / "parent_again.so")
            lines, bad = time_({"parent": load(Path(args.first)), "branch": load(args.second), "parent again": load(Path(twin))},
                               args.rounds, args.window_ms)
    text = "\n".join(head + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        args.out.write_text(text)
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())

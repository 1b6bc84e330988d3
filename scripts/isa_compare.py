"""Compare the gfx950 device code of HIP sources between two git revisions.

    python scripts/isa_compare.py PARENT HEAD conv_mfma.hip conv_mfma_h.hip ... [--alias OLD=NEW ...] [--out report.txt]

For each revision ``tiatoolbox_amd/csrc`` and ``include`` are extracted into a temporary directory (``HEAD`` may be the word
``WORKTREE``: the files as they are on disk), every listed file is compiled with ``build.HIPCC_FLAGS`` plus
``--cuda-device-only -S``, and per kernel the report says whether the instruction stream is the same -- labels renumbered in
order of appearance, comments and assembler directives dropped -- and prints the register, spill, LDS, scratch and kernarg
figures of the code object's metadata.  Kernels are matched by their demangled signature without namespaces; ``--alias OLD=NEW``
(repeatable) replaces the substring ``OLD`` by ``NEW`` in the parent's signatures first, for kernels that the head renames.  A kernel
that differs gets its per-mnemonic instruction counts compared and the extent of the differing lines printed, as they are and with
register numbers masked (what is left then is reordering and real instruction changes).  The comparison is generic: no
instruction is looked for in particular.
"""

from __future__ import annotations

import argparse
import difflib
import functools
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tiatoolbox_amd.build import HIPCC_FLAGS  # noqa: E402

EXTRA = ["--cuda-device-only", "-S"]
META = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("spill_v", ".vgpr_spill_count"),
        ("spill_s", ".sgpr_spill_count"), ("lds", ".group_segment_fixed_size"), ("scratch", ".private_segment_fixed_size"),
        ("kernarg", ".kernarg_segment_size"))
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def extract(rev: str, dest: Path) -> None:
    """``tiatoolbox_amd/csrc`` and ``include`` of ``rev`` under ``dest`` (same relative layout: the sources include ../../include)."""
    for sub in ("tiatoolbox_amd/csrc", "include"):
        if rev == "WORKTREE":
            shutil.copytree(ROOT / sub, dest / sub)
        else:
            tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, sub], check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", str(dest)], input=tar, check=True)


def compile_asm(tree: Path, name: str, defines: tuple[str, ...] = ()) -> str:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = tree / "tiatoolbox_amd" / "csrc"
    cmd = [hipcc, *HIPCC_FLAGS, *EXTRA, *[f"-D{d}" for d in defines], f"-I{tree / 'include'}", f"-I{csrc}", str(csrc / name), "-o", "-"]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        raise SystemExit(f"{name} of {tree.name} does not compile:\n{done.stderr}")
    return done.stdout


def demangle(names: list[str]) -> dict[str, str]:
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([tool], input="\n".join(names) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    # a kernel is known by its signature without the namespaces: a type that moves into a shared header renames the symbol only
    return {n: d.replace("(anonymous namespace)::", "").replace("tia::", "") for n, d in zip(names, out)}


def parse(asm: str) -> tuple[dict[str, list[str]], dict[str, dict[str, int]], int]:
    """-> {kernel symbol: normalised instruction lines}, {kernel symbol: metadata}, number of other device functions"""
    lines = asm.splitlines()
    meta: dict[str, dict[str, int]] = {}
    # the amdhsa.kernels list of the metadata note: an entry per kernel opens with "  - .key:", its own keys are indented by four
    # spaces (the argument list lies deeper)
    entries: list[dict[str, str]] = []
    first = lines.index("amdhsa.kernels:") + 1 if "amdhsa.kernels:" in lines else len(lines)
    for ln in lines[first:]:
        m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", ln)
        if m:
            if m.group(1) == "  - ":
                entries.append({})
            entries[-1][m.group(2)] = m.group(3).strip()
        elif not ln.startswith(" "):
            break
    for e in entries:
        meta[e[".name"]] = {k: int(e.get(f, "0")) for k, f in META}
    functions = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", asm, re.M))
    streams: dict[str, list[str]] = {}
    code = [ln.split(";", 1)[0].strip() for ln in lines]
    for sym in meta:
        start = code.index(sym + ":")
        body, labels = [], {}
        for ln in lines[start + 1:]:
            s = ln.split(";", 1)[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or (s.startswith(".") and not LABEL.fullmatch(s.rstrip(":"))):
                continue  # blank, comment or directive
            body.append(s)
        for s in body:  # labels renumbered in order of first appearance (definition or reference)
            for m in LABEL.findall(s):
                labels.setdefault(m, f".L{len(labels)}")
        streams[sym] = [LABEL.sub(lambda m: labels[m.group(0)], re.sub(r"\s+", " ", s)) for s in body]
    return streams, meta, len(functions - set(meta))


def fmt(m: dict[str, int]) -> str:
    return (f"vgpr {m['vgpr']} agpr {m['agpr']} sgpr {m['sgpr']} spill v{m['spill_v']} s{m['spill_s']} lds {m['lds']} "
            f"scratch {m['scratch']} kernarg {m['kernarg']}")


def mnemonics(stream: list[str]) -> Counter:
    return Counter(s.split(" ", 1)[0] for s in stream if not s.endswith(":"))


def mask(stream: list[str]) -> list[str]:
    """register numbers dropped (v12 -> v, s[4:5] -> s[:]): what is left differs only where instructions do"""
    return [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", lambda m: m.group(1) + ("[:]" if ":" in m.group(2) else ""), s) for s in stream]


def where(parent: list[str], head: list[str]) -> str:
    ops = difflib.SequenceMatcher(None, parent, head, autojunk=False).get_opcodes()
    changed = [(i1, i2) for tag, i1, i2, _, _ in ops if tag != "equal"]
    if not changed:
        return "none"
    return (f"{sum(max(i2 - i1, 1) for i1, i2 in changed)} in {len(changed)} places, between line {changed[0][0] + 1} and line "
            f"{changed[-1][1]} of {len(parent)}")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("head")
    ap.add_argument("files", nargs="+", help="names of .hip files in tiatoolbox_amd/csrc")
    ap.add_argument("--variant", action="append", default=[], metavar="FILE:DEFINE",
                    help="also compile FILE of the head with -DDEFINE (developer builds: compile only)")
    ap.add_argument("--alias", action="append", default=[], metavar="OLD=NEW",
                    help="replace the substring OLD by NEW in the parent's demangled signatures before matching (renamed kernels)")
    ap.add_argument("--out", type=Path)
    args = ap.parse_args()
    aliases = [a.split("=", 1) for a in args.alias]
    report: list[str] = []
    differences = 0
    with tempfile.TemporaryDirectory() as tmp:
        trees = {}
        for side, rev in (("parent", args.parent), ("head", args.head)):
            trees[side] = Path(tmp) / side
            trees[side].mkdir()
            extract(rev, trees[side])
        jobs = [(side, f) for f in args.files for side in ("parent", "head")]
        with ThreadPoolExecutor(max_workers=16) as pool:
            asms = dict(zip(jobs, pool.map(lambda j: compile_asm(trees[j[0]], j[1]), jobs)))
            variants = [v.split(":", 1) for v in args.variant]
            ok = list(pool.map(lambda v: bool(compile_asm(trees["head"], v[0], (v[1],))), variants))
    report.append(f"device code, {args.parent} (parent) against {args.head} (head)")
    report.append("flags: " + " ".join([*HIPCC_FLAGS, *EXTRA]))
    report += [f"alias: {old} -> {new}" for old, new in aliases]
    for f in args.files:
        (ps, pm, pother), (hs, hm, hother) = parse(asms[("parent", f)]), parse(asms[("head", f)])
        names = demangle(sorted(set(ps) | set(hs)))
        renamed = {k: functools.reduce(lambda n, a: n.replace(*a), aliases, names[k]) for k in ps}
        ps, pm = ({renamed[k]: v for k, v in d.items()} for d in (ps, pm))
        hs, hm = ({names[k]: v for k, v in d.items()} for d in (hs, hm))
        report.append("")
        report.append(f"{f}: {len(ps)} kernels at the parent, {len(hs)} at the head; other device functions: {pother} / {hother}")
        for sym in sorted(set(ps) | set(hs)):
            if sym not in ps or sym not in hs:
                differences += 1
                report.append(f"  {'parent' if sym in ps else 'head'} only  {sym}")
                continue
            same = ps[sym] == hs[sym]
            if same and pm[sym] == hm[sym]:
                report.append(f"  same    {len(hs[sym]):4d} lines  {fmt(hm[sym])}  {sym}")
                continue
            differences += 1
            report.append(f"  {'same   ' if same else 'differs'} {len(ps[sym]):4d} -> {len(hs[sym]):4d} lines  {sym}")
            report.append(f"      parent  {fmt(pm[sym])}")
            report.append(f"      head    {fmt(hm[sym])}")
            pc, hc = mnemonics(ps[sym]), mnemonics(hs[sym])
            delta = {k: hc[k] - pc[k] for k in sorted(set(pc) | set(hc)) if hc[k] != pc[k]}
            report.append("      instruction counts (head - parent): " + (", ".join(f"{k} {v:+d}" for k, v in delta.items()) or "equal per mnemonic"))
            report.append("      lines of the parent that differ: " + where(ps[sym], hs[sym]))
            report.append("      the same with register numbers masked: " + where(mask(ps[sym]), mask(hs[sym])))
    if args.variant:
        report.append("")
        report.append("developer variants of the head (compile only):")
        report += [f"  {v[0]} -D{v[1]}: {'compiles' if o else 'no output'}" for v, o in zip(variants, ok)]
    report.append("")
    report.append(f"differences: {differences}")
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if args.out:
        args.out.write_text(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

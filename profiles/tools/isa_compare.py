#!/usr/bin/env python3
"""isa_compare.py TREE_A TREE_B -- do two checkouts compile to the same device code?

For every csrc/*.hip of both trees and for both flag sets of that tree's own csrc/build.sh (libmirt.so and libmirt_default.so) the file is
compiled to gfx950 assembly on the CPU (--cuda-device-only -S: no GPU is needed), the text is cut into one piece per function symbol -- from its
.type line to the end of the resource comment behind it, the kernel descriptor included -- and the pieces are compared as TEXT, line for line.
Lines holding the compiler's per-translation-unit __hip_cuid_ symbol are dropped, and the per-file function index in local labels (.LBB7_3,
.Lfunc_end7) is masked, so that a function added in front of another does not make that one differ.  Nothing else is interpreted.

Per symbol one of: identical; DIFFERS, with both code lengths and the resource fields of the code object's metadata; MISSING (in A only);
NEW (in B only).  The identical ones are counted per file and named only with --all (the grid builder alone brings 400 rocPRIM instances).
`git worktree add DIR COMMIT` makes a TREE_A of any commit.  At most 16 compile jobs.  Exit status 0 unless a compile fails.
"""
import argparse
import concurrent.futures
import os
import pathlib
import re
import shlex
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # as csrc/build.sh
FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
DEFAULT_FROM, DEFAULT_TO, DEFAULT_DEFINE = "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-DPT_PLAIN_DIV=1"


def find_csrc(tree):
    hits = sorted(p.parent for p in pathlib.Path(tree).glob("**/csrc/build.sh") if ".git" not in p.parts)
    if len(hits) != 1:
        sys.exit(f"{tree}: expected one csrc/build.sh, found {len(hits)}")
    return hits[0]


def flag_sets(csrc):
    """The two flag sets, read from build.sh itself so that they cannot drift from what the libraries are built with."""
    text = (csrc / "build.sh").read_text()
    m = re.search(r"^FLAGS=\((.*?)\)", text, re.S | re.M)
    if not m or DEFAULT_FROM not in m.group(1) or DEFAULT_TO not in text or DEFAULT_DEFINE not in text:
        sys.exit(f"{csrc / 'build.sh'}: FLAGS or the default contract's substitution are not where this tool reads them")
    flags = shlex.split(m.group(1))
    return {"libmirt.so": flags, "libmirt_default.so": [DEFAULT_TO if f == DEFAULT_FROM else f for f in flags] + [DEFAULT_DEFINE]}


def compile_asm(hipcc, flags, src, out):
    r = subprocess.run([hipcc, *flags, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", "-o", str(out), str(src)], capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{src}: compile failed\n{r.stderr}")
    return out


def split_symbols(asm):
    """{symbol: {"text": [lines], "len": codeLenInByte, fields...}}"""
    lines = [l for l in asm.splitlines() if "__hip_cuid_" not in l]
    syms, i = {}, 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        j = i + 1
        while j < len(lines) and not lines[j].startswith("; codeLenInByte"):
            j += 1
        length = int(lines[j].split("=")[1]) if j < len(lines) else -1
        while j < len(lines) and lines[j].startswith(";"):
            j += 1
        text = [re.sub(r"(\.Lfunc_end|BB)\d+", r"\1#", l) for l in lines[i:j]]
        syms[m.group(1)] = {"text": text, "len": length}
        i = j
    meta = asm.split("amdhsa.kernels:", 1)
    for block in re.split(r"^  - ", meta[1], flags=re.M)[1:] if len(meta) == 2 else []:
        name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
        if name and name.group(1) in syms:
            for f in FIELDS:
                v = re.search(rf"^\s*{re.escape(f)}:\s+(\S+)", block, re.M)
                syms[name.group(1)][f] = v.group(1) if v else "-"
    return syms


def describe(s):
    return f"{s['len']} B" + "".join(f" {f}={s[f]}" for f in FIELDS if f in s)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--all", action="store_true", help="name the identical symbols too (default: their number per file)")
    args = ap.parse_args()
    jobs = max(1, min(16, args.jobs))
    csrc = [find_csrc(args.tree_a), find_csrc(args.tree_b)]
    sets = [flag_sets(c) for c in csrc]
    for label, tree in (("A", args.tree_a), ("B", args.tree_b)):
        head = subprocess.run(["git", "-C", tree, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "no git checkout"
        dirty = subprocess.run(["git", "-C", tree, "status", "--porcelain", "--", str(csrc[label == "B"])], capture_output=True, text=True).stdout.strip()
        print(f"{label}: {head}{' + uncommitted changes under csrc' if dirty else ''}")
    files = sorted({p.name for c in csrc for p in c.glob("*.hip")})
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        work = {}
        for lib in sets[0]:
            for name in files:
                for t in (0, 1):
                    if (csrc[t] / name).exists():
                        work[lib, name, t] = pool.submit(compile_asm, HIPCC, sets[t][lib], csrc[t] / name, pathlib.Path(tmp) / f"{lib}.{t}.{name}.s")
        total = dict.fromkeys(("identical", "DIFFERS", "MISSING", "NEW"), 0)
        for lib in sets[0]:
            for name in files:
                a, b = (split_symbols(work[lib, name, t].result().read_text()) if (lib, name, t) in work else {} for t in (0, 1))
                same = sum(1 for sym in a if sym in b and a[sym]["text"] == b[sym]["text"])
                print(f"== {lib}  {name}: {len(a)} symbols in A, {len(b)} in B, {same} identical")
                for sym in sorted(set(a) | set(b)):
                    if sym not in b:
                        kind, detail = "MISSING", [f"A: {describe(a[sym])}"]
                    elif sym not in a:
                        kind, detail = "NEW", [f"B: {describe(b[sym])}"]
                    elif a[sym]["text"] == b[sym]["text"]:
                        kind, detail = "identical", []
                    else:
                        kind, detail = "DIFFERS", [f"A: {describe(a[sym])}", f"B: {describe(b[sym])}"]
                    total[kind] += 1
                    if kind == "identical" and not args.all:
                        continue
                    print(f"{kind:9s} {sym}")
                    for d in detail:
                        print(f"            {d}")
        print("== total: " + ", ".join(f"{v} {k}" for k, v in total.items()))


if __name__ == "__main__":
    main()

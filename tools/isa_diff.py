#!/usr/bin/env python3
"""Compare the device code of two sets of sources kernel by kernel (CPU only, no GPU needed).

    python tools/isa_diff.py --parent old/csrc/solve.hip --new ssf-slam_amd/csrc/solve.hip
    python tools/isa_diff.py --parent old.s --new plane_table.s associate.s edges.s solve.s

Each side is one or more .hip sources (compiled to gfx950 assembly with build.py's flags for
that file name, as tools/isa_loop_budget.py does; extra compiler arguments after `--`) or .s
files; the kernels of a side's files are taken together.  Per kernel symbol it prints
`identical` or `differs` with the first differing line, and lists the kernels only one side has.

What is compared, per kernel: its instruction lines with their operands and its block labels,
and the .amdhsa_ lines of its kernel descriptor (registers, LDS, scratch, ...).  Comments, other
directives and metadata are dropped, and local labels (.LBB3_12, ...) are renamed by order of
first appearance inside the kernel, so a kernel that only moved within or between files compares
equal.  It only compares two texts: exit status 0 whatever it finds.
"""
from __future__ import annotations

import argparse
import re
import sys

from isa_loop_budget import compile_to_asm

KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
SYMBOL = re.compile(r"^([A-Za-z_$][\w.$]*):")
LOCAL = re.compile(r"\.L[\w.$]+")


def kernels(asm: str) -> dict:
    """{kernel symbol: normalised lines}: the code from `symbol:` to its .Lfunc_end label, then
    the .amdhsa_ lines of its descriptor."""
    lines = [l.split(";", 1)[0].rstrip() for l in asm.splitlines()]
    names = {m.group(1) for m in map(KERNEL.match, lines) if m}
    out, cur, desc = {}, None, None
    for l in lines:
        k = KERNEL.match(l)
        if k:
            desc = out.setdefault(k.group(1), [])
        elif l.strip() == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            desc.append(" ".join(l.split()))
        s = SYMBOL.match(l)
        if s and s.group(1) in names:
            cur = out.setdefault(s.group(1), [])
            continue
        if cur is None or not l.strip():
            continue
        t = l.strip()
        if t.startswith(".Lfunc_end"):
            cur = None
        elif (t.startswith(".L") and t.endswith(":")) or not t.startswith("."):
            cur.append(" ".join(t.split()))          # a block label or an instruction
    for body in out.values():
        seen = {}
        body[:] = [LOCAL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), l) for l in body]
    return out


def compare(parent: dict, new: dict) -> list:
    """[(symbol, verdict, detail)], verdict one of identical / differs / parent only / new only."""
    rows = []
    for sym in sorted(set(parent) | set(new)):
        if sym not in new or sym not in parent:
            rows.append((sym, "parent only" if sym in parent else "new only", ""))
            continue
        a, b = parent[sym], new[sym]
        if a == b:
            rows.append((sym, "identical", f"{len(a)} lines"))
            continue
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        x, y = (a[i] if i < len(a) else "(end)"), (b[i] if i < len(b) else "(end)")
        rows.append((sym, "differs", f"line {i}: `{x}` -> `{y}`"))
    return rows


def load(paths: list, extra: list) -> dict:
    out = {}
    for p in paths:
        out.update(kernels(open(p).read() if p.endswith(".s") else compile_to_asm(p, extra)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", nargs="+", required=True, metavar="FILE", help=".hip sources or .s files")
    ap.add_argument("--new", nargs="+", required=True, metavar="FILE", help=".hip sources or .s files")
    argv, extra = sys.argv[1:], []
    if "--" in argv:                                   # everything after -- goes to the compiler
        argv, extra = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    a = ap.parse_args(argv)
    rows = compare(load(a.parent, extra), load(a.new, extra))
    print("| kernel | verdict | |\n|---|---|---|")
    for sym, verdict, detail in rows:
        print(f"| `{sym}` | {verdict} | {detail} |")
    n = sum(v == "identical" for _, v, _ in rows)
    print(f"\n{n} of {len(rows)} kernels identical")


if __name__ == "__main__":
    main()

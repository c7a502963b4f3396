#!/usr/bin/env python3
"""Instruction budget of one basic block of a kernel (CPU only, no GPU needed).

    python tools/isa_loop_budget.py ssf-slam_amd/csrc/mask_pose.hip --kernel k_mask_poseIfE \
        --has v_rcp_f64 v_frexp_mant_f64

Compiles a .hip source to gfx950 assembly with build.py's flags for that file (FLAGS plus its
FILE_FLAGS entry; extra compiler arguments after `--`), or reads a .s file, finds the basic
block(s) of the named kernel that contain every mnemonic given with --has, and prints how many
instructions of each class the block holds.  Classes come from the mnemonic's prefix alone:

    v_*f64   other v_   ds_   global_load   scratch_   s_waitcnt   other

It only counts: it asserts nothing about the code.  --mnemonics adds the per-mnemonic histogram.
"""
from __future__ import annotations

import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ssf-slam_amd")

CLASSES = ["v_*f64", "other v_", "ds_", "global_load", "scratch_", "s_waitcnt", "other"]
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
MNEMONIC = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def classify(m: str) -> str:
    if m.startswith("v_"):
        return "v_*f64" if "f64" in m else "other v_"
    for p in ("ds_", "global_load", "scratch_", "s_waitcnt"):
        if m.startswith(p):
            return p
    return "other"


def compile_to_asm(src: str, extra: list) -> str:
    sys.path.insert(0, PKG)
    import build as B

    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    flags = [f for f in B.FLAGS if f != "-fPIC"] + B.FILE_FLAGS.get(os.path.basename(src), [])
    cmd = [B.HIPCC, *flags, *extra, "-S", "--cuda-device-only", src, "-o", out]
    print("# " + " ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    text = open(out).read()
    os.unlink(out)
    return text


def kernel_blocks(asm: str, kernel: str):
    """[(label, [mnemonics])] of the first function whose symbol contains `kernel`.  A block
    starts at a label and ends at the next label or after a branch."""
    blocks, cur, inside, name = [], None, False, None
    for line in asm.splitlines():
        lab = LABEL.match(line)
        if lab:
            sym = lab.group(1)
            if not inside:
                if kernel in sym and not sym.startswith("."):
                    inside, name = True, sym
                    cur = (sym, [])
                    blocks.append(cur)
                continue
            if sym.startswith(".Lfunc_end"):
                break
            cur = (sym, [])
            blocks.append(cur)
            continue
        if not inside:
            continue
        m = MNEMONIC.match(line)
        if not m:
            continue
        if cur is None:
            cur = ("(after branch)", [])
            blocks.append(cur)
        cur[1].append(m.group(1))
        if m.group(1).startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")):
            cur = None
    return name, blocks


def report(label, mns, mnemonics):
    cnt = collections.Counter(classify(m) for m in mns)
    print(f"block {label}: {len(mns)} instructions, {cnt['v_*f64'] + cnt['other v_']} VALU")
    print("| class | count |\n|---|---|")
    for c in CLASSES:
        print(f"| `{c}` | {cnt[c]} |")
    if mnemonics:
        print("\n| mnemonic | count |\n|---|---|")
        for m, k in collections.Counter(mns).most_common():
            print(f"| `{m}` | {k} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help=".hip source (compiled with build.py's flags) or .s assembly")
    ap.add_argument("--kernel", required=True, help="substring of the kernel's (mangled) symbol")
    ap.add_argument("--has", nargs="+", required=True, metavar="MNEMONIC",
                    help="mnemonic prefixes the block must all contain")
    ap.add_argument("--mnemonics", action="store_true", help="also print the per-mnemonic histogram")
    ap.add_argument("--all", action="store_true", help="print every matching block, not the largest")
    argv, extra = sys.argv[1:], []
    if "--" in argv:                                   # everything after -- goes to the compiler
        argv, extra = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    a = ap.parse_args(argv)
    asm = open(a.source).read() if a.source.endswith(".s") else compile_to_asm(a.source, extra)
    name, blocks = kernel_blocks(asm, a.kernel)
    if name is None:
        sys.exit(f"no function symbol contains {a.kernel!r}")
    hits = [(l, m) for l, m in blocks if all(any(x.startswith(p) for x in m) for p in a.has)]
    if not hits:
        sys.exit(f"{name}: no basic block holds all of {a.has}")
    hits.sort(key=lambda b: -len(b[1]))
    print(f"kernel {name}: {len(blocks)} blocks, {len(hits)} with {' + '.join(a.has)}")
    for l, m in (hits if a.all else hits[:1]):
        report(l, m, a.mnemonics)


if __name__ == "__main__":
    main()

"""tools/isa_diff.py on three hand-written assembly listings (no compiler, no GPU): renumbered
labels compare identical, a changed operand or descriptor figure differs, a missing kernel is
reported."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "isa_diff.py")


def _kernel(sym, fn, label0, operand="v0", vgprs=8):
    """One kernel as the compiler prints it: function number fn in its labels, a loop, a
    descriptor."""
    return f"""\
\t.text
\t.globl\t{sym}
{sym}:                      ; @{sym}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_cbranch_scc1 .LBB{fn}_{label0 + 1}
.LBB{fn}_{label0}:                                ; =>This Inner Loop Header
\tv_add_u32_e32 {operand}, 12, v0          ; a comment
\ts_cbranch_vccnz .LBB{fn}_{label0}
.LBB{fn}_{label0 + 1}:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {sym}
\t\t.amdhsa_group_segment_fixed_size 1024
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
\t.size\t{sym}, .Lfunc_end{fn}-{sym}
; NumVgprs: {vgprs}
"""


PARENT = _kernel("_Z3k_aPf", 0, 1) + _kernel("_Z3k_bPf", 1, 1) + _kernel("_Z3k_cPf", 2, 1) + _kernel("_Z3k_dPf", 3, 1)
# k_a moved behind k_b (other function number, other label numbers), k_b with another operand,
# k_d with another register count, k_c gone, k_e new
NEW_1 = _kernel("_Z3k_bPf", 0, 1, operand="v1") + _kernel("_Z3k_aPf", 1, 4)
NEW_2 = _kernel("_Z3k_dPf", 0, 1, vgprs=9) + _kernel("_Z3k_ePf", 1, 1)


def _run(tmp_path):
    for name, text in (("parent.s", PARENT), ("new1.s", NEW_1), ("new2.s", NEW_2)):
        (tmp_path / name).write_text(text)
    r = subprocess.run([sys.executable, TOOL, "--parent", str(tmp_path / "parent.s"), "--new",
                        str(tmp_path / "new1.s"), str(tmp_path / "new2.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {l.split("|")[1].strip(" `"): [c.strip() for c in l.split("|")[2:4]]
            for l in r.stdout.splitlines() if l.startswith("| `")}, r.stdout


def test_renumbered_labels_are_identical(tmp_path):
    rows, out = _run(tmp_path)
    assert rows["_Z3k_aPf"][0] == "identical", out
    assert "1 of 5 kernels identical" in out


def test_changed_operand_and_descriptor_differ(tmp_path):
    rows, out = _run(tmp_path)
    assert rows["_Z3k_bPf"][0] == "differs", out
    assert "`v_add_u32_e32 v0, 12, v0` -> `v_add_u32_e32 v1, 12, v0`" in rows["_Z3k_bPf"][1]
    assert rows["_Z3k_dPf"][0] == "differs", out
    assert "`.amdhsa_next_free_vgpr 8` -> `.amdhsa_next_free_vgpr 9`" in rows["_Z3k_dPf"][1]


def test_missing_and_added_kernels_are_reported(tmp_path):
    rows, out = _run(tmp_path)
    assert rows["_Z3k_cPf"][0] == "parent only", out
    assert rows["_Z3k_ePf"][0] == "new only", out

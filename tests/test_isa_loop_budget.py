"""tools/isa_loop_budget.py on a hand-written assembly listing (no compiler, no GPU): block
splitting at labels and branches, kernel selection by symbol substring, prefix classes."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "isa_loop_budget.py")

ASM = """\
\t.text
_Z5otherv:
\tv_rcp_f64_e32 v[0:1], v[2:3]
\ts_endpgm
.Lfunc_end0:
_Z6kernelIfEvPKT_:                      ; @kernel
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\ts_cbranch_scc1 .LBB1_3
.LBB1_1:                                ; =>This Inner Loop Header
\tglobal_load_dwordx3 v[4:6], v0, s[0:1]
\tscratch_load_dwordx2 v[8:9], off, off offset:16
\tds_read2_b64 v[10:13], v1 offset1:1
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tv_cvt_f64_f32_e32 v[14:15], v4
\tv_fma_f64 v[16:17], v[14:15], v[10:11], v[12:13]
\tv_rcp_f64_e32 v[18:19], v[16:17]
\tv_add_u32_e32 v0, 12, v0
\tv_cmp_gt_u32_e32 vcc, s2, v0
\ts_cbranch_vccnz .LBB1_1
; %bb.2:
\tv_rcp_f64_e32 v[18:19], v[16:17]
.LBB1_3:
\ts_endpgm
.Lfunc_end1:
"""


def _run(tmp_path, *args):
    src = tmp_path / "k.s"
    src.write_text(ASM)
    r = subprocess.run([sys.executable, TOOL, str(src), *args], capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


def test_counts_the_block_with_both_mnemonics(tmp_path):
    rc, out = _run(tmp_path, "--kernel", "kernelIfE", "--has", "v_rcp_f64", "global_load")
    assert rc == 0, out
    assert "1 with v_rcp_f64 + global_load" in out
    assert "block .LBB1_1: 10 instructions, 5 VALU" in out
    for line in ("| `v_*f64` | 3 |", "| `other v_` | 2 |", "| `ds_` | 1 |", "| `global_load` | 1 |",
                 "| `scratch_` | 1 |", "| `s_waitcnt` | 1 |", "| `other` | 1 |"):
        assert line in out, (line, out)


def test_other_functions_and_missing_blocks(tmp_path):
    rc, out = _run(tmp_path, "--kernel", "kernelIfE", "--has", "v_rcp_f64", "--all")
    assert rc == 0 and "2 with v_rcp_f64" in out          # the loop and the block after it, not _Z5otherv
    rc, out = _run(tmp_path, "--kernel", "kernelIfE", "--has", "v_sqrt_f64")
    assert rc != 0 and "no basic block" in out
    rc, out = _run(tmp_path, "--kernel", "absent", "--has", "v_rcp_f64")
    assert rc != 0 and "no function symbol" in out

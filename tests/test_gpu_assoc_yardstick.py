"""The plane association on the device (k_associate_strips in all its modes, the brute
k_associate) against registration_reference.associate_exact, the all-pairs float64 yardstick, on
the seeded cases of tests/assoc_cases.py: search radii 2 .. 4096 m and the unbounded pass, a
masked hole, points on the strip boundaries, empty strips, degenerate and 30 km extents, a far
origin, exact ties.

Every family goes through every launch shape of assoc_cases.rows() -- group mode with its own
float4 strips, with the plane table's strip image and with SoA strips; lane mode split over two
work-groups per pair, compacted, and SoA; brute force -- each named by ssf.register_plan before
the launch (the plan does not say whether a strip image was staged: the image row asserts that
the table made one for a launch and frames of the imaged sizes, no more).  The global-memory
walk takes the densified hole in group and in lane mode, and 129 pairs (every case tiled) take
the compacted lane mode.  Asserted per pair: nn element for element,
ncorr = the yardstick's kept records, and -- for the cases within 300 m of the origin whose
one-step Jacobian has sv_ratio >= 1e-3 in the yardstick's run -- the logged pose and the final
pose of ONE Gauss-Newton step within TOL_T / TOL_R of solve_gn on the yardstick's own records
(the records' content).  Every case runs once more alone and must give the same nn.
"""
import numpy as np
import pytest

import assoc_cases as ac
import registration_cases as rc
import registration_reference as ref
from test_gpu_solve_yardstick import _launch

pytestmark = pytest.mark.gpu

WORST = dict(dt=0.0, dr=0.0)


def _check_pair(cs, res, p):
    y = ac.yardstick(cs)
    o = res["curr_off"][p]
    got = res["nn"][o:o + len(cs.curr)]
    bad = np.flatnonzero(got != y["nn"])
    assert len(bad) == 0, (cs.name, p, len(bad), bad[:8], got[bad[:8]], y["nn"][bad[:8]])
    assert int(res["ncorr"][p]) == int(y["keep"].sum()), (cs.name, p)
    if ac.solve_compared(cs):
        return
    sol = y["sol"]
    assert int(res["nlog"][p]) == len(sol["log"]) == 1, (cs.name, p)
    row, pose = res["log"][p, 0], res["pose_rel"][p]
    assert int(row[8]) == int(sol["log"][0, 8]) == ref.GN_STEP, (cs.name, p)
    for q, t in ((row[:4], row[4:7]), (pose[:4], pose[4:])):
        dt, dr = float(np.abs(t - sol["t"]).max()), ref.quat_angle(q, sol["q"])
        WORST["dt"], WORST["dr"] = max(WORST["dt"], dt), max(WORST["dr"], dr)
        assert dt < rc.TOL_T and dr < rc.TOL_R, (cs.name, p, dt, dr)


def _run_row(dev, name, row, cases, mode, bound, want):
    import ssf
    b = ac.bound_of(cases, bound)
    ac.check_plan(ssf.register_plan(len(cases), b), want, (name, row))
    res = _launch(dev, cases, mode, b)
    if row == "group_image":
        assert res["strip_image"] and any(ac.IMAGE_MIN <= len(c.last) <= ac.IMAGE_MAX for c in cases), (name, row)
    if row == "group_f4_own":
        assert not res["strip_image"], (name, row)
    for p, cs in enumerate(cases):
        _check_pair(cs, res, p)


def _report(capsys, what):
    with capsys.disabled():
        print(f"\n  {what}: worst one-step gaps so far: dt {WORST['dt']:.3g} m, dr {WORST['dr']:.3g} rad")


@pytest.mark.parametrize("name", ac.FAMILIES)
def test_family_through_every_path(dev, name, capsys):
    for row, cases, mode, bound, want in ac.rows(name):
        _run_row(dev, name, row, cases, mode, bound, want)
    skipped = [f"{c.name} ({ac.solve_compared(c)})" for c in ac.family(name, big=True) if ac.solve_compared(c)]
    _report(capsys, f"{name}, solve not compared: {skipped or 'none'}")


def test_global_memory_walk(dev, capsys):
    """a last frame one point above the LDS staging capacity, in group and in lane mode"""
    for row, cases, mode, bound, want in ac.global_rows():
        assert len(cases[0].last) > want["lds_cap"]
        _run_row(dev, "global", row, cases, mode, bound, want)
    _report(capsys, "global walk")


def test_129_pairs_compacted(dev, capsys):
    """every case, tiled to 129 pairs, through the lane mode that hands the solve compacted records"""
    cases = ac.tile(list(ac.cases()), 129)
    _run_row(dev, "all", "lane_compacted", cases, "sorted", 1024,
             dict(strip_path=True, group_mode=False, qsplit=1, compacted=True))
    _report(capsys, "129 pairs")


def test_every_case_alone(dev):
    """one-pair launches: the same nn as in company"""
    for cs in ac.cases() + (ac.hole_big(),):
        res = _launch(dev, [cs], "sorted")
        _check_pair(cs, res, 0)

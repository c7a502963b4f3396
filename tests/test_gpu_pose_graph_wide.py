"""GPU pose-graph optimisation of graphs with more than 32 loop edges (k_pose_graph_wide,
pose_graph.hip) against the dense numpy Gauss-Newton of tests/pgo_reference.py.

The bars are those of test_gpu_pose_graph.py: poses within 1e-5 m and 1e-6 rad, initial cost
within 1e-9 relative, final cost within 1e-6 relative plus pgo_reference.cost_floor; absolute
poses under the tight prior, poses relative to node 0 under the reference's prior.  The graphs
are those of tests/pgo_wide_fixtures.py: the ones whose every stop check is clear run at the
default parameters and must take the yardstick's iteration count; the rest run three steps in
fixed-iteration mode."""
import math

import numpy as np
import pytest
import torch

import pgo_reference as R
import pgo_wide_fixtures as W

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL = 1e-5, 1e-6
GOOD = (R.OK, R.CONVERGED)
KEYS = ("poses", "edge_ij", "edge_meas", "edge_var", "prior_pose", "prior_var")


@pytest.fixture(scope="module")
def fe(dev):
    from ssf import Frontend
    return Frontend(64, device=dev)


def _solve(fe, graphs, **kw):
    from ssf import loop
    return loop.optimize_pose_graphs(fe, [{k: g[k] for k in KEYS} for g in graphs],
                                     loop.pgo_params(**kw) if kw else None)


def _check_against_reference(name, g, got, ref, relative):
    floor = R.cost_floor(g)
    print(f"{name}: status {got['status_name']} it {got['iterations']} (ref {ref['iterations']}) "
          f"cost0 {got['cost0']:.17g} (ref {ref['cost0']:.17g}) cost {got['cost']:.17g} (ref {ref['cost']:.17g}) "
          f"floor {floor:.3g}")
    assert got["status"] in GOOD
    a, b = (R.relative_to_first(got["poses"]), R.relative_to_first(ref["poses"])) if relative else \
        (got["poses"], ref["poses"])
    dt, dr = R.pose_errors(a, b)
    print(f"{name}: pose error {dt:.3g} m {dr:.3g} rad ({'relative to node 0' if relative else 'absolute'})")
    assert dt <= POS_TOL and dr <= ROT_TOL
    assert abs(got["cost0"] - ref["cost0"]) <= 1e-9 * ref["cost0"] + floor
    assert abs(got["cost"] - ref["cost"]) <= 1e-6 * ref["cost"] + floor
    assert got["loops"] == W.true_loops(g)
    assert len(got["cost_log"]) == got["iterations"] + 1
    assert got["cost_log"][0] == got["cost0"] and got["cost_log"][-1] == got["cost"]


@pytest.mark.parametrize("prior", ["tight", "ref"])
@pytest.mark.parametrize("name", list(W.WIDE))
def test_wide_graph_against_reference(fe, name, prior):
    g, ref = W.wide_fixture(name, prior)
    assert W.extra_edges(g) > W.NARROW_LOOPS                 # the host sends it down the wide path
    got = _solve(fe, [g], **W.solve_params(name))[0]
    _check_against_reference(name, g, got, ref, relative=prior == "ref")
    if name in W.WIDE_STOP_RULE:
        print(name, got["cost_log"], ref["cost_log"])
        assert got["status"] == ref["status"] == R.CONVERGED
        assert got["iterations"] == ref["iterations"]
    else:
        assert got["iterations"] == W.FIXED_ITERATIONS == ref["iterations"] and got["status"] == R.OK


def _cut_graph():
    """(40, 40) with chain link 8 - 9 removed: still 39 edges beyond K - 1, so the wide path"""
    g = R.circle_graph(40, loops=R.spread_loops(40, 40, 35), seed=35)
    keep = [e for e, (i, j) in enumerate(g["edge_ij"]) if {int(i), int(j)} != {8, 9}]
    assert len(keep) == len(g["edge_ij"]) - 1
    for k in ("edge_ij", "edge_meas", "edge_var"):
        g[k] = g[k][keep]
    return g


def test_wide_failure_statuses_leave_poses_bitwise(fe):
    cut = _cut_graph()
    nan = R.copy_graph(cut)
    nan["edge_meas"][50, 5] = math.nan
    for name, g, want in (("missing_link", cut, R.NOT_PD), ("nan_measurement", nan, R.BAD_INPUT)):
        assert W.extra_edges(g) > W.NARROW_LOOPS
        got = _solve(fe, [g])[0]
        assert got["status"] == want, (name, got["status_name"])
        assert got["poses"].tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes(), name
        assert got["iterations"] == 0, name


def test_too_many_loops_reports_the_count(fe):
    from ssf import _abi
    g = R.circle_graph(40, loops=R.spread_loops(40, _abi.PGO_MAX_LOOPS + 1, 11), seed=11)
    got = _solve(fe, [g])[0]
    assert got["status"] == R.TOO_MANY_LOOPS and got["loops"] == _abi.PGO_MAX_LOOPS + 1 == 257
    assert got["iterations"] == 0
    assert got["poses"].tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes()


def _same(ra, rb):
    for key in ("status", "iterations", "cost0", "cost", "dx", "loops", "cost_log"):
        if not (ra[key] == rb[key] or (isinstance(ra[key], float) and math.isnan(ra[key]) and math.isnan(rb[key]))):
            return key
    return None if ra["poses"].tobytes() == rb["poses"].tobytes() else "poses"


def test_mixed_batch_isolation_and_determinism(fe):
    bad = R.copy_graph(R.fixture("k12_l3")[0])
    bad["edge_meas"][2, 0] = math.nan
    graphs = [R.fixture("k65_l11")[0], W.wide_fixture("k40_l43")[0], R.circle_graph(0), bad,
              W.wide_fixture("k60_l171")[0], R.fixture("k40_l32", "ref")[0], W.wide_fixture("k40_l256")[0]]
    a = _solve(fe, graphs)
    b = _solve(fe, graphs)
    assert [r["status"] for r in a][2:4] == [R.EMPTY, R.BAD_INPUT]
    for k, (g, ra, rb) in enumerate(zip(graphs, a, b)):
        assert _same(ra, rb) is None, (k, _same(ra, rb))
        if k in (2, 3):
            assert ra["poses"].tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes()
            continue
        one = _solve(fe, [g])[0]
        assert one["status"] in GOOD, k
        assert _same(ra, one) is None, (k, _same(ra, one))
    # the narrow graphs: the bits they have in a batch without wide graphs
    narrow = [0, 2, 3, 5]
    c = _solve(fe, [graphs[k] for k in narrow])
    for k, rc in zip(narrow, c):
        assert _same(a[k], rc) is None, (k, _same(a[k], rc))


# ------------------------------------------------------------------------- LoopCloser(optimize=True)
def _two_laps(n=80, step=2.0, per=10):
    """ground truth twice round a closed square (10 keyframes a side: keyframe k revisits k - 40)
    and a drifting odometry of it"""
    from ssf import loop
    gt, od = [], []
    x = y = 0.0
    for k in range(n):
        yaw = (k // per) * math.pi / 2
        gt.append(loop.get_transformation(x, y, 0.0, 0.0, 0.0, yaw))
        x += step * math.cos(yaw)
        y += step * math.sin(yaw)
    od.append(gt[0].copy())
    for k in range(1, n):                                   # yaw bias and a scale error per step
        d = np.linalg.inv(gt[k - 1]) @ gt[k]
        d = d @ loop.get_transformation(0.01, 0.0, 0.002, 0.0, 0.0005, 0.004)
        od.append(od[-1] @ d)
    return gt, od


def _drive_laps(fe, optimize, gt, od, lap=40):
    """every odometry pose through LoopCloser.process; every keyframe k >= lap + 1 closes a
    hand-built loop to k - lap (add_loop_factor replaced: what a perfect ICP would return).
    -> (closer, statuses of every closure, the graph as it stood before the last loop edge,
    the last constraint)"""
    from ssf import loop
    lc = loop.LoopCloser(fe, optimize=True) if optimize else loop.LoopCloser(fe)
    plane = torch.zeros(8, 4, device=fe.device)
    n = len(od)
    seen = {}

    def constraint():
        cur = len(lc.key6d) - 1
        if cur < lap + 1:
            return None
        pre = cur - lap
        corr = gt[cur] @ np.linalg.inv(lc._T6(cur))
        pose_from = loop.get_transformation(*loop.get_translation_and_euler_angles(corr @ lc._T6(cur)))
        c = loop.LoopConstraint(cur, pre, loop.between(pose_from, lc._T6(pre)), 0.05, corr)
        if cur == n - 1 and optimize:
            seen["graph"], seen["last"] = lc.pose_graph(), c
        return c

    lc.add_loop_factor = constraint
    statuses = []
    for k, T in enumerate(od):
        p = loop.pose7_from_matrix(T)
        out = lc.process(plane, p[:4], p[4:], 0.1 * k)
        assert out[2]                                       # every frame is a keyframe
        if out[1] is not None and optimize:
            statuses.append(lc.last_optimization["status"])
            assert lc.last_optimization["loops"] == len(statuses)
    return lc, statuses, seen.get("graph"), seen.get("last")


def test_loop_closer_passes_the_33rd_loop(fe):
    from ssf import loop
    gt, od = _two_laps()
    n = len(od)
    lc, statuses, g, last = _drive_laps(fe, True, gt, od)
    assert len(statuses) == 39 and all(s in GOOD for s in statuses), statuses
    assert lc.last_optimization["loops"] == 39 and len(lc.graph_edges) == n - 1 + 39
    # the last solve against the yardstick: the graph before the last loop edge, plus that edge
    assert len(g["edge_ij"]) == n - 1 + 38 and len(g["poses"]) == n
    g["edge_ij"] = np.concatenate([g["edge_ij"], [[last.key_cur, last.key_pre]]]).astype(np.int32)
    g["edge_meas"] = np.concatenate([g["edge_meas"], [loop.pose7_from_matrix(last.between)]])
    g["edge_var"] = np.concatenate([g["edge_var"], [[last.noise] * 6]])
    ref = R.solve(g)
    opt = lc.last_optimization
    print(f"yardstick: iterations {ref['iterations']} margins {R.stop_margins(ref['cost_log'])}; "
          f"device: iterations {opt['iterations']} cost_log {opt['cost_log']}")
    dt, dr = R.pose_errors(R.relative_to_first(opt["poses"]), R.relative_to_first(ref["poses"]))
    print(f"last solve vs reference: {dt:.3g} m {dr:.3g} rad")
    assert dt <= POS_TOL and dr <= ROT_TOL
    floor = R.cost_floor(g)
    assert abs(opt["cost0"] - ref["cost0"]) <= 1e-9 * ref["cost0"] + floor
    assert abs(opt["cost"] - ref["cost"]) <= 1e-6 * ref["cost"] + floor
    for i, p in enumerate(opt["poses"]):
        v = loop.get_translation_and_euler_angles(loop.pose_from_quat(p[:4], p[4:]))
        assert lc.key6d[i][:6] == np.array(v, np.float32).tolist(), i

    off, _, _, _ = _drive_laps(fe, False, gt, od)
    assert off.last_optimization is None and not off.graph_edges and not off.graph_init

    def error(key6d, k):                                    # of node k relative to node 0
        rel = np.linalg.inv(loop.get_transformation(*key6d[0][:6])) @ loop.get_transformation(*key6d[k][:6])
        return float(np.linalg.norm((rel - np.linalg.inv(gt[0]) @ gt[k])[:3, 3]))
    print(f"end-point error {error(off.key6d, n - 1):.4f} -> {error(lc.key6d, n - 1):.4f} m, "
          f"mid-point {error(off.key6d, n // 2):.4f} -> {error(lc.key6d, n // 2):.4f} m")
    assert error(lc.key6d, n - 1) < error(off.key6d, n - 1)
    assert error(lc.key6d, n // 2) < error(off.key6d, n // 2)

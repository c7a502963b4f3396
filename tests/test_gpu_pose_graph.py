"""GPU pose-graph optimisation (ssf_pose_graph_batch, pose_graph.hip; runOptimize /
correctPoses of src/mapOptmization.cpp:280-332) against the dense numpy Gauss-Newton of
tests/pgo_reference.py (same residual, Jacobians, retraction and stop rule; np.linalg.solve).

Bars: poses within 1e-5 m and 1e-6 rad; initial cost within 1e-9 relative (evaluation only);
final cost within 1e-6 relative.  A cost that f64 rounding alone can produce
(pgo_reference.cost_floor) counts as zero on both sides.  Under the reference's prior
(translation variance 1e8) the global position is numerically free (cond(H) ~ 1e16), so those
cases compare poses relative to node 0; absolute comparisons use a prior with every variance
1e-4."""
import math

import numpy as np
import pytest
import torch

import pgo_reference as R

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


def _check_against_reference(g, got, ref, relative):
    floor = R.cost_floor(g)
    print(f"status {got['status_name']} it {got['iterations']} (ref {ref['iterations']}) cost0 {got['cost0']:.17g} "
          f"(ref {ref['cost0']:.17g}) cost {got['cost']:.17g} (ref {ref['cost']:.17g}) floor {floor:.3g}")
    assert got["status"] in GOOD
    a, b = (R.relative_to_first(got["poses"]), R.relative_to_first(ref["poses"])) if relative else \
        (got["poses"], ref["poses"])
    dt, dr = R.pose_errors(a, b)
    print(f"pose error {dt:.3g} m {dr:.3g} rad")
    assert dt <= POS_TOL and dr <= ROT_TOL
    assert abs(got["cost0"] - ref["cost0"]) <= 1e-9 * ref["cost0"] + floor
    assert abs(got["cost"] - ref["cost"]) <= 1e-6 * ref["cost"] + floor
    assert got["loops"] == sum(1 for i, j in g["edge_ij"] if abs(int(i) - int(j)) != 1)
    assert len(got["cost_log"]) == got["iterations"] + 1
    assert got["cost_log"][0] == got["cost0"] and got["cost_log"][-1] == got["cost"]


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_tight_prior_absolute(fe, name):
    g, ref = R.fixture(name, "tight")
    got = _solve(fe, [g])[0]
    _check_against_reference(g, got, ref, relative=False)
    if name == "k1":                       # nothing to move: the pose stays, the cost is zero
        dt, dr = R.pose_errors(got["poses"], g["poses"])
        assert dt <= POS_TOL and dr <= ROT_TOL and got["cost"] <= R.cost_floor(g)


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_reference_prior_relative_to_node0(fe, name):
    g, ref = R.fixture(name, "ref")
    yaw = [math.atan2(2 * (p[3] * p[2] + p[0] * p[1]), 1 - 2 * (p[1] ** 2 + p[2] ** 2)) for p in g["poses"]]
    if len(yaw) >= 5:                      # a full circle: the yaw wraps through +-pi on the way
        assert any(abs(a - b) > math.pi for a, b in zip(yaw[:-1], yaw[1:]))
    _check_against_reference(g, _solve(fe, [g])[0], ref, relative=True)


def test_fixed_iteration_mode(fe):
    for name in ("k5_l1", "k65_l11"):
        g, _ = R.fixture(name)
        ref = R.solve(g, max_iter=3, func_tol=0.0)
        got = _solve(fe, [g], max_iter=3, func_tol=0.0)[0]
        assert got["iterations"] == 3 == ref["iterations"] and got["status"] == R.OK
        _check_against_reference(g, got, ref, relative=False)
    g, _ = R.fixture("k12_l3")
    got = _solve(fe, [g], max_iter=0)[0]                   # evaluation only
    assert got["iterations"] == 0 and got["status"] == R.OK and got["cost"] == got["cost0"]
    assert np.array_equal(got["poses"][:, 4:], g["poses"][:, 4:])


@pytest.mark.parametrize("prior", ["tight", "ref"])
def test_default_stop_rule_iteration_count(fe, prior):
    for name in R.STOP_RULE_FIXTURES:
        g, ref = R.fixture(name, prior)
        margins = R.stop_margins(ref["cost_log"])
        assert all(m >= 100 or m <= 0.01 for m in margins), (name, margins)
        got = _solve(fe, [g])[0]
        print(name, got["iterations"], ref["iterations"], got["cost_log"], ref["cost_log"])
        assert got["status"] == ref["status"] == R.CONVERGED
        assert got["iterations"] == ref["iterations"]


def _failure_cases():
    from ssf import _abi
    base, _ = R.fixture("k12_l3")
    too_many = R.circle_graph(40, loops=R.spread_loops(40, _abi.PGO_MAX_LOOPS + 1, 11), seed=11)
    idx = R.copy_graph(base); idx["edge_ij"][4] = (4, 12)
    neg = R.copy_graph(base); neg["edge_ij"][0] = (-1, 0)
    same = R.copy_graph(base); same["edge_ij"][6] = (6, 6)
    zvar = R.copy_graph(base); zvar["edge_var"][3, 2] = 0.0
    nvar = R.copy_graph(base); nvar["prior_var"][5] = -1.0
    nan = R.copy_graph(base); nan["edge_meas"][7, 5] = math.nan
    infp = R.copy_graph(base); infp["poses"][9, 4] = math.inf
    empty = R.circle_graph(0)
    cut = R.copy_graph(base)                                # link 8 -> 9 missing: T is singular
    keep = [e for e, (i, j) in enumerate(cut["edge_ij"]) if {int(i), int(j)} != {8, 9}]
    for k in ("edge_ij", "edge_meas", "edge_var"):
        cut[k] = cut[k][keep]
    return [("too_many_loops", too_many, R.TOO_MANY_LOOPS), ("index_eq_K", idx, R.BAD_INPUT),
            ("index_negative", neg, R.BAD_INPUT), ("i_eq_j", same, R.BAD_INPUT),
            ("zero_variance", zvar, R.BAD_INPUT), ("negative_prior_variance", nvar, R.BAD_INPUT),
            ("nan_measurement", nan, R.BAD_INPUT), ("inf_pose", infp, R.BAD_INPUT), ("K0", empty, R.EMPTY),
            ("missing_link", cut, R.NOT_PD)]


def test_failure_statuses_leave_poses_bitwise(fe):
    for name, g, want in _failure_cases():
        got = _solve(fe, [g])[0]
        assert got["status"] == want, (name, got["status_name"])
        assert got["poses"].tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes(), name
        assert got["iterations"] == 0, name


def test_batch_isolation_and_determinism(fe):
    bad = R.copy_graph(R.fixture("k12_l3")[0])
    bad["edge_meas"][2, 0] = math.nan
    graphs = [R.fixture("k65_l11")[0], R.fixture("k5_l1", "ref")[0], R.circle_graph(0), bad,
              R.fixture("k130_l1")[0], R.fixture("k1")[0], R.fixture("k40_l32", "ref")[0]]
    assert len(graphs) == 7
    a = _solve(fe, graphs)
    b = _solve(fe, graphs)
    assert [r["status"] for r in a][2:4] == [R.EMPTY, R.BAD_INPUT]
    for k, (g, ra, rb) in enumerate(zip(graphs, a, b)):
        for key in ("status", "iterations", "cost0", "cost", "dx", "loops", "cost_log"):
            assert ra[key] == rb[key] or (isinstance(ra[key], float) and math.isnan(ra[key]) and math.isnan(rb[key])), (k, key)
        assert ra["poses"].tobytes() == rb["poses"].tobytes(), k
        if k in (2, 3):
            assert ra["poses"].tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes()
            continue
        one = _solve(fe, [g])[0]
        assert one["status"] in GOOD and ra["status"] == one["status"], k
        assert ra["poses"].tobytes() == one["poses"].tobytes(), k
        assert (ra["iterations"], ra["cost0"], ra["cost"], ra["cost_log"]) == \
            (one["iterations"], one["cost0"], one["cost"], one["cost_log"]), k


# ------------------------------------------------------------------------- LoopCloser(optimize=True)
def _square(n=40, step=2.0):
    """ground truth on a closed square (10 keyframes a side) and a drifting odometry of it"""
    from ssf import loop
    gt, od = [], []
    x = y = 0.0
    per = n // 4
    for k in range(n):
        side = k // per
        yaw = side * math.pi / 2
        gt.append(loop.get_transformation(x, y, 0.0, 0.0, 0.0, yaw))
        x += step * math.cos(yaw)
        y += step * math.sin(yaw)
    od.append(gt[0].copy())
    for k in range(1, n):                                   # yaw bias and a scale error per step
        d = np.linalg.inv(gt[k - 1]) @ gt[k]
        d = d @ loop.get_transformation(0.01, 0.0, 0.002, 0.0, 0.0005, 0.004)
        od.append(od[-1] @ d)
    return gt, od


def _drive(fe, optimize, gt, od, constraint_for):
    """every odometry pose through LoopCloser.process; the last keyframe closes a hand-built loop
    (add_loop_factor replaced: no ICP)"""
    from ssf import loop
    lc = loop.LoopCloser(fe, optimize=True) if optimize else loop.LoopCloser(fe)
    plane = torch.zeros(8, 4, device=fe.device)
    n = len(od)
    lc.add_loop_factor = lambda: constraint_for(lc) if len(lc.key6d) == n else None
    out = None
    for k, T in enumerate(od):
        p = loop.pose7_from_matrix(T)
        out = lc.process(plane, p[:4], p[4:], 0.1 * k)
        assert out[2]                                       # every frame is a keyframe
    return lc, out


def test_loop_closer_optimize_rewrites_key_poses(fe):
    from ssf import loop
    gt, od = _square()
    n = len(od)
    six = [loop.get_translation_and_euler_angles(loop.pose_from_quat(*np.split(loop.pose7_from_matrix(T), [4])))
           for T in od]
    before = [np.array(v, np.float32).tolist() for v in six]      # the key poses as first stored

    def constraint_for(lc):
        cur, pre = n - 1, 0
        assert [v[:6] for v in lc.key6d] == before          # nothing rewritten before the loop
        corr = gt[cur] @ np.linalg.inv(lc._T6(cur))         # what a perfect ICP would return
        pose_from = loop.get_transformation(*loop.get_translation_and_euler_angles(corr @ lc._T6(cur)))
        return loop.LoopConstraint(cur, pre, loop.between(pose_from, lc._T6(pre)), 0.05, corr)

    lc, (T, c, _) = _drive(fe, True, gt, od, constraint_for)
    assert c is not None and lc.last_optimization["status"] in GOOD
    assert len(lc.graph_edges) == n and lc.last_optimization["loops"] == 1
    # the recorded graph as it stood when the loop closed: the estimates are the double poses
    # of addOdomFactor (the solve has since overwritten them with the solution)
    g = lc.pose_graph()
    g["poses"] = np.array([loop.pose7_from_matrix(loop.get_transformation(*v)) for v in six])
    assert np.array_equal(g["edge_ij"][:-1], np.stack([np.arange(n - 1), np.arange(1, n)], 1))
    assert tuple(g["edge_ij"][-1]) == (n - 1, 0) and np.allclose(g["edge_var"][-1], 0.05)
    assert np.allclose(g["prior_var"], R.REF_PRIOR_VAR) and np.allclose(g["edge_var"][0], R.ODOM_VAR)
    ref = R.solve(g)
    assert all(m >= 100 or m <= 0.01 for m in R.stop_margins(ref["cost_log"]))   # a clear stop
    dt, dr = R.pose_errors(R.relative_to_first(lc.last_optimization["poses"]), R.relative_to_first(ref["poses"]))
    print(f"vs reference: {dt:.3g} m {dr:.3g} rad, iterations {lc.last_optimization['iterations']} "
          f"(ref {ref['iterations']})")
    assert dt <= POS_TOL and dr <= ROT_TOL
    for i, p in enumerate(lc.last_optimization["poses"]):
        v = loop.get_translation_and_euler_angles(loop.pose_from_quat(p[:4], p[4:]))
        assert lc.key6d[i][:6] == np.array(v, np.float32).tolist(), i
    assert np.array_equal(T, lc._T6(-1))                    # T_map_0_curr from the last key pose
    assert np.allclose(lc.trans_loop_adjust, c.correction)

    def error(key6d, k):                                    # of node k relative to node 0
        rel = np.linalg.inv(loop.get_transformation(*key6d[0][:6])) @ loop.get_transformation(*key6d[k][:6])
        return float(np.linalg.norm((rel - np.linalg.inv(gt[0]) @ gt[k])[:3, 3]))
    print(f"end-point error {error(before, n - 1):.4f} -> {error(lc.key6d, n - 1):.4f} m, "
          f"mid-point {error(before, n // 2):.4f} -> {error(lc.key6d, n // 2):.4f} m")
    assert error(lc.key6d, n - 1) < error(before, n - 1)
    assert error(lc.key6d, n // 2) < error(before, n // 2)  # the path already driven is corrected

    off, (T0, c0, _) = _drive(fe, False, gt, od, constraint_for)
    assert c0 is not None and off.last_optimization is None and not off.graph_edges and not off.graph_init
    assert [v[:6] for v in off.key6d] == before
    assert np.allclose(off.trans_loop_adjust, c0.correction)


def test_several_closers_in_one_launch(fe):
    from ssf import loop
    gt, od = _square(20, 1.5)
    closers, cons = [], []
    for s in range(3):
        lc = loop.LoopCloser(fe, optimize=True)
        lc.add_loop_factor = lambda: None
        plane = torch.zeros(8, 4, device=fe.device)
        for k, T in enumerate(od[:20 - 2 * s]):
            p = loop.pose7_from_matrix(T)
            lc.process(plane, p[:4], p[4:], 0.1 * k)
        cur = len(lc.key6d) - 1
        corr = gt[cur] @ np.linalg.inv(lc._T6(cur))
        cons.append(loop.LoopConstraint(cur, 0, loop.between(gt[cur], lc._T6(0)), 0.02, corr))
        closers.append(lc)
    singles = []
    for lc, c in zip(closers, cons):
        g = lc.pose_graph()
        g["edge_ij"] = np.concatenate([g["edge_ij"], [[c.key_cur, c.key_pre]]]).astype(np.int32)
        g["edge_meas"] = np.concatenate([g["edge_meas"], [loop.pose7_from_matrix(c.between)]])
        g["edge_var"] = np.concatenate([g["edge_var"], [[c.noise] * 6]])
        singles.append(loop.optimize_pose_graphs(fe, [g])[0])
    Ts = loop.optimize_loop_closers(fe, closers, cons)
    for lc, one, T in zip(closers, singles, Ts):
        assert lc.last_optimization["status"] in GOOD
        assert lc.last_optimization["poses"].tobytes() == one["poses"].tobytes()
        assert np.array_equal(T, lc._T6(-1))


def test_run_sequence_map_optimize(dev, tmp_path):
    """An out-and-back drive through the onlyPC node graph: mapOptmization closes a loop on the
    way back.  With map_optimize the pose graph is solved and the key poses are rewritten; the
    odometry, and the map trajectory up to the loop, are what they are without it."""
    from ssf import loop, nodes, synth
    sc = synth.Scene(0)
    order = list(range(30)) + list(range(28, 18, -1))
    scans = {k: synth.scan(0, k, n_az=600, scene=sc) for k in set(order)}
    data = tmp_path / "data"
    data.mkdir()
    for i, k in enumerate(order):
        np.savez(str(data / f"{i:06d}.npz"), pos1=scans[k]["pos1"].numpy(), gt=scans[k]["flow"].numpy())
    runs = {}
    for flag in (False, True):
        tum2, tum3 = str(tmp_path / f"odom2_{flag}.txt"), str(tmp_path / f"map_{flag}.txt")
        with torch.cuda.device(dev):
            kw = dict(map_optimize=True) if flag else {}
            res = nodes.run_sequence(str(data), tum2, launch="onlyPC", map_tum_path=tum3, rate_hz=1.0, **kw)
        runs[flag] = (res, open(tum2).read(), open(tum3).read().splitlines())
    (r0, o0, m0), (r1, o1, m1) = runs[False], runs[True]
    assert len(r0["loops"]) == 1 and len(r1["loops"]) == 1
    assert "optimization" not in r0 and o0 == o1
    c = r1["loops"][0]
    opt = r1["optimization"]
    assert opt["status"] in GOOD and opt["loops"] == 1 and opt["cost"] < opt["cost0"]
    assert len(opt["poses"]) == c.key_cur + 1               # solved when that keyframe came in
    differ = [i for i, (a, b) in enumerate(zip(m0, m1)) if a != b]
    assert len(m0) == len(m1) and differ, "the corrected keyframe is published at its new pose"
    assert m0[:differ[0]] == m1[:differ[0]]
    for i, p in enumerate(opt["poses"]):
        v = loop.get_translation_and_euler_angles(loop.pose_from_quat(p[:4], p[4:]))
        assert r1["key_poses"][i][:6] == np.array(v, np.float32).tolist(), i

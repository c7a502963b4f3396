"""ssf_pose_graph_batch_lm on the GPU against tests/pgo_lm_reference.py (numpy f64, dense): the
step control of k_pose_graph_lm / k_pose_graph_wide_lm.  From far starts with radius0 = 1e16 (the
reject path and the doubling divisor) and near ones with the default radius, with and without a loss
on the loop edges, the device takes the yardstick's accept / reject path and ends where it ends;
the cost log never rises; a batch gives every graph its solo bits; without `lm` the entry point is
ssf_pose_graph_batch_robust; under a huge radius it is the plain solver within the parity bars.

Bars (the solver's): poses 1e-5 m / 1e-6 rad (absolute under the tight prior, X0^-1 Xi under the
reference prior), cost0 1e-9, cost and the accepted-point log 1e-6 relative, the outcome codes
equal, the radius after every attempt 1e-6 relative.  tests/test_pgo_lm_reference.py certifies that
every decision of the yardstick runs used here is clear of its threshold by a factor of 10."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pgo_lm_reference as M
import pgo_reference as R
import pgo_robust_reference as Q

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL = 1e-5, 1e-6
GOOD = (R.OK, R.CONVERGED)
KEYS = ("poses", "edge_ij", "edge_meas", "edge_var", "prior_pose", "prior_var")


@pytest.fixture(scope="module")
def fe(dev):
    from ssf import Frontend
    return Frontend(64, device=dev)


def _solve(fe, graphs, kind=None, radius0=1e4, lm_log=True, **kw):
    from ssf import loop
    return loop.optimize_pose_graphs(fe, [{key: g[key] for key in KEYS} for g in graphs],
                                     loop.pgo_params(**kw) if kw else None,
                                     robust=None if kind is None else loop.pgo_robust(kind), edge_out=True,
                                     lm=loop.pgo_lm(radius0=radius0), lm_log=lm_log)


def _non_increasing(log):
    return all(b <= a for a, b in zip(log[:-1], log[1:]))


def _check(name, g, got, ref, relative):
    floor = R.cost_floor(g)
    a, b = (R.relative_to_first(got["poses"]), R.relative_to_first(ref["poses"])) if relative else \
        (got["poses"], ref["poses"])
    dt, dr = R.pose_errors(a, b)
    n = min(len(got["lm_log"]), len(ref["lm_log"]))
    rad = float(np.max(np.abs(got["lm_log"][:n, 2] - ref["lm_log"][:n, 2]) / ref["lm_log"][:n, 2])) if n else 0.0
    clog = max((abs(x - y) / (y + floor) for x, y in zip(got["cost_log"], ref["cost_log"])), default=0.0)
    print(f"{name}: status {got['status_name']} attempts {got['iterations']} (ref {ref['iterations']}) accepted "
          f"{got['accepted']} (ref {ref['accepted']}) outcomes {''.join(str(int(o)) for o in got['lm_log'][:, 3])}")
    print(f"{name}: pose error {dt:.3g} m {dr:.3g} rad, cost0 {abs(got['cost0'] - ref['cost0']) / ref['cost0']:.3g} "
          f"cost {abs(got['cost'] - ref['cost']) / ref['cost']:.3g} log {clog:.3g} radius {rad:.3g} (relative)")
    assert got["status"] == ref["status"] and got["status"] in GOOD
    assert got["iterations"] == ref["iterations"] and got["accepted"] == ref["accepted"]
    assert got["lm_log"].shape == ref["lm_log"].shape
    assert np.array_equal(got["lm_log"][:, 3], ref["lm_log"][:, 3])
    assert np.all(np.abs(got["lm_log"][:, 2] - ref["lm_log"][:, 2]) <= 1e-6 * ref["lm_log"][:, 2])
    assert abs(got["radius"] - ref["radius"]) <= 1e-6 * ref["radius"] and got["radius"] == got["lm_log"][-1, 2]
    assert dt <= POS_TOL and dr <= ROT_TOL
    assert abs(got["cost0"] - ref["cost0"]) <= 1e-9 * ref["cost0"] + floor
    assert abs(got["cost"] - ref["cost"]) <= 1e-6 * ref["cost"] + floor
    assert len(got["cost_log"]) == got["iterations"] + 1 == len(ref["cost_log"])
    assert all(abs(x - y) <= 1e-6 * y + floor for x, y in zip(got["cost_log"], ref["cost_log"]))
    assert got["cost_log"][0] == got["cost0"] and got["cost_log"][-1] == got["cost"]
    assert _non_increasing(got["cost_log"])
    assert abs(got["dx"] - ref["dx"]) <= 1e-5 + 1e-6 * ref["dx"]
    # (weight, s) belong to the last accepted point
    assert np.all(np.abs(got["edge_weight"] - ref["edge_weight"]) <= 1e-6 * ref["edge_weight"])
    efloor = 2 * floor / (len(g["edge_ij"]) + 1)
    assert np.all(np.abs(got["edge_chi2"] - ref["edge_chi2"]) <= 1e-6 * ref["edge_chi2"] + efloor)


@pytest.mark.parametrize("name,kind", [(n, k) for n, c in M.PARITY.items() for k in c[1]])
def test_against_yardstick(fe, name, kind):
    g, ref, prm = M.parity_case(name, kind)
    got = _solve(fe, [g], kind, radius0=prm["radius0"], max_iter=prm["max_iter"], func_tol=prm["func_tol"])[0]
    _check(f"{name}/{kind}", g, got, ref, name.endswith("_ref"))
    wide = len(g["edge_ij"]) - (len(g["poses"]) - 1) > 32
    assert wide == ("wide" in name)
    if name.startswith("far"):
        out = list(got["lm_log"][:, 3])
        assert M.REJECTED in out and M.ACCEPTED in out[out.index(M.REJECTED):]


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("name", ["far_k6", "far_k12", "far_wide40"])
def test_eight_attempts_from_a_far_start_never_raise_the_cost(fe, name, kind):
    """the defaults of a loop closure (8 attempts, radius0 1e4) where Gauss-Newton's cost rises"""
    g = M.PARITY[name][0]()
    got = _solve(fe, [g], kind, radius0=1e4, max_iter=8, func_tol=1e-6)[0]
    back = M.cost_at(g, got["poses"], kind)
    print(f"{name}/{kind}: cost0 {got['cost0']:.6g} cost {got['cost']:.6g} accepted {got['accepted']}/{got['iterations']} "
          f"re-evaluated {back:.17g} ({abs(back - got['cost']) / back:.3g} relative)")
    assert got["status"] in GOOD and got["iterations"] <= 8
    assert _non_increasing(got["cost_log"]) and len(got["cost_log"]) == got["iterations"] + 1
    assert got["cost"] <= got["cost0"] and got["cost"] == got["cost_log"][-1]
    assert abs(back - got["cost"]) <= 1e-9 * back + R.cost_floor(g)
    assert got["accepted"] >= 1 and got["cost"] < got["cost0"] and got["dx"] > 0.0


# ---------------------------------------------------------------------------------- raw calls
def _raw(fe, graphs, prm, robust, lm, with_log, entry="ssf_pose_graph_batch_lm", sentinel=0.0):
    """One call of the C entry point -> (rc, poses, stats, cost log, edge output, lm log)."""
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    dev = fe.device
    cat = lambda key, dt, w: torch.from_numpy(np.concatenate(  # noqa: E731
        [np.ascontiguousarray(g[key], dt).reshape(-1, w) for g in graphs] + [np.zeros((1, w), dt)])).to(dev)
    pose, meas, var, ij = cat("poses", np.float64, 7), cat("edge_meas", np.float64, 7), \
        cat("edge_var", np.float64, 6), cat("edge_ij", np.int32, 2)
    prior, pvar = cat("prior_pose", np.float64, 7), cat("prior_var", np.float64, 6)
    h_noff = torch.tensor(np.concatenate([[0], np.cumsum([len(g["poses"]) for g in graphs])]), dtype=torch.int32)
    h_eoff = torch.tensor(np.concatenate([[0], np.cumsum([len(g["edge_ij"]) for g in graphs])]), dtype=torch.int32)
    d_noff, d_eoff = h_noff.to(dev), h_eoff.to(dev)
    G = len(graphs)
    stats = torch.full((G, _abi.PGO_OUT_STRIDE), sentinel, dtype=torch.float64, device=dev)
    clog = torch.full((G, prm.max_iter + 1), sentinel, dtype=torch.float64, device=dev)
    eout = torch.full((int(h_eoff[-1]) + 1, _abi.PGO_EDGE_OUT_STRIDE), sentinel, dtype=torch.float64, device=dev)
    llog = torch.full((G, prm.max_iter, _abi.PGO_LM_LOG_STRIDE), sentinel, dtype=torch.float64, device=dev)
    args = [fe._h, _stream(dev), G, _ptr(pose), _ptr(d_noff), C.c_void_p(h_noff.data_ptr()), _ptr(ij), _ptr(meas),
            _ptr(var), _ptr(d_eoff), C.c_void_p(h_eoff.data_ptr()), _ptr(prior), _ptr(pvar), C.byref(prm),
            _ptr(stats), _ptr(clog), None if robust is None else C.byref(robust), _ptr(eout)]
    if entry == "ssf_pose_graph_batch_lm":
        args += [None if lm is None else C.byref(lm), _ptr(llog) if with_log else None]
    rc = getattr(_abi.lib(), entry)(*args)
    torch.cuda.synchronize(dev)
    return rc, pose.cpu().numpy(), stats.cpu().numpy(), clog.cpu().numpy(), eout.cpu().numpy(), llog.cpu().numpy()


def _cut_graph():
    cut = R.copy_graph(R.fixture("k12_l3")[0])              # link 8 -> 9 missing: T is singular
    keep = [e for e, (i, j) in enumerate(cut["edge_ij"]) if {int(i), int(j)} != {8, 9}]
    for key in ("edge_ij", "edge_meas", "edge_var"):
        cut[key] = cut[key][keep]
    return cut


@pytest.mark.parametrize("kind", [None, "cauchy"])
def test_one_call_mixing_graph_kinds(fe, kind):
    """narrow and wide graphs and one without a chain link in one launch, without a loss and with
    one: every good graph has the bits of its solo solve, call after call; the broken one ends
    NOT_PD with its poses untouched and its log NaN"""
    from ssf import _abi, loop
    graphs = [M.PARITY["far_k12"][0](), M.PARITY["far_wide40"][0](), _cut_graph(), M.PARITY["near_k12"][0]()]
    prm, lm = loop.pgo_params(max_iter=12, func_tol=1e-6), loop.pgo_lm(radius0=1e16)
    rb = None if kind is None else loop.pgo_robust(kind)
    first = _raw(fe, graphs, prm, rb, lm, True)
    again = _raw(fe, graphs, prm, rb, lm, True)
    assert first[0] == again[0] == _abi.SSF_OK
    for a, b in zip(first[1:], again[1:]):
        assert a.tobytes() == b.tobytes()
    _, pose, stats, clog, eout, llog = first
    noff = np.concatenate([[0], np.cumsum([len(g["poses"]) for g in graphs])])
    eoff = np.concatenate([[0], np.cumsum([len(g["edge_ij"]) for g in graphs])])
    for k, g in enumerate(graphs):
        mine = (pose[noff[k]:noff[k + 1]], stats[k], clog[k], eout[eoff[k]:eoff[k + 1]], llog[k])
        if k == 2:
            assert int(stats[k, _abi.PGO_OUT["STATUS"]]) == R.NOT_PD
            assert mine[0].tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes()
            assert np.isnan(llog[k]).all() and np.isnan(mine[3]).all()
            assert stats[k, _abi.PGO_OUT["ITERATIONS"]] == 0 and stats[k, _abi.PGO_OUT["ACCEPTED"]] == 0
            continue
        rc, p1, s1, c1, e1, l1 = _raw(fe, [g], prm, rb, lm, True)
        assert rc == _abi.SSF_OK and int(s1[0, 0]) in GOOD, k
        solo = (p1[:len(g["poses"])], s1[0], c1[0], e1[:len(g["edge_ij"])], l1[0])
        for a, b in zip(mine, solo):
            assert a.tobytes() == b.tobytes(), k
        attempts = int(stats[k, _abi.PGO_OUT["ITERATIONS"]])
        assert 1 <= attempts <= 12 and not np.isnan(llog[k, :attempts, 2:]).any()
        assert np.isnan(llog[k, attempts:]).all() and np.isnan(clog[k, attempts + 1:]).all()
        assert _non_increasing(list(clog[k, :attempts + 1]))
        assert stats[k, _abi.PGO_OUT["ACCEPTED"]] == (llog[k, :attempts, 3] == _abi.PGO_LM_ACCEPTED).sum()


@pytest.mark.parametrize("name", R.STOP_RULE_FIXTURES)
def test_without_lm_the_entry_point_is_the_robust_one(fe, name):
    from ssf import _abi, loop
    g = R.fixture(name)[0]
    prm = loop.pgo_params()
    for rb in (None, loop.pgo_robust("huber")):
        new = _raw(fe, [g], prm, rb, None, False, sentinel=-7.0)
        old = _raw(fe, [g], prm, rb, None, False, entry="ssf_pose_graph_batch_robust", sentinel=-7.0)
        assert new[0] == old[0] == _abi.SSF_OK and int(new[2][0, 0]) in GOOD
        for a, b in zip(new[1:], old[1:]):
            assert a.tobytes() == b.tobytes()
        assert new[2][0, _abi.PGO_OUT["ACCEPTED"]] == 0.0 and new[2][0, _abi.PGO_OUT["RADIUS"]] == 0.0
        assert (new[5] == -7.0).all()                      # the log is not touched


@pytest.mark.parametrize("name", list(R.STOP_RULE_FIXTURES) + ["wide40"])
def test_huge_radius_is_the_plain_solver(fe, name):
    from ssf import loop
    g = Q.graph40() if name == "wide40" else R.fixture(name)[0]
    plain = loop.optimize_pose_graphs(fe, [{key: g[key] for key in KEYS}])[0]
    got = _solve(fe, [g], None, radius0=1e16)[0]
    dt, dr = R.pose_errors(got["poses"], plain["poses"])
    print(f"{name}: {dt:.3g} m {dr:.3g} rad from ssf_pose_graph_batch, cost "
          f"{abs(got['cost'] - plain['cost']) / plain['cost']:.3g} relative, {got['iterations']} attempts")
    assert plain["status"] in GOOD and got["status"] == plain["status"]
    assert got["iterations"] == plain["iterations"] == got["accepted"]
    assert dt <= POS_TOL and dr <= ROT_TOL
    assert abs(got["cost0"] - plain["cost0"]) <= 1e-9 * plain["cost0"]
    assert abs(got["cost"] - plain["cost"]) <= 1e-6 * plain["cost"] + R.cost_floor(g)
    assert np.array_equal(got["edge_weight"], np.ones(len(g["edge_ij"])))


def test_bad_step_control_is_rejected_on_a_live_context(fe):
    from ssf import _abi, loop
    g = R.fixture("k12_l3")[0]
    prm = loop.pgo_params()
    nan, inf = math.nan, math.inf
    bad = [(0.0, 1e-3, 1e16, 1e-32), (-1.0, 1e-3, 1e16, 1e-32), (nan, 1e-3, 1e16, 1e-32), (inf, 1e-3, 1e16, 1e-32),
           (1e4, 1e-3, 0.0, 1e-32), (1e4, 1e-3, inf, 1e-32), (1e4, 1e-3, nan, 1e-32), (1e4, 1e-3, 1e16, 0.0),
           (1e4, 1e-3, 1e16, -1.0), (1e4, 1e-3, 1e16, nan), (1e4, 1e-3, 1.0, 2.0), (1e4, -1e-3, 1e16, 1e-32),
           (1e4, 1.0, 1e16, 1e-32), (1e4, nan, 1e16, 1e-32)]
    for vals in bad:
        rc, pose, stats, clog, eout, llog = _raw(fe, [g], prm, None, _abi.PgoLm(*vals), True, sentinel=-7.0)
        assert rc == _abi.SSF_E_ARG, vals
        assert b"pose_graph_batch_lm" in _abi.lib().ssf_last_error(fe._h)
        assert pose[:len(g["poses"])].tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes()
        assert (stats == -7.0).all() and (llog == -7.0).all() and (eout == -7.0).all()
    rc = _raw(fe, [g], prm, None, None, True, sentinel=-7.0)    # a log without step control
    assert rc[0] == _abi.SSF_E_ARG and (rc[2] == -7.0).all()
    rc, _, stats, _, _, llog = _raw(fe, [g], prm, None, loop.pgo_lm(), True, sentinel=-7.0)
    assert rc == _abi.SSF_OK and int(stats[0, 0]) in GOOD and not (llog == -7.0).any()


# ------------------------------------------------------------------------ LoopCloser(lm=...)
def _square(n=20, step=1.5):
    """ground truth on a closed square and a drifting odometry of it (the drive of
    test_gpu_pose_graph_robust.py)"""
    from ssf import loop
    gt, od = [], []
    x = y = 0.0
    per = n // 4
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


def test_loop_closer_with_step_control(fe):
    """the 20-keyframe square with a true closure and then a false one (3 m off), Cauchy loss,
    step control and 30 attempts: every solve ends converged or ok and never raises its cost"""
    from ssf import loop
    gt, od = _square()
    n = len(od)
    lc = loop.LoopCloser(fe, optimize=True, robust=loop.pgo_robust("cauchy"), lm=loop.pgo_lm(),
                         pgo=loop.pgo_params(max_iter=30))
    plane = torch.zeros(8, 4, device=fe.device)

    def constraint():
        cur = len(lc.key6d) - 1
        if cur != n - 1:
            return None
        corr = gt[cur] @ np.linalg.inv(lc._T6(cur))
        pose_from = loop.get_transformation(*loop.get_translation_and_euler_angles(corr @ lc._T6(cur)))
        return loop.LoopConstraint(cur, 0, loop.between(pose_from, lc._T6(0)), 0.05, corr)

    lc.add_loop_factor = constraint
    for k, T in enumerate(od):
        p = loop.pose7_from_matrix(T)
        assert lc.process(plane, p[:4], p[4:], 0.1 * k)[2]  # every frame is a keyframe
    solves = [lc.last_optimization]
    cur, pre = 15, 5
    false_between = np.linalg.inv(gt[cur]) @ gt[pre] @ loop.get_transformation(3.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    lc.close_loop(loop.LoopConstraint(cur, pre, false_between, 0.05, np.eye(4)))
    solves.append(lc.last_optimization)
    for k, res in enumerate(solves):
        print(f"closure {k}: {res['status_name']} accepted {res['accepted']}/{res['iterations']} radius "
              f"{res['radius']:.3g} cost {res['cost0']:.6g} -> {res['cost']:.6g}")
        assert res["status"] in GOOD and res["loops"] == k + 1
        assert _non_increasing(res["cost_log"]) and res["cost"] <= res["cost0"]
        assert 1 <= res["accepted"] <= res["iterations"] <= 30 and res["radius"] > 0.0
    w = lc.loop_weights()
    assert [(a, b) for a, b, _ in w] == [(n - 1, 0), (cur, pre)] and w[1][2] < w[0][2] <= 1.0


def test_optimize_loop_closers_takes_lm(fe):
    from ssf import loop
    g = M.PARITY["far_k6"][0]()
    lcs = []
    for _ in range(2):
        lc = loop.LoopCloser(fe, optimize=True)
        lc.graph_init = [np.array(p) for p in g["poses"]]
        lc.graph_edges = [(int(i), int(j), m, v) for (i, j), m, v in zip(g["edge_ij"][:-1], g["edge_meas"], g["edge_var"])]
        lc.graph_prior = g["prior_pose"]
        lc.key6d = [[0.0] * 7 for _ in g["poses"]]
        lcs.append(lc)
    i, j = (int(v) for v in g["edge_ij"][-1])
    T = loop.pose_from_quat(g["edge_meas"][-1][:4], g["edge_meas"][-1][4:])
    cons = [loop.LoopConstraint(i, j, T, float(g["edge_var"][-1][0]), np.eye(4)) for _ in lcs]
    loop.optimize_loop_closers(fe, lcs, cons, loop.pgo_params(max_iter=12), lm=loop.pgo_lm(radius0=1e16))
    for lc in lcs:
        res = lc.last_optimization
        assert res["status"] in GOOD and "accepted" in res and res["radius"] > 0.0
        assert _non_increasing(res["cost_log"]) and 1 <= res["accepted"] < res["iterations"] <= 12


def test_run_sequence_map_lm(dev, tmp_path):
    """The out-and-back drive of test_gpu_pose_graph.py through the onlyPC node graph with map_lm
    and map_iters: they reach the solve of the loop closure."""
    from ssf import loop, nodes, synth
    sc = synth.Scene(0)
    order = list(range(30)) + list(range(28, 18, -1))
    scans = {k: synth.scan(0, k, n_az=600, scene=sc) for k in set(order)}
    data = tmp_path / "data"
    data.mkdir()
    for i, k in enumerate(order):
        np.savez(str(data / f"{i:06d}.npz"), pos1=scans[k]["pos1"].numpy(), gt=scans[k]["flow"].numpy())
    with torch.cuda.device(dev):
        res = nodes.run_sequence(str(data), None, launch="onlyPC", map_tum_path=str(tmp_path / "map.txt"),
                                 rate_hz=1.0, map_optimize=True, map_lm=loop.pgo_lm(), map_iters=30)
    opt = res["optimization"]
    assert len(res["loops"]) == 1 and opt["status"] in GOOD and opt["loops"] == 1
    assert 1 <= opt["accepted"] <= opt["iterations"] <= 30 and opt["radius"] > 0.0
    assert _non_increasing(opt["cost_log"]) and opt["cost"] <= opt["cost0"]
    assert "edge_weight" not in opt

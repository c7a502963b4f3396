"""Robust loop-edge losses of the GPU pose-graph optimiser (ssf_pose_graph_batch_robust;
k_pose_graph_robust / k_pose_graph_wide_robust, pose_graph.hip) against the numpy
IRLS Gauss-Newton of tests/pgo_robust_reference.py.

The bars are those of test_gpu_pose_graph.py: poses within 1e-5 m and 1e-6 rad (absolute under
the tight prior, relative to node 0 under the reference's prior), initial cost within 1e-9
relative, final cost within 1e-6 relative plus pgo_reference.cost_floor.  Edge weights and the
per-edge squared residuals are held to 1e-6 relative, like the final cost they are taken with; a
squared residual that f64 rounding alone can produce (an edge's share of cost_floor) counts as
zero on both sides.  A case runs at the default stop rule where every stop check of the yardstick
is clear of func_tol by a factor of 10, and three steps in fixed-iteration mode elsewhere."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pgo_reference as R
import pgo_robust_reference as Q
import pgo_wide_fixtures as W

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL = 1e-5, 1e-6
GOOD = (R.OK, R.CONVERGED)
KEYS = ("poses", "edge_ij", "edge_meas", "edge_var", "prior_pose", "prior_var")
LOSSES = ("huber", "cauchy", "geman_mcclure")
PRIORS = dict(tight=R.TIGHT_PRIOR_VAR, ref=R.REF_PRIOR_VAR)
FIXED = dict(max_iter=3, func_tol=0.0)


@pytest.fixture(scope="module")
def fe(dev):
    from ssf import Frontend
    return Frontend(64, device=dev)


def _solve(fe, graphs, kind=None, k=None, edge_out=False, **kw):
    from ssf import loop
    return loop.optimize_pose_graphs(fe, [{key: g[key] for key in KEYS} for g in graphs],
                                     loop.pgo_params(**kw) if kw else None,
                                     robust=None if kind is None else loop.pgo_robust(kind, k), edge_out=edge_out)


def _yardstick(key, g, kind, k=None):
    """-> (the yardstick's solution, the parameters it was run with): the default stop rule where
    every one of its decisions is clear by a factor of 10, else three fixed steps.  Once per process."""
    def build():
        s = Q.solve(g, kind, k)
        if all(m >= 10 or m <= 0.1 for m in R.stop_margins(s["cost_log"])):
            return s, {}
        return Q.solve(g, kind, k, **FIXED), FIXED
    return Q.cached(("gpu", key, kind, k), build)


def _edge_floor(g):
    return 2 * R.cost_floor(g) / (len(g["edge_ij"]) + 1)


def _check(name, g, got, ref, relative, params):
    floor = R.cost_floor(g)
    print(f"{name}: status {got['status_name']} it {got['iterations']} (ref {ref['iterations']}) "
          f"cost0 {got['cost0']:.17g} (ref {ref['cost0']:.17g}) cost {got['cost']:.17g} (ref {ref['cost']:.17g}) "
          f"mode {'fixed' if params else 'default'}")
    assert got["status"] == ref["status"] and got["status"] in GOOD
    assert got["iterations"] == ref["iterations"]
    a, b = (R.relative_to_first(got["poses"]), R.relative_to_first(ref["poses"])) if relative else \
        (got["poses"], ref["poses"])
    dt, dr = R.pose_errors(a, b)
    dw = float(np.max(np.abs(got["edge_weight"] - ref["edge_weight"]) / ref["edge_weight"]))
    ds = np.abs(got["edge_chi2"] - ref["edge_chi2"])
    print(f"{name}: pose error {dt:.3g} m {dr:.3g} rad, cost0 {abs(got['cost0'] - ref['cost0']) / ref['cost0']:.3g} "
          f"cost {abs(got['cost'] - ref['cost']) / ref['cost']:.3g} weight {dw:.3g} "
          f"chi2 {float(np.max(ds / np.maximum(ref['edge_chi2'], _edge_floor(g)))):.3g} (relative)")
    assert dt <= POS_TOL and dr <= ROT_TOL
    assert abs(got["cost0"] - ref["cost0"]) <= 1e-9 * ref["cost0"] + floor
    assert abs(got["cost"] - ref["cost"]) <= 1e-6 * ref["cost"] + floor
    assert got["loops"] == W.true_loops(g)
    assert len(got["cost_log"]) == got["iterations"] + 1
    assert got["cost_log"][0] == got["cost0"] and got["cost_log"][-1] == got["cost"]
    assert got["edge_weight"].shape == got["edge_chi2"].shape == (len(g["edge_ij"]),)
    assert np.all(np.abs(got["edge_weight"] - ref["edge_weight"]) <= 1e-6 * ref["edge_weight"])
    assert np.all(ds <= 1e-6 * ref["edge_chi2"] + _edge_floor(g))
    chain = [e for e in range(len(g["edge_ij"])) if e not in Q.loop_edges(g)]
    assert np.array_equal(got["edge_weight"][chain], np.ones(len(chain)))


# ------------------------------------------------------------------------------ narrow kernel
NARROW = {
    "k6_l2": (lambda pv: R.circle_graph(6, [(0, 4), (1, 5)], prior_var=pv), (0,)),
    "k12_l3": (lambda pv: R.circle_graph(12, [(0, 10), (1, 11), (2, 9)], prior_var=pv), (1,)),
}


@pytest.mark.parametrize("prior", list(PRIORS))
@pytest.mark.parametrize("kind", LOSSES)
@pytest.mark.parametrize("name", list(NARROW))
def test_narrow_graph_against_yardstick(fe, name, kind, prior):
    build, which = NARROW[name]
    g, bad = Q.cached((name, prior), lambda: Q.corrupt_loops(build(PRIORS[prior]), which))
    assert W.extra_edges(g) <= W.NARROW_LOOPS
    ref, params = _yardstick((name, prior), g, kind)
    got = _solve(fe, [g], kind, **params)[0]
    _check(f"{name}/{kind}/{prior}", g, got, ref, prior == "ref", params)
    assert got["edge_weight"][bad[0]] == got["edge_weight"].min() < 1.0


# -------------------------------------------------------------------------------- wide kernel
def _k40(prior):
    return Q.cached(("k40", prior), lambda: Q.corrupt_loops(
        R.circle_graph(40, R.spread_loops(40, 33, 0), seed=1, prior_var=PRIORS[prior]), (3, 17, 30)))


@pytest.mark.parametrize("prior", list(PRIORS))
@pytest.mark.parametrize("kind", LOSSES)
def test_wide_graph_against_yardstick(fe, kind, prior):
    g, bad = _k40(prior)
    assert W.extra_edges(g) > W.NARROW_LOOPS
    ref, params = _yardstick(("k40", prior), g, kind)
    got = _solve(fe, [g], kind, **params)[0]
    _check(f"k40_l33/{kind}/{prior}", g, got, ref, prior == "ref", params)
    clean = [e for e in Q.loop_edges(g) if e not in bad]
    assert got["edge_weight"][bad].max() < got["edge_weight"][clean].min()


@pytest.mark.parametrize("prior", list(PRIORS))
def test_wide_graph_over_256_columns_huber(fe, prior):
    g, bad = Q.cached(("k60", prior), lambda: Q.corrupt_loops(W.WIDE["k60_l85"](PRIORS[prior]), (2, 20, 41, 60, 84)))
    assert 6 * W.true_loops(g) + 1 > 256
    ref, params = _yardstick(("k60", prior), g, "huber")
    got = _solve(fe, [g], "huber", **params)[0]
    _check(f"k60_l85/huber/{prior}", g, got, ref, prior == "ref", params)
    clean = [e for e in Q.loop_edges(g) if e not in bad]
    assert got["edge_weight"][bad].max() < got["edge_weight"][clean].min()


# ------------------------------------------------- the new kernels against the plain ones
def _plain_cases():
    out = [(name, R.fixture(name, prior)[0], {}, prior) for name in R.STOP_RULE_FIXTURES for prior in PRIORS]
    out += [(name, W.wide_fixture(name, prior)[0], W.solve_params(name), prior)
            for name in ("k40_l33", "k60_l85") for prior in PRIORS]
    return out


def _agree_with_plain(name, g, plain, got, relative):
    """the bars of _check between two device runs, unit weights, and the reported s add up to the cost"""
    floor = R.cost_floor(g)
    assert plain["status"] in GOOD and got["status"] == plain["status"], name
    assert got["iterations"] == plain["iterations"] and got["loops"] == plain["loops"], name
    a, b = (R.relative_to_first(got["poses"]), R.relative_to_first(plain["poses"])) if relative else \
        (got["poses"], plain["poses"])
    dt, dr = R.pose_errors(a, b)
    assert dt <= POS_TOL and dr <= ROT_TOL, name
    assert abs(got["cost0"] - plain["cost0"]) <= 1e-9 * plain["cost0"] + floor, name
    assert abs(got["cost"] - plain["cost"]) <= 1e-6 * plain["cost"] + floor, name
    assert np.array_equal(got["edge_weight"], np.ones(len(g["edge_ij"]))), name
    total = float(got["edge_chi2"].sum()) + Q.prior_chi2(g, got["poses"])
    print(f"{name}: bit-identical poses {got['poses'].tobytes() == plain['poses'].tobytes()}, cost log "
          f"{got['cost_log'] == plain['cost_log']}; pose difference {dt:.3g} m {dr:.3g} rad; "
          f"sum of s {total:.17g} against 2 cost {2 * got['cost']:.17g}")
    assert abs(total - 2 * got["cost"]) <= 1e-9 * 2 * got["cost"] + 2 * floor, name


def test_kind_none_through_the_robust_kernels_is_the_plain_solver(fe):
    for name, g, params, prior in _plain_cases():
        plain = _solve(fe, [g], **params)[0]
        assert "edge_weight" not in plain and "edge_chi2" not in plain
        got = _solve(fe, [g], edge_out=True, **params)[0]
        _agree_with_plain(f"{name}/{prior}/edge_out", g, plain, got, prior == "ref")
        got = _solve(fe, [g], "none", **params)[0]
        _agree_with_plain(f"{name}/{prior}/none", g, plain, got, prior == "ref")


def test_huber_with_every_edge_an_inlier_is_the_plain_solver(fe):
    for name, g, params, prior in _plain_cases():
        plain = _solve(fe, [g], **params)[0]
        got = _solve(fe, [g], "huber", 1e6, **params)[0]
        _agree_with_plain(f"{name}/{prior}/huber 1e6", g, plain, got, prior == "ref")


# --------------------------------------------------------------------- one call, mixed graphs
def _same(ra, rb):
    for key in ("status", "iterations", "cost0", "cost", "dx", "loops", "cost_log"):
        if not (ra[key] == rb[key] or (isinstance(ra[key], float) and math.isnan(ra[key]) and math.isnan(rb[key]))):
            return key
    for key in ("poses", "edge_weight", "edge_chi2"):
        if ra[key].tobytes() != rb[key].tobytes():
            return key
    return None


def test_one_call_mixing_graph_kinds(fe):
    nan = R.copy_graph(R.fixture("k12_l3")[0])
    nan["edge_meas"][7, 5] = math.nan
    cut = R.copy_graph(R.fixture("k12_l3")[0])              # link 8 -> 9 missing: T is singular
    keep = [e for e, (i, j) in enumerate(cut["edge_ij"]) if {int(i), int(j)} != {8, 9}]
    for key in ("edge_ij", "edge_meas", "edge_var"):
        cut[key] = cut[key][keep]
    narrow = Q.cached(("k12_l3", "tight"), lambda: Q.corrupt_loops(NARROW["k12_l3"][0](PRIORS["tight"]), (1,)))[0]
    graphs = [narrow, _k40("tight")[0], R.circle_graph(0), nan, R.fixture("k65_l0")[0], cut]
    want = [None, None, R.EMPTY, R.BAD_INPUT, None, R.NOT_PD]
    res = _solve(fe, graphs, "huber")
    for k, (g, r, st) in enumerate(zip(graphs, res, want)):
        assert r["edge_weight"].shape == r["edge_chi2"].shape == (len(g["edge_ij"]),), k
        if st is not None:
            assert r["status"] == st, (k, r["status_name"])
            assert r["poses"].tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes(), k
            assert np.isnan(r["edge_weight"]).all() and np.isnan(r["edge_chi2"]).all(), k
            continue
        one = _solve(fe, [g], "huber")[0]
        assert one["status"] in GOOD, k
        assert _same(r, one) is None, (k, _same(r, one))
    assert W.true_loops(graphs[4]) == 0 and res[4]["loops"] == 0
    assert np.array_equal(res[4]["edge_weight"], np.ones(len(graphs[4]["edge_ij"])))
    assert np.all(res[1]["edge_weight"] > 0) and res[1]["edge_weight"].min() < 1.0


# ------------------------------------------------------------------------------- bad arguments
def test_bad_loss_is_rejected_on_a_live_context(fe):
    from ssf import _abi, loop
    from ssf.frontend import _ptr, _stream
    g = R.fixture("k12_l3")[0]
    dev = fe.device
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    K, E = len(g["poses"]), len(g["edge_ij"])
    pose = up(g["poses"], np.float64)
    ij, meas, var = up(g["edge_ij"], np.int32), up(g["edge_meas"], np.float64), up(g["edge_var"], np.float64)
    prior, pvar = up(g["prior_pose"], np.float64), up(g["prior_var"], np.float64)
    h_noff, h_eoff = torch.tensor([0, K], dtype=torch.int32), torch.tensor([0, E], dtype=torch.int32)
    d_noff, d_eoff = h_noff.to(dev), h_eoff.to(dev)
    stats = torch.zeros(1, _abi.PGO_OUT_STRIDE, dtype=torch.float64, device=dev)
    eout = torch.full((E, _abi.PGO_EDGE_OUT_STRIDE), -7.0, dtype=torch.float64, device=dev)
    prm = loop.pgo_params()

    def call(rb):
        return _abi.lib().ssf_pose_graph_batch_robust(
            fe._h, _stream(dev), 1, _ptr(pose), _ptr(d_noff), C.c_void_p(h_noff.data_ptr()), _ptr(ij), _ptr(meas),
            _ptr(var), _ptr(d_eoff), C.c_void_p(h_eoff.data_ptr()), _ptr(prior), _ptr(pvar), C.byref(prm),
            _ptr(stats), None, C.byref(rb), _ptr(eout))

    for kind, k in ((7, 1.0), (-1, 1.0), (_abi.PGO_ROBUST_HUBER, 0.0), (_abi.PGO_ROBUST_HUBER, -1.0),
                    (_abi.PGO_ROBUST_CAUCHY, math.nan), (_abi.PGO_ROBUST_GEMAN_MCCLURE, math.inf)):
        assert call(_abi.PgoRobust(kind, k)) == _abi.SSF_E_ARG, (kind, k)
        assert b"pose_graph_batch_robust" in _abi.lib().ssf_last_error(fe._h)
    torch.cuda.synchronize(dev)
    assert pose.cpu().numpy().tobytes() == np.ascontiguousarray(g["poses"], np.float64).tobytes()
    assert bool((eout == -7.0).all()) and bool((stats == 0.0).all())
    # kind none ignores k; the same buffers then solve
    assert call(_abi.PgoRobust(_abi.PGO_ROBUST_NONE, math.nan)) == _abi.SSF_OK
    torch.cuda.synchronize(dev)
    assert int(stats[0, 0]) in GOOD and bool((eout[:, 0] == 1.0).all())


# ------------------------------------------------------------------ LoopCloser(robust=...)
def _square(n=20, step=1.5):
    """ground truth on a closed square and a drifting odometry of it (test_gpu_pose_graph.py's
    drive, at the size its several-closers test uses: 0.35 m of drift when the loop closes, so the
    true closure stays near Huber's threshold.  On the 40-keyframe, 2 m-step square the drift is
    2 m, the true closure is an outlier as well (weight 0.14 on the yardstick) and the loss does
    not help: DESIGN.md §6.7)"""
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


def _drive(fe, gt, od, robust):
    """every odometry pose through LoopCloser.process; the last keyframe closes a hand-built true
    loop to keyframe 0 (add_loop_factor replaced: what a perfect ICP would return)"""
    from ssf import loop
    lc = loop.LoopCloser(fe, optimize=True, robust=robust)
    plane = torch.zeros(8, 4, device=fe.device)
    n = len(od)

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
    return lc


def _error(poses7, gt):
    """largest distance of a node from its ground truth, both relative to node 0 [m]"""
    from ssf import loop
    a = R.relative_to_first(poses7)
    b = R.relative_to_first(np.array([loop.pose7_from_matrix(T) for T in gt]))
    return float(np.linalg.norm(a[:, 4:] - b[:, 4:], axis=1).max())


def _key_poses7(lc):
    from ssf import loop
    return np.array([loop.pose7_from_matrix(loop.get_transformation(*k[:6])) for k in lc.key6d])


def test_loop_closer_down_weights_a_false_loop(fe):
    from ssf import loop
    gt, od = _square()
    n = len(od)
    cur, pre = 15, 5                                        # a false closure: the true between, 3 m off
    false_between = np.linalg.inv(gt[cur]) @ gt[pre] @ loop.get_transformation(3.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    runs = {}
    for name, robust in (("plain", None), ("huber", loop.pgo_robust("huber"))):
        lc = _drive(fe, gt, od, robust)
        assert lc.last_optimization["status"] in GOOD and lc.last_optimization["loops"] == 1
        g = lc.pose_graph()                                 # as it stands before the false edge
        c = loop.LoopConstraint(cur, pre, false_between, 0.05, np.eye(4))
        lc.close_loop(c)
        g["edge_ij"] = np.concatenate([g["edge_ij"], [[cur, pre]]]).astype(np.int32)
        g["edge_meas"] = np.concatenate([g["edge_meas"], [loop.pose7_from_matrix(c.between)]])
        g["edge_var"] = np.concatenate([g["edge_var"], [[c.noise] * 6]])
        ref = Q.solve(g, "none" if robust is None else "huber")
        runs[name] = (lc, ref)
        assert lc.last_optimization["status"] in GOOD and lc.last_optimization["loops"] == 2
        assert len(lc.graph_edges) == n - 1 + 2
    (plain, ref_plain), (huber, ref_huber) = runs["plain"], runs["huber"]
    assert "edge_weight" not in plain.last_optimization and "edge_chi2" not in plain.last_optimization
    assert plain.loop_weights() == []
    w = huber.loop_weights()
    print("loop weights", w, "yardstick", ref_huber["edge_weight"][-2:])
    assert [(a, b) for a, b, _ in w] == [(n - 1, 0), (cur, pre)]
    assert w[1][2] < w[0][2] <= 1.0 and w[1][2] == min(v for _, _, v in w)
    # the ordering on the yardstick, on the recorded graphs, then on the device's key poses
    y_plain, y_huber = _error(ref_plain["poses"], gt), _error(ref_huber["poses"], gt)
    d_plain, d_huber = _error(_key_poses7(plain), gt), _error(_key_poses7(huber), gt)
    print(f"distance to ground truth: plain {d_plain:.4f} m, huber {d_huber:.4f} m "
          f"(yardstick {y_plain:.4f} m, {y_huber:.4f} m)")
    assert y_huber < y_plain
    assert d_huber < d_plain


def test_run_sequence_map_robust(dev, tmp_path):
    """The out-and-back drive of test_gpu_pose_graph.py through the onlyPC node graph with
    map_robust: the loss reaches the solve of the loop closure and the weights come back."""
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
                                 rate_hz=1.0, map_optimize=True, map_robust=loop.pgo_robust("huber"))
    opt = res["optimization"]
    assert len(res["loops"]) == 1 and opt["status"] in GOOD and opt["loops"] == 1
    E = len(opt["poses"]) - 1 + 1                           # the chain and the loop edge
    assert opt["edge_weight"].shape == opt["edge_chi2"].shape == (E,)
    assert np.array_equal(opt["edge_weight"][:-1], np.ones(E - 1)) and 0.0 < opt["edge_weight"][-1] <= 1.0
    s, k = float(opt["edge_chi2"][-1]), 1.345
    assert abs(opt["edge_weight"][-1] - Q.weight("huber", k, s)) <= 1e-12

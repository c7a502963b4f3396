"""Pose-graph optimiser, CPU side: the argument checks of ssf_pose_graph_batch (before any HIP
call), its default parameters, and the sanity of the numpy yardstick (tests/pgo_reference.py)
the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest

import pgo_reference as R


def test_params_default_and_constants():
    from ssf import _abi
    L = _abi.lib()
    p = _abi.PgoParams()
    assert L.ssf_pgo_params_default(C.byref(p)) == _abi.SSF_OK
    assert (p.max_iter, p.func_tol) == (8, 1e-6)
    assert L.ssf_pgo_params_default(None) == _abi.SSF_E_ARG
    assert L.ssf_abi_version() == 2
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include",
                                          "ssf_frontend.h")).read()
    assert f"#define SSF_PGO_MAX_LOOPS {_abi.PGO_MAX_LOOPS}" in hdr and _abi.PGO_MAX_LOOPS >= 32
    assert f"#define SSF_PGO_OUT_STRIDE {_abi.PGO_OUT_STRIDE}" in hdr
    assert f"#define SSF_PGO_MAX_ITER {_abi.PGO_MAX_ITER}" in hdr
    assert (R.OK, R.CONVERGED, R.EMPTY, R.BAD_INPUT, R.TOO_MANY_LOOPS, R.NOT_PD) == (
        _abi.PGO_OK, _abi.PGO_CONVERGED, _abi.PGO_EMPTY, _abi.PGO_BAD_INPUT, _abi.PGO_TOO_MANY_LOOPS,
        _abi.PGO_NOT_PD)


def test_arg_errors_with_null_context():
    """a null context is SSF_E_ARG whatever else is passed, and nothing is dereferenced"""
    from ssf import _abi
    L = _abi.lib()
    p = _abi.PgoParams()
    L.ssf_pgo_params_default(C.byref(p))
    nul = [None] * 10
    assert L.ssf_pose_graph_batch(None, None, 1, *nul, C.byref(p), None, None) == _abi.SSF_E_ARG
    assert L.ssf_pose_graph_batch(None, None, -1, *nul, C.byref(p), None, None) == _abi.SSF_E_ARG
    assert L.ssf_pose_graph_batch(None, None, 0, *nul, None, None, None) == _abi.SSF_E_ARG
    off = np.array([0, 3], np.int32)
    bad = np.array([3, 0], np.int32)
    buf = np.zeros(64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = [vp(buf), vp(off), vp(bad), vp(buf), vp(buf), vp(buf), vp(off), vp(off), vp(buf), vp(buf)]
    assert L.ssf_pose_graph_batch(None, None, 1, *args, C.byref(p), vp(buf), None) == _abi.SSF_E_ARG
    assert L.ssf_last_error(None) == b"null context"


def test_python_entry_rejects_ragged_edges():
    from ssf import loop
    g, _ = R.fixture("k5_l1")
    g["edge_var"] = g["edge_var"][:-1]
    with pytest.raises(ValueError, match="differ in length"):
        loop.optimize_pose_graphs(None, [g])
    assert loop.optimize_pose_graphs(None, []) == []


def _numeric_jacobians(xi, xj, z, var, h=1e-6):
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for c in range(6):
        d = np.zeros(6)
        d[c] = h
        Ji[:, c] = (R.residual_only(R.retract(xi, d), xj, z, var) - R.residual_only(R.retract(xi, -d), xj, z, var)) / (2 * h)
        Jj[:, c] = (R.residual_only(xi, R.retract(xj, d), z, var) - R.residual_only(xi, R.retract(xj, -d), z, var)) / (2 * h)
    return Ji, Jj


def test_reference_jacobians_match_central_differences():
    rng = np.random.default_rng(0)
    g, _ = R.fixture("k12_l3")
    for trial in range(12):
        i, j = rng.choice(12, 2, replace=False)
        xi, xj = g["poses"][i], g["poses"][j]
        # residual rotations from tiny to large (the Jr^-1 closed form and its small-angle series)
        scale = [0.0, 1e-9, 1e-3, 0.3, 1.0, 2.0][trial % 6]
        z = R.retract(R.pose_between(xi, xj), np.concatenate([scale * rng.normal(size=3), rng.normal(size=3)]))
        var = rng.uniform(0.5, 2.0, 6)
        _, Ji, Jj = R.between_factor(xi, xj, z, var)
        Ni, Nj = _numeric_jacobians(xi, xj, z, var)
        assert np.abs(Ji - Ni).max() < 1e-6 and np.abs(Jj - Nj).max() < 1e-6, (trial, scale)
    # the prior: E = P^-1 X0, the dj form
    x0 = g["poses"][4]
    P = R.retract(x0, np.array([0.2, -0.1, 0.3, 1.0, -2.0, 0.5]))
    _, _, Jj = R.between_factor(R.IDENTITY, x0, P, np.ones(6))
    _, Nj = _numeric_jacobians(R.IDENTITY, x0, P, np.ones(6))
    assert np.abs(Jj - Nj).max() < 1e-6


def test_reference_consistent_chain_has_zero_cost():
    for name in ("k1", "k2", "k65_l0"):
        g, s = R.fixture(name)
        assert s["cost0"] <= R.cost_floor(g), (name, s["cost0"])
        assert s["cost"] <= R.cost_floor(g), (name, s["cost"])
        dt, dr = R.pose_errors(s["poses"], g["poses"])
        assert dt < 1e-9 and dr < 1e-10, (name, dt, dr)


@pytest.mark.parametrize("prior", ["tight", "ref"])
def test_reference_cost_is_monotone_and_reduced(prior):
    for name in R.FIXTURES:
        g, s = R.fixture(name, prior)
        log, floor = s["cost_log"], R.cost_floor(g)
        assert all(b <= a * (1 + 1e-12) + floor for a, b in zip(log[:-1], log[1:])), (name, log)
        assert len(log) == s["iterations"] + 1
        if len(g["edge_ij"]) > len(g["poses"]) - 1 and name != "k12_l3":
            assert s["status"] == R.CONVERGED and s["cost"] < s["cost0"], name


@pytest.mark.parametrize("prior", ["tight", "ref"])
def test_stop_rule_fixtures_are_far_from_the_tolerance(prior):
    """what the GPU stop-rule test relies on: every check of these fixtures is decided by a
    factor of at least 100, so rounding cannot move the iteration count"""
    for name in R.STOP_RULE_FIXTURES:
        g, s = R.fixture(name, prior)
        assert s["status"] == R.CONVERGED and s["cost"] > 1e6 * R.cost_floor(g)
        assert all(m >= 100 or m <= 0.01 for m in R.stop_margins(s["cost_log"])), (name, s["cost_log"])


def test_gauge_relative_poses_do_not_depend_on_the_prior():
    """the reference prior leaves the global position numerically free; relative to node 0 the
    two priors give the same trajectory"""
    for name in ("k5_l1", "k65_l11"):
        a = R.relative_to_first(R.fixture(name, "tight")[1]["poses"])
        b = R.relative_to_first(R.fixture(name, "ref")[1]["poses"])
        dt, dr = R.pose_errors(a, b)
        assert dt < 1e-5 and dr < 1e-6, (name, dt, dr)

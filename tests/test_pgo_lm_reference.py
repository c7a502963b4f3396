"""The premises of the step-control pose-graph tests, on the CPU: the yardstick of
tests/pgo_lm_reference.py converges from far starts where Gauss-Newton's cost rises, reduces to
tests/pgo_reference.py under a huge radius, and every decision of the runs the GPU tests compare
against is clear of its threshold; the host side of the new options rejects bad input before any
GPU work."""
import ctypes as C
import math

import numpy as np
import pytest

import pgo_lm_reference as M
import pgo_reference as R
import pgo_robust_reference as Q


def _non_increasing(log):
    return all(b <= a for a, b in zip(log[:-1], log[1:]))


@pytest.mark.parametrize("kind", ["none", "cauchy"])
@pytest.mark.parametrize("K", [6, 12])
def test_far_start_converges_where_gauss_newton_rises(K, kind):
    """Recorded, not asserted: 11/20 and 12/21 accepted/attempts for K = 6 (none, Cauchy), 18/28 and
    19/29 for K = 12."""
    far, near = M.far_small(K)
    s = Q.cached(("lm_far", K, kind), lambda: M.solve(far, kind, max_iter=40, radius0=1e16))
    n = M.solve(near, kind, max_iter=40, radius0=1e16)
    print(f"K {K} {kind}: {s['accepted']}/{s['iterations']} accepted/attempts, cost {s['cost0']:.6g} -> "
          f"{s['cost']:.12g} (from the unperturbed start {n['cost']:.12g})")
    assert _non_increasing(s["cost_log"]) and len(s["cost_log"]) == s["iterations"] + 1
    assert s["cost_log"][0] == s["cost0"] and s["cost_log"][-1] == s["cost"] <= s["cost0"]
    out = s["outcome"]
    assert M.REJECTED in out and M.ACCEPTED in out[out.index(M.REJECTED):]
    assert s["status"] == R.CONVERGED and n["status"] == R.CONVERGED
    assert abs(s["cost"] - n["cost"]) <= 1e-6 * n["cost"]
    assert s["accepted"] == out.count(M.ACCEPTED) and s["lm_log"].shape == (s["iterations"], 4)
    # the contrast the step control exists for: Gauss-Newton's cost rises on the same input
    gn = Q.solve(far, kind, max_iter=8)
    assert not _non_increasing(gn["cost_log"])


@pytest.mark.parametrize("name", R.STOP_RULE_FIXTURES)
def test_huge_radius_is_gauss_newton(name):
    g, ref = R.fixture(name)
    s = M.solve(g, "none", radius0=1e16)
    assert M.REJECTED not in s["outcome"] and M.INVALID not in s["outcome"]
    assert s["status"] == ref["status"] and s["iterations"] == ref["iterations"] == s["accepted"]
    dt, dr = R.pose_errors(s["poses"], ref["poses"])
    print(f"{name}: {dt:.3g} m {dr:.3g} rad from pgo_reference.solve")
    assert dt <= 1e-9 and dr <= 1e-10
    assert abs(s["cost"] - ref["cost"]) <= 1e-9 * ref["cost"]


@pytest.mark.parametrize("name,kind", [(n, k) for n, c in M.PARITY.items() for k in c[1]])
def test_parity_cases_decide_clearly(name, kind):
    """What the GPU parity tests rely on: in the run they compare against, every accept decision
    (rho >= 1e-2, or the trial raised the cost) and every stop check is clear by a factor of 10."""
    g, s, prm = M.parity_case(name, kind)
    rho = [r for r in s["rho"] if not math.isnan(r)]
    print(f"{name}/{kind}: {prm}, {s['accepted']}/{s['iterations']} accepted/attempts, status {s['status']}, "
          f"smallest accepted rho {min(r for r, o in zip(s['rho'], s['outcome']) if o == M.ACCEPTED):.3g}, "
          f"largest rejected rho {max([r for r, o in zip(s['rho'], s['outcome']) if o == M.REJECTED], default=math.nan):.3g}")
    assert M.first_unclear(s) is None
    assert len(rho) == s["iterations"] and s["iterations"] >= 2 and s["accepted"] >= 2
    assert _non_increasing(s["cost_log"])
    if prm["radius0"] == 1e16 and name.startswith("far"):     # the reject path and the dec doubling
        assert s["outcome"][:2] == [M.REJECTED, M.REJECTED] and M.ACCEPTED in s["outcome"]
    else:
        assert M.REJECTED not in s["outcome"]
    for margin in s["stop_margin"]:
        assert margin is None or margin >= 10 or margin <= 0.1


def test_far_start_generator_is_seeded_and_keeps_node_0():
    g = R.circle_graph(6, [(5, 0)], seed=2)
    a, b = M.far_start(g, 3, 1.0, 5.0), M.far_start(g, 3, 1.0, 5.0)
    assert a["poses"].tobytes() == b["poses"].tobytes()
    assert np.array_equal(a["poses"][0], g["poses"][0]) and not np.allclose(a["poses"][1:], g["poses"][1:])
    assert np.allclose(np.linalg.norm(a["poses"][:, :4], axis=1), 1.0)


def test_invalid_steps_end_the_solve_at_the_start():
    """NaN measurements make every step non-finite: more than five invalid attempts in a row end
    the solve with its poses as given."""
    g = R.fixture("k5_l1")[0]
    g["edge_meas"][1, 5] = math.nan
    s = M.solve(g, "none", max_iter=20)
    assert s["outcome"] == [M.INVALID] * 6 and s["iterations"] == 6 and s["accepted"] == 0
    assert s["poses"].tobytes() == np.array([R.pose_unit(p) for p in g["poses"]]).tobytes()


# ----------------------------------------------------------------------------- the host side
def test_pgo_lm_defaults_and_bad_input():
    from ssf import _abi, loop
    p = loop.pgo_lm()
    assert (p.radius0, p.min_relative_decrease, p.max_radius, p.min_radius) == (1e4, 1e-3, 1e16, 1e-32)
    assert loop.pgo_lm(radius0=10.0).radius0 == 10.0 and loop.parse_lm(True).radius0 == 1e4
    assert loop.parse_lm("1e16").radius0 == 1e16
    for kw in (dict(radius0=0.0), dict(radius0=-1.0), dict(radius0=math.nan), dict(max_radius=math.inf),
               dict(min_radius=0.0), dict(min_radius=1.0, max_radius=0.5), dict(min_relative_decrease=-0.1),
               dict(min_relative_decrease=1.0), dict(min_relative_decrease=math.nan), dict(radius0="x")):
        with pytest.raises(ValueError):
            loop.pgo_lm(**kw)
    for text in ("", "big", "0", "-3", "nan"):
        with pytest.raises(ValueError):
            loop.parse_lm(text)
    assert _abi.lib().ssf_pgo_lm_default(None) == _abi.SSF_E_ARG
    assert _abi.PGO_OUT["ACCEPTED"] == 6 and _abi.PGO_OUT["RADIUS"] == 7 and _abi.PGO_OUT_STRIDE == 8
    assert C.sizeof(_abi.PgoLm) == 32
    with pytest.raises(ValueError, match="lm_log"):
        loop.optimize_pose_graphs(None, [R.fixture("k5_l1")[0]], lm_log=True)


def test_new_entry_point_rejects_a_null_context():
    from ssf import _abi, loop
    prm, lm = loop.pgo_params(), loop.pgo_lm()
    assert _abi.lib().ssf_pose_graph_batch_lm(None, None, 1, *([None] * 10), C.byref(prm), None, None, None, None,
                                              C.byref(lm), None) == _abi.SSF_E_ARG


def test_cli_rejects_bad_map_lm(tmp_path, capsys):
    from ssf import run
    base = [str(tmp_path), "--map-tum", "m.txt"]
    for argv, msg in ((base + ["--map-lm"], "--map-optimize"),
                      (base + ["--map-lm=1e3"], "--map-optimize"),
                      (base + ["--map-iters", "30"], "--map-optimize"),
                      (base + ["--map-optimize", "--map-lm=0"], "positive"),
                      (base + ["--map-optimize", "--map-lm=-2"], "positive"),
                      (base + ["--map-optimize", "--map-lm=huge"], "number"),
                      (base + ["--map-optimize", "--map-iters", "0"], "positive"),
                      (base + ["--map-optimize", "--map-lm", "--map-iters", "-4"], "positive")):
        with pytest.raises(SystemExit) as e:
            run.main(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, argv


def test_nodes_reject_map_lm_without_optimize(tmp_path):
    from ssf import loop, nodes
    with pytest.raises(ValueError, match="map_optimize"):
        nodes.run_sequence(str(tmp_path), None, launch="onlyPC", map_tum_path="", map_lm=loop.pgo_lm())
    with pytest.raises(ValueError, match="map_optimize"):
        nodes.run_sequence(str(tmp_path), None, launch="onlyPC", map_tum_path="", map_iters=30)
    with pytest.raises(ValueError, match="positive"):
        nodes.run_sequence(str(tmp_path), None, launch="onlyPC", map_tum_path="", map_optimize=True, map_iters=0)

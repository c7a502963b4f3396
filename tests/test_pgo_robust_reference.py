"""The premises of the robust pose-graph tests, on the CPU: the yardstick of
tests/pgo_robust_reference.py restates the loss table of include/ssf_frontend.h, reduces to
tests/pgo_reference.py without a loss and does what a robust loss is for; the host side of the
new option rejects bad input before any GPU work."""
import ctypes as C
import math

import numpy as np
import pytest

import pgo_reference as R
import pgo_robust_reference as Q

CORRUPTED = (3, 17, 30)            # positions in the loop list of the 40-node / 33-loop graph


@pytest.mark.parametrize("name", ["k5_l1", "k12_l3", "k40_l32"])
def test_kind_none_is_the_plain_yardstick_bitwise(name):
    g, ref = R.fixture(name)
    got = Q.solve(g, "none")
    assert got["status"] == ref["status"] and got["iterations"] == ref["iterations"]
    assert got["poses"].tobytes() == ref["poses"].tobytes()
    assert got["cost_log"] == ref["cost_log"]
    assert np.array_equal(got["edge_weight"], np.ones(len(g["edge_ij"])))
    # the reported s are those of the last evaluation: with the prior's they give the cost
    total = got["edge_chi2"].sum() + Q.prior_chi2(g, got["poses"])
    assert abs(total - 2 * got["cost"]) <= 1e-12 * max(total, R.cost_floor(g))


@pytest.mark.parametrize("kind", Q.KINDS)
def test_loss_table(kind):
    k = Q.DEFAULT_K[kind] or 1.0
    assert Q.DEFAULT_K == dict(none=0.0, huber=1.345, cauchy=0.1, geman_mcclure=1.0)
    assert Q.weight(kind, k, 0.0) == 1.0 and Q.rho2(kind, k, 0.0) == 0.0
    # d(2 rho)/ds = w: central differences, step h = 1e-6 s, truncation ~ h^2 rho''' and rounding
    # ~ eps / 1e-6: 1e-8 relative covers both
    for s in (1e-3, 0.25 * k * k, 0.99 * k * k, 1.01 * k * k, 4.0 * k * k, 100.0, 1e4):
        h = 1e-6 * s
        d = (Q.rho2(kind, k, s + h) - Q.rho2(kind, k, s - h)) / (2 * h)
        assert abs(d - Q.weight(kind, k, s)) <= 1e-8 * max(1.0, Q.weight(kind, k, s)), (kind, s)
        assert 0.0 < Q.weight(kind, k, s) <= 1.0 and Q.rho2(kind, k, s) <= s
    if kind == "huber":                        # continuous, with a continuous weight, at e = k
        s0 = k * k
        lo, hi = np.nextafter(s0, 0.0), np.nextafter(s0, np.inf)
        assert abs(Q.rho2(kind, k, hi) - Q.rho2(kind, k, lo)) <= 4 * np.finfo(np.float64).eps * s0
        assert Q.rho2(kind, k, lo) == lo and Q.weight(kind, k, lo) == 1.0
        assert abs(Q.weight(kind, k, hi) - 1.0) <= 4 * np.finfo(np.float64).eps
        assert abs(Q.weight(kind, k, 4 * s0) - 0.5) <= 1e-15                 # e = 2 k: w = 1 / 2,
        assert abs(Q.rho2(kind, k, 4 * s0) - 3 * s0) <= 1e-15 * s0           # 2 rho = 2 k (2 k - k / 2)


def _corrupted40():
    return Q.cached("g40", lambda: Q.corrupt_loops(Q.graph40(), CORRUPTED))


def _solved40(kind):
    return Q.cached(("s40", kind), lambda: Q.solve(_corrupted40()[0], kind))


def test_huber_halves_the_damage_of_three_false_loops():
    g, bad = _corrupted40()
    assert len(g["poses"]) == 40 and len(Q.loop_edges(g)) == 33 and len(bad) == 3
    plain, huber = _solved40("none"), _solved40("huber")
    assert plain["status"] in (R.OK, R.CONVERGED) and huber["status"] in (R.OK, R.CONVERGED)
    d_plain = Q.distance_to_ground_truth(plain["poses"], g["gt"])
    d_huber = Q.distance_to_ground_truth(huber["poses"], g["gt"])
    print(f"distance to ground truth: plain {d_plain:.3f} m, huber {d_huber:.3f} m")
    assert d_huber < 0.5 * d_plain


def test_corrupted_edges_get_the_smallest_weights():
    g, bad = _corrupted40()
    w = _solved40("huber")["edge_weight"]
    clean = [e for e in range(len(w)) if e not in bad]
    print("corrupted", w[bad], "smallest clean", w[clean].min())
    assert w[bad].max() < w[clean].min()
    chain = [e for e in range(len(w)) if e not in Q.loop_edges(g)]
    assert np.array_equal(w[chain], np.ones(len(chain)))


def test_pgo_robust_rejects_bad_input():
    from ssf import _abi, loop
    for kind, k in (("huber", 1.345), ("cauchy", 0.1), ("geman_mcclure", 1.0), ("none", 0.0)):
        r = loop.pgo_robust(kind)
        assert (r.kind, r.k) == (_abi.PGO_ROBUST_KINDS[kind], k)
    r = loop.pgo_robust("huber", 2.5)
    assert (r.kind, r.k) == (_abi.PGO_ROBUST_HUBER, 2.5)
    for kind, k in (("tukey", None), ("", None), (1, None), (None, None), ("huber", 0.0), ("huber", -1.0),
                    ("cauchy", math.nan), ("geman_mcclure", math.inf), ("huber", "x")):
        with pytest.raises(ValueError):
            loop.pgo_robust(kind, k)
    assert loop.parse_robust("cauchy:0.5").k == 0.5 and loop.parse_robust("huber").k == 1.345
    for text in ("huber:", "huber:0", "huber:nan", "welsch", ":1"):
        with pytest.raises(ValueError):
            loop.parse_robust(text)
    out = _abi.PgoRobust()
    L = _abi.lib()
    assert L.ssf_pgo_robust_default(7, C.byref(out)) == _abi.SSF_E_ARG
    assert L.ssf_pgo_robust_default(-1, C.byref(out)) == _abi.SSF_E_ARG
    assert L.ssf_pgo_robust_default(_abi.PGO_ROBUST_HUBER, None) == _abi.SSF_E_ARG


def test_cli_rejects_bad_map_robust(tmp_path, capsys):
    from ssf import run
    for argv, msg in (([str(tmp_path), "--map-tum", "m.txt", "--map-robust", "huber"], "--map-optimize"),
                      ([str(tmp_path), "--map-tum", "m.txt", "--map-optimize", "--map-robust", "tukey"], "kind"),
                      ([str(tmp_path), "--map-tum", "m.txt", "--map-optimize", "--map-robust", "huber:-1"], "positive")):
        with pytest.raises(SystemExit) as e:
            run.main(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, argv


def test_nodes_reject_map_robust_without_optimize(tmp_path):
    from ssf import loop, nodes
    with pytest.raises(ValueError, match="map_optimize"):
        nodes.run_sequence(str(tmp_path), None, launch="onlyPC", map_tum_path="", map_robust=loop.pgo_robust("huber"))


def test_new_entry_point_rejects_a_null_context():
    from ssf import _abi, loop
    L = _abi.lib()
    prm, rb = loop.pgo_params(), loop.pgo_robust("huber")
    assert L.ssf_pose_graph_batch_robust(None, None, 1, *([None] * 10), C.byref(prm), None, None,
                                         C.byref(rb), None) == _abi.SSF_E_ARG
    assert L.ssf_pose_graph_batch_robust(None, None, 0, *([None] * 10), C.byref(prm), None, None,
                                         None, None) == _abi.SSF_E_ARG

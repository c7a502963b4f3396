"""Pose graphs with more than 32 loop edges, CPU side: the constants of the header, the Python
ABI and the kernel source agree; the Python entry treats ragged input as before; and the
premises of tests/test_gpu_pose_graph_wide.py hold for the numpy yardstick (which graphs take
the wide path, which have a clear stop rule)."""
import os
import re

import numpy as np
import pytest

import pgo_reference as R
import pgo_wide_fixtures as W

ROOT = os.path.join(os.path.dirname(__file__), "..")


def test_loop_cap_constants_agree():
    from ssf import _abi
    L = _abi.lib()
    assert L.ssf_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "ssf_frontend.h")).read()
    assert _abi.PGO_MAX_LOOPS == 256
    assert f"#define SSF_PGO_MAX_LOOPS {_abi.PGO_MAX_LOOPS}" in hdr
    assert f"#define SSF_PGO_OUT_STRIDE {_abi.PGO_OUT_STRIDE}" in hdr
    assert f"#define SSF_PGO_MAX_ITER {_abi.PGO_MAX_ITER}" in hdr
    csrc = os.path.join(ROOT, "ssf-slam_amd", "csrc")           # the kernel source: pose_graph.hip and its stage headers
    src = open(os.path.join(csrc, "pose_graph.hip")).read()
    stages = re.findall(r'#include "(pgo_\w+\.hpp)"', src)
    assert stages
    src += "".join(open(os.path.join(csrc, h)).read() for h in stages)
    m = re.search(r"constexpr int kPgoNarrowLoops = (\d+);", src)
    assert m and int(m.group(1)) == W.NARROW_LOOPS == 32
    assert "L > SSF_PGO_MAX_LOOPS" in src                # the kernel's cap is the header's
    # the failure test of test_gpu_pose_graph.py builds PGO_MAX_LOOPS + 1 distinct loops on 40 nodes
    assert _abi.PGO_MAX_LOOPS + 1 <= 39 * 38


def test_python_entry_rejects_ragged_wide_graph():
    from ssf import loop
    g, _ = W.wide_fixture("k40_l33")
    g["edge_meas"] = g["edge_meas"][:-1]
    with pytest.raises(ValueError, match="differ in length"):
        loop.optimize_pose_graphs(None, [R.fixture("k5_l1")[0], g])
    g, _ = W.wide_fixture("k40_l33")
    g["prior_var"] = g["prior_var"][:-1]
    with pytest.raises(ValueError):
        loop.optimize_pose_graphs(None, [g])
    assert loop.optimize_pose_graphs(None, []) == []


def test_wide_fixtures_take_the_wide_path():
    want = {"k40_l33": (40, 33), "k40_l42": (40, 42), "k40_l43": (40, 43), "k60_l85": (60, 85),
            "k60_l86": (60, 86), "k60_l170": (60, 170), "k60_l171": (60, 171), "k40_l256": (40, 256),
            "k300_l40": (300, 40), "k40_l50_rev_dup": (40, 50), "k40_l20_dup14": (40, 20)}
    assert set(want) == set(W.WIDE)
    for name, (K, L) in want.items():
        g, _ = W.wide_fixture(name)
        assert (len(g["poses"]), W.true_loops(g)) == (K, L), name
        assert W.extra_edges(g) > W.NARROW_LOOPS, name
        assert len({(int(i), int(j)) for i, j in g["edge_ij"] if abs(int(i) - int(j)) != 1}) == L, name
    g, _ = W.wide_fixture("k40_l20_dup14")               # wide by its edge count only
    assert W.true_loops(g) <= W.NARROW_LOOPS < W.extra_edges(g) == 34
    g, _ = W.wide_fixture("k40_l50_rev_dup")
    chain = [(int(i), int(j)) for i, j in g["edge_ij"] if abs(int(i) - int(j)) == 1]
    assert (8, 7) in chain and (31, 30) in chain and chain.count((12, 13)) == 2 and chain.count((13, 14)) == 2
    # 6 L + 1 right-hand sides on both sides of 256, 512 and 1024
    cols = sorted(6 * L + 1 for _, L in want.values())
    for edge in (256, 512, 1024):
        assert any(edge - 6 < c <= edge for c in cols) and any(edge < c <= edge + 6 for c in cols), edge


@pytest.mark.parametrize("prior", ["tight", "ref"])
def test_wide_stop_rule_fixtures_are_far_from_the_tolerance(prior):
    """what the GPU test's iteration-count assertion relies on: every check of these graphs is
    decided by a factor of at least 100, so rounding cannot move the iteration count"""
    for name in W.WIDE_STOP_RULE:
        g, s = W.wide_fixture(name, prior)
        assert s["status"] == R.CONVERGED and s["cost"] > 1e6 * R.cost_floor(g), name
        assert 3 <= s["iterations"] <= 4, (name, s["iterations"])
        assert all(m >= 100 or m <= 0.01 for m in R.stop_margins(s["cost_log"])), (name, s["cost_log"])


@pytest.mark.parametrize("prior", ["tight", "ref"])
def test_fixed_iteration_fixtures_reduce_the_cost(prior):
    for name in W.WIDE:
        if name in W.WIDE_STOP_RULE:
            continue
        g, s = W.wide_fixture(name, prior)
        assert W.solve_params(name) == dict(max_iter=3, func_tol=0.0)
        assert s["status"] == R.OK and s["iterations"] == 3 and len(s["cost_log"]) == 4, name
        assert s["cost"] < s["cost0"] and s["cost"] > 1e6 * R.cost_floor(g), name


def test_wide_failure_graph_premises():
    """(40, 40) without chain link 8 - 9 still has more than 32 edges beyond K - 1, and more loop
    edges than that count: the wide kernel's prologue must answer NOT_PD"""
    g = R.circle_graph(40, loops=R.spread_loops(40, 40, 35), seed=35)
    keep = [e for e, (i, j) in enumerate(g["edge_ij"]) if {int(i), int(j)} != {8, 9}]
    assert len(keep) == len(g["edge_ij"]) - 1
    extra = len(keep) - 39
    assert extra == 39 > W.NARROW_LOOPS and W.true_loops(g) == 40 > extra
    assert np.isfinite(g["edge_meas"]).all() and g["edge_meas"].shape[0] > 51

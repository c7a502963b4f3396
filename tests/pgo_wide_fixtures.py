"""Graphs with more than 32 loop edges for the pose-graph tests (the wide path of
pose_graph.hip), built from tests/pgo_reference.py as it stands.  Shared by
test_pose_graph_wide_host.py (the premises, on the CPU) and test_gpu_pose_graph_wide.py."""
import pgo_reference as R

NARROW_LOOPS = 32          # up to here a graph is solved with a lane per right-hand side


def _spread(K, L, seed, **kw):
    return lambda pv: R.circle_graph(K, loops=R.spread_loops(K, L, seed), seed=seed, prior_var=pv, **kw)


# (K, L): 6 L + 1 right-hand sides straddle 256, 512 and 1024, the pass boundaries of any pass
# width that is a power of two up to 1024
WIDE = {
    "k40_l33": _spread(40, 33, 30),             # 199 columns: the first graph over the old cap
    "k40_l42": _spread(40, 42, 31),             # 253
    "k40_l43": _spread(40, 43, 32),             # 259
    "k60_l85": _spread(60, 85, 14),             # 511
    "k60_l86": _spread(60, 86, 15),             # 517
    "k60_l170": _spread(60, 170, 18),           # 1021
    "k60_l171": _spread(60, 171, 16),           # 1027
    "k40_l256": _spread(40, 256, 17),           # 1537: the cap, 1536 capacitance rows over the threads
    "k300_l40": _spread(300, 40, 30),           # 241: nodes strided over the threads
    # links 7 and 30 reversed, 12 and 13 given twice
    "k40_l50_rev_dup": _spread(40, 50, 33, reversed_edges=(7, 30), duplicated_edges=(12, 13)),
    # 20 true loops and 14 doubled chain links: 34 edges beyond K - 1, so the wide path by its
    # edge count, with L <= 32
    "k40_l20_dup14": _spread(40, 20, 34, duplicated_edges=tuple(range(3, 31, 2))),
}
# every stop check of the yardstick is decided by a factor of at least 100, under both priors
# (asserted on the CPU by test_pose_graph_wide_host.py)
WIDE_STOP_RULE = ("k60_l85", "k60_l86", "k60_l170", "k60_l171", "k40_l256", "k300_l40")
# the rest is compared after exactly three steps
FIXED_ITERATIONS = 3

_CACHE = {}


def wide_fixture(name, prior="tight"):
    """-> (graph, yardstick solution): at the default parameters for WIDE_STOP_RULE, after
    FIXED_ITERATIONS steps (func_tol 0) for the others.  Built once per process."""
    key = (name, prior)
    if key not in _CACHE:
        g = WIDE[name](R.TIGHT_PRIOR_VAR if prior == "tight" else R.REF_PRIOR_VAR)
        s = R.solve(g) if name in WIDE_STOP_RULE else R.solve(g, FIXED_ITERATIONS, 0.0)
        _CACHE[key] = (g, s)
    g, s = _CACHE[key]
    return R.copy_graph(g), s


def solve_params(name):
    """keyword arguments of loop.pgo_params for the run wide_fixture's solution belongs to"""
    return {} if name in WIDE_STOP_RULE else dict(max_iter=FIXED_ITERATIONS, func_tol=0.0)


def true_loops(g):
    return sum(1 for i, j in g["edge_ij"] if abs(int(i) - int(j)) != 1)


def extra_edges(g):
    """edges beyond the K - 1 of a chain: what the host sizes and dispatches by"""
    return len(g["edge_ij"]) - (len(g["poses"]) - 1)

"""Dense numpy f64 IRLS Gauss-Newton on SE(3) pose graphs with a robust loss on the loop edges:
the yardstick of ssf_pose_graph_batch_robust.  It restates the contract of include/ssf_frontend.h
on top of tests/pgo_reference.py (same residual, Jacobians, retraction and stop rule;
np.linalg.solve on J^T J).  Nothing in the package imports this file.

For an edge with whitened residual r, s = r^T r and e = sqrt(s); weight w and doubled loss
2 rho follow GTSAM's m-estimators on the whitened error norm:

    none             w = 1                      2 rho = s
    huber(k)         1 if e <= k else k / e     s if e <= k else 2 k (e - k / 2)       k = 1.345
    cauchy(k)        k^2 / (k^2 + s)            k^2 log1p(s / k^2)                      k = 0.1
    geman_mcclure(k) (k^2 / (k^2 + s))^2        k^2 s / (k^2 + s)                       k = 1.0

The loss applies to the loop edges (|i - j| != 1); chain edges and the prior stay quadratic.  At
each linearisation the six rows of a loop edge in r and J are multiplied by sqrt(w); the cost is
0.5 * (sum of s over the prior and the chain edges + sum of 2 rho over the loop edges)."""
import math

import numpy as np

import pgo_reference as R

KINDS = ("none", "huber", "cauchy", "geman_mcclure")
DEFAULT_K = dict(none=0.0, huber=1.345, cauchy=0.1, geman_mcclure=1.0)


def weight(kind, k, s):
    e = math.sqrt(s)
    if kind == "none":
        return 1.0
    if kind == "huber":
        return 1.0 if e <= k else k / e
    if kind == "cauchy":
        return k * k / (k * k + s)
    if kind == "geman_mcclure":
        return (k * k / (k * k + s)) ** 2
    raise ValueError(kind)


def rho2(kind, k, s):
    """2 rho(s)"""
    e = math.sqrt(s)
    if kind == "none":
        return s
    if kind == "huber":
        return s if e <= k else 2.0 * k * (e - 0.5 * k)
    if kind == "cauchy":
        return k * k * math.log1p(s / (k * k))
    if kind == "geman_mcclure":
        return k * k * s / (k * k + s)
    raise ValueError(kind)


def loop_edges(g):
    """indices of the loop edges: every edge with |i - j| != 1, in edge order"""
    return [e for e, (i, j) in enumerate(np.asarray(g["edge_ij"]).reshape(-1, 2)) if abs(int(i) - int(j)) != 1]


def solve(g, kind="none", k=None, max_iter=8, func_tol=1e-6):
    """The kernel's loop -> dict(poses, status, iterations, cost0, cost, cost_log, edge_weight [E],
    edge_chi2 [E]); the last two belong to the evaluation whose cost is `cost`."""
    k = DEFAULT_K[kind] if k is None else float(k)
    X = np.array([R.pose_unit(p) for p in np.asarray(g["poses"], np.float64).reshape(-1, 7)])
    E = len(g["edge_ij"])
    loops = loop_edges(g)
    log, status, iters = [], R.OK, 0
    for it in range(max_iter + 1):
        r, J = R.linearise(g, X)
        chi2 = np.array([float(r[6 * e:6 * e + 6] @ r[6 * e:6 * e + 6]) for e in range(E)])
        w = np.ones(E)
        extra = 0.0                                  # sum over the loop edges of 2 rho - s
        for e in loops:
            w[e] = weight(kind, k, chi2[e])
            extra += rho2(kind, k, chi2[e]) - chi2[e]
        # r @ r as pgo_reference.solve forms it, so that kind none reproduces it bit for bit (every
        # 2 rho - s is then exactly zero)
        cost = 0.5 * (float(r @ r) + extra)
        log.append(cost)
        if it == max_iter:
            break
        if it > 0 and func_tol > 0 and abs(log[-2] - cost) <= func_tol * log[-2]:
            status = R.CONVERGED
            break
        for e in loops:
            sw = math.sqrt(w[e])
            r[6 * e:6 * e + 6] *= sw
            J[6 * e:6 * e + 6] *= sw
        dx = np.linalg.solve(J.T @ J, -(J.T @ r)).reshape(-1, 6)
        X = np.array([R.retract(x, d) for x, d in zip(X, dx)])
        iters = it + 1
    return dict(poses=X, status=status, iterations=iters, cost0=log[0], cost=log[-1], cost_log=log,
                edge_weight=w, edge_chi2=chi2)


def corrupt_loops(g, which, seed=5, rot_sigma=0.3, trans_sigma=3.0):
    """A copy of g with the measurements of the loop edges number `which` (positions in the loop
    list, edge order) moved by seeded noise N(0, rot_sigma rad) / N(0, trans_sigma m) in the
    tangent: false closures.  -> (graph, edge indices of the corrupted loops)"""
    rng = np.random.default_rng(seed)
    out = R.copy_graph(g)
    loops = loop_edges(g)
    edges = [loops[l] for l in which]
    for e in edges:
        d = np.concatenate([rng.normal(0, rot_sigma, 3), rng.normal(0, trans_sigma, 3)])
        out["edge_meas"][e] = R.retract(R.pose_unit(out["edge_meas"][e]), d)
    return out, edges


def offset_loops(g, which, offset=(3.0, 0.0, 0.0)):
    """As corrupt_loops, with a fixed translation offset (metres, in the measurement's frame)."""
    out = R.copy_graph(g)
    loops = loop_edges(g)
    edges = [loops[l] for l in which]
    for e in edges:
        out["edge_meas"][e] = R.retract(R.pose_unit(out["edge_meas"][e]), np.concatenate([np.zeros(3), offset]))
    return out, edges


def distance_to_ground_truth(poses, gt):
    """largest translation distance of a node from its ground truth [m]"""
    return float(np.linalg.norm(np.asarray(poses)[:, 4:] - np.asarray(gt)[:, 4:], axis=1).max())


def prior_chi2(g, poses):
    """s of the prior factor at `poses`"""
    r = R.between_factor(R.IDENTITY, R.pose_unit(poses[0]), g["prior_pose"], g["prior_var"])[0]
    return float(r @ r)


def graph40():
    """the 40-node / 33-loop graph of the wide-kernel cases"""
    return R.circle_graph(40, R.spread_loops(40, 33, 0), seed=1)


_CACHE = {}


def cached(key, build):
    """build() once per process; the tests share the yardstick's solutions and leave them as
    they are"""
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]

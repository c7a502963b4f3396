"""Dense numpy f64 Levenberg-Marquardt on SE(3) pose graphs: the yardstick of
ssf_pose_graph_batch_lm.  It restates the step rule of include/ssf_frontend.h (Ceres'
LevenbergMarquardtStrategy) on top of tests/pgo_reference.py (residual, Jacobians, retraction) and
tests/pgo_robust_reference.py (the loss on the loop edges).  Nothing in the package imports this
file.

One attempt solves (H + diag(d) / radius) dx = -g with H = J^T J and g = J^T r over every factor
(the loop rows scaled by sqrt(w)), d = clip(diag(H), 1e-6, 1e32), by np.linalg.solve; a pivot
failure is what np.linalg.cholesky of that matrix reports.  mcc = -sum_e (r_e . v_e + v_e . v_e / 2),
v = J dx, is the decrease the model promises; the trial point X (+) dx is accepted when
rho = (cost - trial cost) / mcc > min_relative_decrease.  See solve() for the rest."""
import math

import numpy as np

import pgo_reference as R
import pgo_robust_reference as RR

REJECTED, ACCEPTED, INVALID = 0, 1, 2
DEFAULTS = dict(radius0=1e4, min_relative_decrease=1e-3, max_radius=1e16, min_radius=1e-32)


def evaluate(g, X, kind="none", k=None):
    """-> (cost, r, J, weight [E], chi2 [E]) at X: r and J with the loop rows scaled by sqrt(w),
    the cost with 2 rho on the loop edges (formed as pgo_robust_reference.solve forms it)."""
    k = RR.DEFAULT_K[kind] if k is None else float(k)
    E = len(g["edge_ij"])
    r, J = R.linearise(g, X)
    chi2 = np.array([float(r[6 * e:6 * e + 6] @ r[6 * e:6 * e + 6]) for e in range(E)])
    w = np.ones(E)
    extra = 0.0
    for e in RR.loop_edges(g):
        w[e] = RR.weight(kind, k, chi2[e])
        extra += RR.rho2(kind, k, chi2[e]) - chi2[e]
    cost = 0.5 * (float(r @ r) + extra)
    for e in RR.loop_edges(g):
        sw = math.sqrt(w[e])
        r[6 * e:6 * e + 6] *= sw
        J[6 * e:6 * e + 6] *= sw
    return cost, r, J, w, chi2


def cost_at(g, poses, kind="none", k=None):
    X = np.array([R.pose_unit(p) for p in np.asarray(poses, np.float64).reshape(-1, 7)])
    return evaluate(g, X, kind, k)[0]


def solve(g, kind="none", k=None, max_iter=8, func_tol=1e-6, radius0=1e4, min_relative_decrease=1e-3,
          max_radius=1e16, min_radius=1e-32):
    """The kernel's loop -> dict(poses (the last accepted point), status, iterations (attempts),
    accepted, radius, dx (max-norm of the last accepted step), cost0, cost, cost_log (the cost
    after every attempt, cost0 first), lm_log [attempts, 4] (trial cost, mcc, radius after the
    attempt, outcome), edge_weight, edge_chi2 (at the last accepted point), and per attempt
    rho (NaN for an invalid one), outcome, accept_clear (the accept decision holds by a factor
    of 10: rho >= 10 min_relative_decrease, or the trial raised the cost; None for an invalid
    attempt) and stop_margin ((prev - cost) / (func_tol prev) at the stop check of an accepted
    attempt, else None))."""
    X = np.array([R.pose_unit(p) for p in np.asarray(g["poses"], np.float64).reshape(-1, 7)])
    cost, r, J, w, chi2 = evaluate(g, X, kind, k)
    cost0, log = cost, [cost]
    radius, dec, invalid, accepted, status, dxmax = float(radius0), 2.0, 0, 0, R.OK, 0.0
    lm_log, rhos, outcomes, accept_clear, stop_margin = [], [], [], [], []
    attempts = 0
    for _ in range(max_iter):
        attempts += 1
        H = J.T @ J
        A = H + np.diag(np.clip(np.diag(H), 1e-6, 1e32) / radius)
        mcc, dx = math.nan, None
        try:
            np.linalg.cholesky(A)
            dx = np.linalg.solve(A, -(J.T @ r))
            if np.all(np.isfinite(dx)):
                v = J @ dx
                mcc = -float(r @ v + 0.5 * (v @ v))
        except np.linalg.LinAlgError:
            pass
        if not mcc > 0:                                    # invalid step
            radius /= dec
            dec *= 2
            log.append(cost)
            lm_log.append([math.nan, mcc, radius, INVALID])
            rhos.append(math.nan); outcomes.append(INVALID); accept_clear.append(None); stop_margin.append(None)
            invalid += 1
            if invalid > 5:
                break
            continue
        invalid = 0
        XT = np.array([R.retract(x, d) for x, d in zip(X, dx.reshape(-1, 6))])
        ct, rt, Jt, wt, chi2t = evaluate(g, XT, kind, k)
        rho = (cost - ct) / mcc
        rhos.append(rho)
        stop = False
        if rho > min_relative_decrease:
            prev = cost
            X, cost, r, J, w, chi2 = XT, ct, rt, Jt, wt, chi2t
            accepted += 1
            dxmax = float(np.abs(dx).max())
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), max_radius)
            dec = 2.0
            outcomes.append(ACCEPTED)
            accept_clear.append(bool(rho >= 10 * min_relative_decrease))
            stop_margin.append((prev - cost) / (func_tol * prev) if func_tol > 0 and prev > 0 else None)
            if func_tol > 0 and prev - cost <= func_tol * prev:
                status, stop = R.CONVERGED, True
        else:
            radius /= dec
            dec *= 2
            outcomes.append(REJECTED)
            accept_clear.append(bool(ct > cost) or not math.isfinite(ct))
            stop_margin.append(None)
        log.append(cost)
        lm_log.append([ct, mcc, radius, outcomes[-1]])
        if stop or radius < min_radius:
            break
    return dict(poses=X, status=status, iterations=attempts, accepted=accepted, radius=radius, dx=dxmax,
                cost0=cost0, cost=cost, cost_log=log, lm_log=np.array(lm_log, np.float64).reshape(-1, 4),
                edge_weight=w, edge_chi2=chi2, rho=rhos, outcome=outcomes, accept_clear=accept_clear,
                stop_margin=stop_margin)


def first_unclear(res, factor=10.0):
    """-> (attempt, "accept" | "stop") of the first decision of a run that does not hold by
    `factor`, or None: the device, whose sums round differently, takes the same path up to there"""
    for a, (c, m) in enumerate(zip(res["accept_clear"], res["stop_margin"]), start=1):
        if c is not None and not c:
            return a, "accept"
        if m is not None and 1.0 / factor < m < factor:
            return a, "stop"
    return None


def decisions_clear(res, factor=10.0):
    return first_unclear(res, factor) is None


def far_start(g, seed, rs, ts):
    """A copy of g with every node but the first moved in the tangent by N(0, rs rad) /
    N(0, ts m), nodes 1 .. K - 1 in order from np.random.default_rng(seed)."""
    rng = np.random.default_rng(seed)
    out = R.copy_graph(g)
    poses = np.array(out["poses"], np.float64).reshape(-1, 7)
    for i in range(1, len(poses)):
        poses[i] = R.retract(R.pose_unit(poses[i]), np.concatenate([rng.normal(0, rs, 3), rng.normal(0, ts, 3)]))
    out["poses"] = poses
    return out


# ------------------------------------------------------------------------------------ fixtures
def _small(K):
    if K == 6:
        return R.circle_graph(6, [(5, 0), (4, 1)], seed=2)
    return R.circle_graph(12, [(11, 0), (8, 2), (5, 10)], seed=3)


def far_small(K):
    """-> (far-start graph, the same graph at its unperturbed start): the K = 6 / K = 12 circles
    with loop 1 corrupted, far start seed 3, 1 rad / 5 m"""
    g, _ = RR.corrupt_loops(_small(K), [1])
    return far_start(g, 3, 1.0, 5.0), g


def far_wide40():
    """K = 40, L = 33 (the wide kernel), loops 0, 5, 9 corrupted, far start seed 2, 0.5 rad / 3 m"""
    g, _ = RR.corrupt_loops(RR.graph40(), [0, 5, 9])
    return far_start(g, 2, 0.5, 3.0), g


def far_wide43(prior_var=R.TIGHT_PRIOR_VAR):
    """K = 40, L = 43: 259 columns, two column passes of the wide kernel; far start as far_wide40"""
    g = R.circle_graph(40, R.spread_loops(40, 43, 0), seed=1, prior_var=prior_var)
    return far_start(g, 2, 0.5, 3.0), g


# the GPU parity cases: name -> (builder of the graph, kinds, radius0, max_iter); the tight prior,
# but for the names that end in _ref (mapOptmization's prior: the poses compare relative to node 0)
PARITY = {
    "far_k6": (lambda: far_small(6)[0], RR.KINDS, 1e16, 40),
    "far_k12": (lambda: far_small(12)[0], RR.KINDS, 1e16, 40),
    "far_wide40": (lambda: far_wide40()[0], RR.KINDS, 1e16, 30),
    "far_wide43": (lambda: far_wide43()[0], ("cauchy",), 1e16, 30),
    "far_wide43_ref": (lambda: far_wide43(R.REF_PRIOR_VAR)[0], ("cauchy",), 1e16, 30),
    "near_k12": (lambda: R.fixture("k12_l3")[0], ("none",), 1e4, 8),
    "near_k12_ref": (lambda: R.fixture("k12_l3", "ref")[0], ("none",), 1e4, 8),
    "near_wide40": (lambda: RR.graph40(), ("none",), 1e4, 8),
}


def parity_case(name, kind):
    """-> (graph, yardstick solution, parameters of that solve): solved once per process.  The stop
    rule is on (func_tol 1e-6) when every decision of the run is clear by a factor of 10.  A run
    whose first unclear decision is the stop check of attempt a is used with fixed attempts
    instead (func_tol 0, max_iter a: it ends where that check stood); one whose first unclear
    decision is the acceptance of attempt a ends before it (max_iter a - 1)."""
    def build():
        mk, _, radius0, max_iter = PARITY[name]
        g = mk()
        prm = dict(max_iter=max_iter, func_tol=1e-6, radius0=radius0)
        s = solve(g, kind, **prm)
        u = first_unclear(s)
        if u is not None:
            prm = dict(prm, max_iter=u[0], func_tol=0.0) if u[1] == "stop" else dict(prm, max_iter=u[0] - 1)
            s = solve(g, kind, **prm)
        return g, s, prm
    g, s, prm = RR.cached(("lm_parity", name, kind), build)
    return R.copy_graph(g), s, dict(prm)

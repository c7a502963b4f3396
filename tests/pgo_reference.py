"""Dense numpy f64 Gauss-Newton on SE(3) pose graphs: the yardstick of the GPU pose-graph
optimiser (ssf_pose_graph_batch).  Same residual, Jacobians, retraction and stop rule; the
linear solve is np.linalg.solve on J^T J.  Nothing in the package imports this file.

Poses are 7 doubles, q(x, y, z, w) then t; the tangent is (rotation, translation); the
retraction is X * [Exp(w), v].  A graph is a dict(poses [K, 7], edge_ij [E, 2], edge_meas
[E, 7], edge_var [E, 6], prior_pose [7], prior_var [6]).  The module also builds the fixtures
the tests share (drifting circles with inconsistent loops)."""
import math

import numpy as np

OK, CONVERGED, EMPTY, BAD_INPUT, TOO_MANY_LOOPS, NOT_PD = range(6)
REF_PRIOR_VAR = np.array([1e-2, 1e-2, math.pi ** 2, 1e8, 1e8, 1e8])      # mapOptmization.cpp:151
TIGHT_PRIOR_VAR = np.full(6, 1e-4)
ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])                  # :160


# ------------------------------------------------------------------------------- SE(3) helpers
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def quat_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def quat_log(q):
    q = np.asarray(q, np.float64)
    if q[3] < 0:
        q = -q
    n = np.linalg.norm(q[:3])
    k = 2.0 / q[3] if n < 1e-12 else 2.0 * math.atan2(n, q[3]) / n
    return k * q[:3]


def quat_exp(w):
    th = np.linalg.norm(w)
    if th < 1e-8:
        q = np.array([0.5 * w[0], 0.5 * w[1], 0.5 * w[2], 1.0])
    else:
        q = np.append(math.sin(0.5 * th) / th * np.asarray(w), math.cos(0.5 * th))
    return q / np.linalg.norm(q)


def jr_inv(phi):
    th = np.linalg.norm(phi)
    P = skew(phi)
    if th < 1e-8:
        return np.eye(3) + 0.5 * P
    c = 1.0 / th ** 2 - (1.0 + math.cos(th)) / (2.0 * th * math.sin(th))
    return np.eye(3) + 0.5 * P + c * (P @ P)


def pose_unit(p):
    p = np.array(p, np.float64)
    p[:4] /= np.linalg.norm(p[:4])
    return p


def pose_mul(a, b):
    """a * b for 7-vectors."""
    return np.concatenate([quat_mul(a[:4], b[:4]), a[4:] + quat_R(a[:4]) @ b[4:]])


def pose_inv(a):
    qc = quat_conj(a[:4])
    return np.concatenate([qc, -(quat_R(qc) @ a[4:])])


def pose_between(a, b):
    return pose_mul(pose_inv(a), b)


def retract(x, d):
    q = quat_mul(x[:4], quat_exp(d[:3]))
    return np.concatenate([q / np.linalg.norm(q), x[4:] + quat_R(x[:4]) @ d[3:]])


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def between_factor(xi, xj, z, var):
    """-> whitened (r [6], Ji [6, 6], Jj [6, 6]) of E = Z^-1 Xi^-1 Xj."""
    z = pose_unit(z)
    Ri, Rj, Rz = quat_R(xi[:4]), quat_R(xj[:4]), quat_R(z[:4])
    RM = Ri.T @ Rj
    tM = Ri.T @ (xj[4:] - xi[4:])
    RE = Rz.T @ RM
    tE = Rz.T @ (tM - z[4:])
    qe = quat_mul(quat_conj(z[:4]), quat_mul(quat_conj(xi[:4]), xj[:4]))
    phi = quat_log(qe / np.linalg.norm(qe))
    Jr = jr_inv(phi)
    w = 1.0 / np.sqrt(np.asarray(var, np.float64))
    Jj = np.zeros((6, 6))
    Jj[:3, :3] = Jr
    Jj[3:, 3:] = RE
    Ji = np.zeros((6, 6))
    Ji[:3, :3] = -Jr @ RM.T
    Ji[3:, :3] = Rz.T @ skew(tM)
    Ji[3:, 3:] = -Rz.T
    return np.concatenate([phi, tE]) * w, Ji * w[:, None], Jj * w[:, None]


def residual_only(xi, xj, z, var):
    return between_factor(xi, xj, z, var)[0]


def linearise(g, X):
    """-> (r [6 (E + 1)], J [6 (E + 1), 6 K]): the edges in order, then the prior."""
    K, E = len(X), len(g["edge_ij"])
    r = np.zeros(6 * (E + 1))
    J = np.zeros((6 * (E + 1), 6 * K))
    for e, (i, j) in enumerate(np.asarray(g["edge_ij"]).reshape(-1, 2)):
        re, Ji, Jj = between_factor(X[i], X[j], g["edge_meas"][e], g["edge_var"][e])
        r[6 * e:6 * e + 6] = re
        J[6 * e:6 * e + 6, 6 * i:6 * i + 6] = Ji
        J[6 * e:6 * e + 6, 6 * j:6 * j + 6] = Jj
    re, _, Jj = between_factor(IDENTITY, X[0], g["prior_pose"], g["prior_var"])
    r[6 * E:] = re
    J[6 * E:, 0:6] = Jj
    return r, J


def solve(g, max_iter=8, func_tol=1e-6):
    """The kernel's loop -> dict(poses, status, iterations, cost0, cost, cost_log)."""
    X = np.array([pose_unit(p) for p in np.asarray(g["poses"], np.float64).reshape(-1, 7)])
    log, status, iters = [], OK, 0
    for it in range(max_iter + 1):
        r, J = linearise(g, X)
        cost = 0.5 * float(r @ r)
        log.append(cost)
        if it == max_iter:
            break
        if it > 0 and func_tol > 0 and abs(log[-2] - cost) <= func_tol * log[-2]:
            status = CONVERGED
            break
        dx = np.linalg.solve(J.T @ J, -(J.T @ r)).reshape(-1, 6)
        X = np.array([retract(x, d) for x, d in zip(X, dx)])
        iters = it + 1
    return dict(poses=X, status=status, iterations=iters, cost0=log[0], cost=log[-1], cost_log=log)


def relative_to_first(P):
    P = np.asarray(P, np.float64).reshape(-1, 7)
    inv0 = pose_inv(pose_unit(P[0]))
    return np.array([pose_mul(inv0, pose_unit(p)) for p in P])


def pose_errors(a, b):
    """-> (max translation difference [m], max rotation angle between the poses [rad])."""
    a, b = np.asarray(a, np.float64).reshape(-1, 7), np.asarray(b, np.float64).reshape(-1, 7)
    dt = float(np.abs(a[:, 4:] - b[:, 4:]).max()) if len(a) else 0.0
    dr = 0.0
    for p, q in zip(a, b):
        dr = max(dr, float(np.linalg.norm(quat_log(quat_mul(quat_conj(pose_unit(p)[:4]), pose_unit(q)[:4])))))
    return dt, dr


# ------------------------------------------------------------------------------------ fixtures
def yaw_pose(x, y, z, yaw, roll=0.0, pitch=0.0):
    q = quat_mul(quat_mul(quat_exp([0, 0, yaw]), quat_exp([0, pitch, 0])), quat_exp([roll, 0, 0]))
    return np.concatenate([q, [x, y, z]])


def circle_graph(K, loops=(), seed=0, prior_var=TIGHT_PRIOR_VAR, radius=None, reversed_edges=(),
                 duplicated_edges=(), loop_var=0.05, loop_noise=0.05):
    """A full circle driven once (the yaw passes +-pi), odometry with drift, and `loops` (i, j)
    measured from the ground truth plus noise, so they disagree with the drifted odometry.
    reversed_edges: chain links k given as (k + 1 -> k); duplicated_edges: links given twice."""
    rng = np.random.default_rng(seed)
    radius = radius or max(5.0, K / 6.0)
    gt = []
    for k in range(K):
        a = 2 * math.pi * k / max(K, 1) * 0.98
        gt.append(yaw_pose(radius * math.cos(a), radius * math.sin(a), 0.1 * math.sin(3 * a), a + math.pi / 2,
                           0.02 * math.sin(a), 0.03 * math.cos(2 * a)))
    gt = np.array(gt).reshape(-1, 7)
    poses = [gt[0].copy()] if K else []
    ij, meas, var = [], [], []
    for k in range(K - 1):
        m = pose_between(gt[k], gt[k + 1])
        m = retract(m, np.concatenate([rng.normal(0, 2e-3, 3) + [0, 0, 1e-3], rng.normal(0, 2e-2, 3)]))
        poses.append(pose_mul(poses[-1], m))
        reps = 2 if k in duplicated_edges else 1
        for _ in range(reps):
            if k in reversed_edges:
                ij.append((k + 1, k)); meas.append(pose_inv(m))
            else:
                ij.append((k, k + 1)); meas.append(m)
            var.append(ODOM_VAR)
    for (i, j) in loops:
        m = retract(pose_between(gt[i], gt[j]),
                    np.concatenate([rng.normal(0, loop_noise * 0.2, 3), rng.normal(0, loop_noise, 3)]))
        ij.append((i, j)); meas.append(m); var.append(np.full(6, loop_var))
    return dict(poses=np.array(poses, np.float64).reshape(-1, 7),
                edge_ij=np.array(ij, np.int32).reshape(-1, 2),
                edge_meas=np.array(meas, np.float64).reshape(-1, 7),
                edge_var=np.array(var, np.float64).reshape(-1, 6),
                prior_pose=(gt[0].copy() if K else IDENTITY.copy()), prior_var=np.array(prior_var, np.float64),
                gt=gt)


def spread_loops(K, L, seed=0):
    """L distinct loop edges (i -> j), |i - j| >= 2, spread over a K-node chain."""
    rng = np.random.default_rng(1000 + seed)
    out = set()
    while len(out) < L:
        i, j = (int(v) for v in rng.integers(0, K, 2))
        if abs(i - j) >= 2:
            out.add((i, j))
    return sorted(out)


def copy_graph(g, **over):
    out = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    out.update(over)
    return out


# name -> builder(prior_var); the GPU tests and the host tests share these
def _k1(pv):
    return circle_graph(1, prior_var=pv)


def _k2(pv):
    g = circle_graph(2, prior_var=pv)
    g["edge_meas"][0] = pose_between(g["poses"][0], g["poses"][1])      # consistent: zero cost
    return g


def _k12(pv):
    # (11 -> 0) and (9 -> 2) overlap, (7 -> 4) is nested in both; link 5 reversed, link 2 doubled
    return circle_graph(12, loops=[(11, 0), (9, 2), (7, 4)], seed=3, prior_var=pv, reversed_edges=(5,),
                        duplicated_edges=(2,))


FIXTURES = {
    "k1": _k1,
    "k2": _k2,
    "k5_l1": lambda pv: circle_graph(5, loops=[(4, 0)], seed=1, prior_var=pv),
    "k12_l3": _k12,
    "k65_l0": lambda pv: circle_graph(65, seed=4, prior_var=pv),
    "k65_l1": lambda pv: circle_graph(65, loops=[(64, 0)], seed=5, prior_var=pv),
    "k65_l11": lambda pv: circle_graph(65, loops=spread_loops(65, 11, 23), seed=23, prior_var=pv),
    "k130_l0": lambda pv: circle_graph(130, seed=7, prior_var=pv),
    "k130_l1": lambda pv: circle_graph(130, loops=[(129, 1)], seed=8, prior_var=pv),
    "k130_l11": lambda pv: circle_graph(130, loops=spread_loops(130, 11, 9), seed=9, prior_var=pv),
    "k40_l32": lambda pv: circle_graph(40, loops=spread_loops(40, 32, 10), seed=10, prior_var=pv),
}
_CACHE = {}


def fixture(name, prior="tight"):
    """-> (graph, reference solution at the default parameters), built once per process."""
    key = (name, prior)
    if key not in _CACHE:
        g = FIXTURES[name](TIGHT_PRIOR_VAR if prior == "tight" else REF_PRIOR_VAR)
        _CACHE[key] = (g, solve(g))
    g, s = _CACHE[key]
    return copy_graph(g), s


# fixtures whose every stop check is at least 100x away from func_tol (asserted by the tests)
STOP_RULE_FIXTURES = ("k5_l1", "k12_l3", "k65_l11")


def cost_floor(g):
    """What rounding alone can put into a cost: each of the 6 (E + 1) whitened residuals carries
    an error of about 16 eps * max(1, |t|) / sigma_min, so a cost below
    0.5 * 6 (E + 1) * (that)^2 is zero as far as f64 can tell."""
    E = len(g["edge_ij"])
    P = np.asarray(g["poses"], np.float64).reshape(-1, 7)
    scale = max(1.0, float(np.abs(P[:, 4:]).max()) if len(P) else 1.0)
    var = np.concatenate([np.asarray(g["edge_var"], np.float64).reshape(-1), np.asarray(g["prior_var"], np.float64)])
    err = 16 * np.finfo(np.float64).eps * scale / math.sqrt(float(var.min()))
    return 0.5 * 6 * (E + 1) * err * err


def stop_margins(cost_log, func_tol=1e-6):
    """|cost_{k-1} - cost_k| / cost_{k-1} over func_tol at every stop check of a run (inf for a
    zero cost, where the check passes whatever the rounding)."""
    out = []
    for a, b in zip(cost_log[:-1], cost_log[1:]):
        out.append(abs(a - b) / a / func_tol if a > 0 else math.inf)
    return out

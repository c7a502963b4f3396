"""An independent yardstick for the registration stage (lidarOdometry_onlyPC.cpp:25-43, 74-82,
147-252): numpy float64 on the float32 values the device stores.  It shares no text with
oracle/ssf_oracle.c or the kernels and is built differently on purpose:

  * the Jacobian comes from forward-mode jets run through PlaneFeatureCost's own expressions,
    times EigenQuaternionParameterization's 4x3 Plus-Jacobian (what ceres::AutoDiffCostFunction
    and the parameterisation do), not from a hand-derived cross product;
  * the LM / GN steps are least-squares solutions of the (augmented) Jacobian system by
    np.linalg.lstsq, as DENSE_QR solves them, never the normal equations;
  * the plane fit is colPivHouseholderQr().solve() as mathematics (greedy pivoting, Eigen's rank
    rule, the basic solution), in float64.

Every decision a solver takes is logged with its margin (tested quantity / threshold), so a test
can tell a disagreement from a coin toss.  jacobian_self_check() compares the jets with central
differences through Plus.  Nothing here is tuned to what the code under test returns.
"""
import numpy as np

HUBER_A = 0.1
EPS32 = float(np.finfo(np.float32).eps)
# log statuses, as the device and the oracle number them
REJECTED, ACCEPTED, INVALID, PARAM_TOL, FUNC_TOL, GRAD_TOL, GN_STEP = 0, 1, 2, 3, 4, 5, 6


# ---------------------------------------------------------------------------- quaternions (xyzw)
def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def quat_rotate(q, v):
    """Eigen's _transformVector: uv = 2 qv x v;  v + w uv + qv x uv  (v [..., 3])"""
    qv = np.asarray(q[:3], np.float64)
    uv = 2.0 * np.cross(qv, v)
    return v + q[3] * uv + np.cross(qv, uv)


def plus(q, d):
    """EigenQuaternionParameterization::Plus: [sin|d| d/|d|, cos|d|] * q"""
    d = np.asarray(d, np.float64)
    nd = np.sqrt(np.dot(d, d))
    if not nd > 0.0:
        return np.array(q, np.float64)
    return quat_mul(np.r_[np.sin(nd) / nd * d, np.cos(nd)], q)


def plus_jacobian(q):
    """EigenQuaternionParameterization::ComputeJacobian, rows x, y, z, w"""
    x, y, z, w = q
    return np.array([[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]], np.float64)


def quat_angle(q1, q2):
    """rotation angle between two (not necessarily unit) quaternions"""
    a, b = np.asarray(q1) / np.linalg.norm(q1), np.asarray(q2) / np.linalg.norm(q2)
    v = quat_mul(a, quat_conj(b))
    return 2.0 * np.arctan2(np.linalg.norm(v[:3]), abs(v[3]))


def local_delta(q_a, t_a, q_b, t_b):
    """the 6-vector d with (q_a, t_a) ~ (Plus(q_b, d[:3]), t_b + d[3:]) for nearby poses"""
    a, b = np.asarray(q_a) / np.linalg.norm(q_a), np.asarray(q_b) / np.linalg.norm(q_b)
    v = quat_mul(a, quat_conj(b))
    if v[3] < 0:
        v = -v
    return np.r_[v[:3], np.asarray(t_a) - np.asarray(t_b)]


def compose(q0l, t0l, q, t):
    """publishResult (:87-90): q_0_curr = q_0_last q,  t_0_curr = t_0_last + q_0_last t"""
    return quat_mul(q0l, q), np.asarray(t0l, np.float64) + quat_rotate(np.asarray(q0l, np.float64),
                                                                       np.asarray(t, np.float64))


# ---------------------------------------------------------------------------- association
def transform_to_last(curr_xyz, q, t):
    """transformToLast (:74-82): double math, stored to float"""
    p = np.asarray(curr_xyz, np.float32).astype(np.float64)
    return (quat_rotate(np.asarray(q, np.float64), p) + np.asarray(t, np.float64)).astype(np.float32)


def associate(last, curr, q, t, valid=None):
    """Exact 1-NN of every transformed current point among last[:, :3], every last point
    considered: all m distances by the expanded form |L|^2 - 2 x . L in float64 (one matrix
    product) shortlist the three nearest, whose d2 are then recomputed as sum (x - L)^2; (d2, index)
    order.  The shortlist's error (2^-52 of |x|^2, 3e-9 m^2 at 5 km) cannot drop the winner of a
    pair whose gap the cases require to be >= 1e-3 relative, and a smaller gap shows in `gap`.
    Exact, then, for gap >= 1e-3 and for ties among at most three points: a tie among four or more
    (a lattice cell's centre) can leave the lowest index outside the shortlist of three --
    associate_exact() has no shortlist and is the yardstick there.
    -> (nn [c] int, gap [c]: (second-best d2 - best d2) / second-best d2, keep [c] bool)."""
    L = np.asarray(last, np.float32)[:, :3].astype(np.float64)
    s = transform_to_last(np.asarray(curr)[:, :3], q, t).astype(np.float64)
    c, m = len(s), len(L)
    if m == 0:                                   # an empty last frame: no neighbour, nothing kept
        return np.full(c, -1, np.int64), np.ones(c), np.zeros(c, bool)
    nn = np.zeros(c, np.int64)
    gap = np.ones(c)
    k = min(3, m)
    for lo in range(0, c, 1024):
        x = s[lo:lo + 1024]
        # candidates by the expanded form (one matrix product), then their exact d2
        approx = (L * L).sum(1)[None, :] - 2.0 * (x @ L.T)
        cand = np.argpartition(approx, k - 1, axis=1)[:, :k] if m > k else np.tile(np.arange(m), (len(x), 1))
        d2 = ((x[:, None, :] - L[cand]) ** 2).sum(-1)
        o = np.lexsort((cand, d2), axis=1)
        cand, d2 = np.take_along_axis(cand, o, 1), np.take_along_axis(d2, o, 1)
        nn[lo:lo + 1024] = cand[:, 0]
        if m > 1:
            gap[lo:lo + 1024] = np.where(d2[:, 1] > 0, (d2[:, 1] - d2[:, 0]) / np.where(d2[:, 1] > 0, d2[:, 1], 1.0), 0.0)
    keep = np.ones(c, bool) if valid is None else np.asarray(valid)[nn] != 0
    return nn, gap, keep


def associate_exact(last, curr, q, t, valid=None):
    """The 1-NN of :168 with nothing left out: the transformed query of transformToLast (:74-82,
    float32) and the last points (float32), both converted exactly to float64; every one of the
    c x m squared distances as sum (x - L)^2, never the expanded form; the winner the first of
    np.lexsort((index, d2)), so an exact tie of any multiplicity goes to the lowest index.
    Queries go in chunks of ~2e6 distances (m = 11 000 stays in memory).
    -> (nn [c] int, gap [c]: (second-best d2 - best d2) / second-best d2, 0 on a tie, keep [c])."""
    L = np.asarray(last, np.float32)[:, :3].astype(np.float64)
    s = transform_to_last(np.asarray(curr)[:, :3], q, t).astype(np.float64)
    c, m = len(s), len(L)
    if m == 0:
        return np.full(c, -1, np.int64), np.ones(c), np.zeros(c, bool)
    nn = np.zeros(c, np.int64)
    gap = np.ones(c)
    step = max(1, 2_000_000 // m)
    for lo in range(0, c, step):
        x = s[lo:lo + step]
        d2 = ((x[:, None, :] - L[None, :, :]) ** 2).sum(-1)
        index = np.broadcast_to(np.arange(m), d2.shape)
        order = np.lexsort((index, d2), axis=1)
        nn[lo:lo + step] = order[:, 0]
        if m > 1:
            rows = np.arange(len(x))
            first, second = d2[rows, order[:, 0]], d2[rows, order[:, 1]]
            gap[lo:lo + step] = np.where(second > 0, (second - first) / np.where(second > 0, second, 1.0), 0.0)
    keep = np.ones(c, bool) if valid is None else np.asarray(valid)[nn] != 0
    return nn, gap, keep


# ---------------------------------------------------------------------------- plane table
def intensity_row(f):
    """:181-183: int i = int(f); int row = 100 * (f - i + 0.002)  (f - i in float, then double)"""
    f = np.float32(f)
    i = int(f)
    return int(100.0 * (float(np.float32(f - np.float32(i))) + 0.002))


def plane_pick(last, a):
    """:173-205 for last-frame point a -> dict(pick [5] (or None when fewer than 5 neighbours),
    n (the gated rank), d2n, gap45, gap_n (relative d2 gaps between ranks 4|5 and n|n+1),
    gate_gap |d2[n] - 1|, other (other-row points taken))."""
    L = np.asarray(last, np.float32)
    X = L[:, :3].astype(np.float64)
    d2 = ((X - X[a]) ** 2).sum(1)
    order = np.lexsort((np.arange(len(X)), d2))[:30]
    d = d2[order]
    if len(order) < 5:
        return dict(pick=None, n=5, d2n=np.inf, gap45=1.0, gap_n=1.0, gate_gap=np.inf, other=0)
    v5, vr, n = list(order[:5]), [], 5
    p_row = intensity_row(L[order[0], 3])
    for ik in range(5, len(order)):
        row = intensity_row(L[order[ik], 3])
        if row != p_row and 0 <= row <= 63:
            vr.append(order[ik])
            n = ik
            if len(vr) >= 2:
                break
    if len(vr) == 1:
        v5[4] = vr[0]
    if len(vr) == 2:
        v5[3], v5[4] = vr
    rel = lambda i: (d[i + 1] - d[i]) / d[i + 1] if i + 1 < len(d) and d[i + 1] > 0 else 1.0  # noqa: E731
    d2n = d[n] if n < len(d) else np.inf
    return dict(pick=np.array(v5), n=n, d2n=d2n, gap45=rel(4), gap_n=min(rel(n - 1), rel(n)) if n < len(d) else 1.0,
                gate_gap=abs(d2n - 1.0), other=len(vr))


def plane_fit5(A, plane_max):
    """matA0.colPivHouseholderQr().solve(-1), normalize(), the four consecutive-difference tests
    (:208-232) for the 5x3 float32 matrix A -> dict(normal, rank, valid, x (the un-normalised
    solution), kappa, margin = min | |dd| - plane_max |, pivots)."""
    A = np.asarray(A, np.float32).astype(np.float64)
    R = A.copy()
    b = -np.ones(5)
    perm = [0, 1, 2]
    piv = []
    rank = 0
    for k in range(3):
        nrm = np.sqrt((R[k:, k:] ** 2).sum(0))
        j = k + int(np.argmax(nrm))
        R[:, [k, j]] = R[:, [j, k]]
        perm[k], perm[j] = perm[j], perm[k]
        x = R[k:, k].copy()
        alpha = np.sqrt(x @ x)
        piv.append(alpha)
        # Eigen's rank(): a pivot counts while |pivot| > eps * |max pivot| * min(rows, cols)
        if not alpha > EPS32 * piv[0] * 3.0 or alpha == 0.0:
            break
        rank = k + 1
        v = x.copy()
        v[0] += alpha if x[0] >= 0 else -alpha
        v /= np.sqrt(v @ v)
        R[k:, k:] -= 2.0 * np.outer(v, v @ R[k:, k:])
        b[k:] -= 2.0 * v * (v @ b[k:])
    x = np.zeros(3)
    if rank:
        z = np.linalg.solve(np.triu(R[:rank, :rank]), b[:rank])
        for i in range(rank):
            x[perm[i]] = z[i]
    n = x.copy()
    zz = n @ n
    if zz > 0:
        n = n / np.sqrt(zz)
    dd = np.abs((A[:4] - A[1:5]) @ n)
    sv = np.linalg.svd(A, compute_uv=False)
    return dict(normal=n, rank=rank, valid=bool(np.all(dd <= plane_max)), x=x,
                kappa=sv[0] / sv[2] if sv[2] > 0 else np.inf,
                margin=float(np.min(np.abs(dd - plane_max))), pivots=np.array(piv))


# ---------------------------------------------------------------------------- jets
class Jet:
    """value [N] and its 7 ambient partials [N, 7] (q x y z w, t x y z): what ceres::Jet<double, 7>
    carries through a templated functor"""

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def const(v):
        v = np.asarray(v, np.float64)
        return Jet(v, np.zeros(v.shape + (7,)))

    @staticmethod
    def param(x, k, n):
        d = np.zeros((n, 7))
        d[:, k] = 1.0
        return Jet(np.full(n, float(x)), d)

    def __add__(self, o):
        return Jet(self.v + o.v, self.d + o.d)

    def __sub__(self, o):
        return Jet(self.v - o.v, self.d - o.d)

    def __mul__(self, o):
        return Jet(self.v * o.v, self.d * o.v[:, None] + o.d * self.v[:, None])


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _po_last(po, q, t):
    """q_last_curr * po_curr + t_last_curr (:36-39) over jets; Eigen's product with a vector is
    _transformVector"""
    n = len(po)
    qj = [Jet.param(q[k], k, n) for k in range(4)]
    tj = [Jet.param(t[k], 4 + k, n) for k in range(3)]
    p = [Jet.const(po[:, k]) for k in range(3)]
    qv, w = qj[:3], qj[3]
    uv = _cross(qv, p)
    uv = [u + u for u in uv]
    c2 = _cross(qv, uv)
    return [p[k] + w * uv[k] + c2[k] + tj[k] for k in range(3)]


def _huber(s):
    """ceres::HuberLoss(0.1)::Evaluate -> rho, rho'; rho'' <= 0 everywhere"""
    b = HUBER_A * HUBER_A
    r = np.sqrt(np.where(s > b, s, 1.0))
    rho0 = np.where(s > b, 2.0 * HUBER_A * r - b, s)
    rho1 = np.where(s > b, np.maximum(np.finfo(np.float64).tiny, HUBER_A / r), 1.0)
    return rho0, rho1


def evaluate(po, pa, n, q, t, edges=None):
    """-> (cost, J [rows, 6], r [rows]) of the problem frameRegistration builds: one
    PlaneFeatureCost block per correspondence, autodiff by jets, local Jacobian by the
    parameterisation, ceres::Corrector with rho'' <= 0 (residual and Jacobian times sqrt(rho')),
    every block twice (:160).  edges = (po, c, u): the project's point-to-line blocks
    e = (I - u u^T)(R po + t - c), a 3-vector residual under one Huber on |e|^2."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    G = np.zeros((7, 6))
    G[:4, :3] = plus_jacobian(q)
    G[4:, 3:] = np.eye(3)
    Js, rs, cost = [], [], 0.0
    po, pa, n = (np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3) for x in (po, pa, n))
    if len(po):
        pl = _po_last(po, q, t)
        res = _dot([pl[k] - Jet.const(pa[:, k]) for k in range(3)], [Jet.const(n[:, k]) for k in range(3)])
        rho0, rho1 = _huber(res.v * res.v)
        w = np.sqrt(rho1)
        cost += 0.5 * rho0.sum()
        Js.append((res.d @ G) * w[:, None])
        rs.append(res.v * w)
    if edges is not None and len(edges[0]):
        epo, ec, eu = (np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3) for x in edges)
        pl = _po_last(epo, q, t)
        d = [pl[k] - Jet.const(ec[:, k]) for k in range(3)]
        u = [Jet.const(eu[:, k]) for k in range(3)]
        ud = _dot(u, d)
        e = [d[k] - u[k] * ud for k in range(3)]
        s = sum(x.v * x.v for x in e)
        rho0, rho1 = _huber(s)
        w = np.sqrt(rho1)
        cost += 0.5 * rho0.sum()
        Js.append(np.stack([(x.d @ G) * w[:, None] for x in e], 1).reshape(-1, 6))
        rs.append(np.stack([x.v * w for x in e], 1).reshape(-1))
    if not Js:
        return 0.0, np.zeros((0, 6)), np.zeros(0)
    J, r = np.concatenate(Js), np.concatenate(rs)
    return 2.0 * cost, np.concatenate([J, J]), np.concatenate([r, r])


def jacobian_self_check(po, pa, n, q, t, edges=None, h=1e-6):
    """largest |J_jets - J_central-differences| relative to the largest |J| (differences of the
    corrected residual through Plus with the Huber weight held, as Ceres holds it)"""
    _, J0, _ = evaluate(po, pa, n, q, t, edges)
    if not len(J0):
        return 0.0
    num = np.zeros_like(J0)
    w = _weights(po, pa, n, q, t, edges)      # sqrt(rho') of each row at (q, t), held
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rp = _raw_residual(po, pa, n, plus(q, d[:3]), np.asarray(t) + d[3:], edges)
        rm = _raw_residual(po, pa, n, plus(q, -d[:3]), np.asarray(t) - d[3:], edges)
        num[:, k] = w * (rp - rm) / (2 * h)
    return float(np.abs(num - J0).max() / max(np.abs(J0).max(), 1e-300))


def _raw_residual(po, pa, n, q, t, edges):
    """plain (no jets, no loss) residual rows in evaluate()'s row order"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    out = []
    po, pa, n = (np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3) for x in (po, pa, n))
    R = np.stack([quat_rotate(q, e) for e in np.eye(3)], 1)      # columns: rotated basis vectors
    if len(po):
        out.append((((po @ R.T) + t - pa) * n).sum(1))
    if edges is not None and len(edges[0]):
        epo, ec, eu = (np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3) for x in edges)
        d = (epo @ R.T) + t - ec
        out.append((d - eu * (eu * d).sum(1, keepdims=True)).reshape(-1))
    r = np.concatenate(out) if out else np.zeros(0)
    return np.concatenate([r, r])


def _weights(po, pa, n, q, t, edges):
    r = _raw_residual(po, pa, n, q, t, edges)
    half = len(r) // 2
    nb = len(np.asarray(po).reshape(-1, 3))
    w = np.ones(half)
    w[:nb] = np.sqrt(_huber(r[:nb] ** 2)[1])
    if half > nb:
        s = (r[nb:half].reshape(-1, 3) ** 2).sum(1)
        w[nb:] = np.repeat(np.sqrt(_huber(s)[1]), 3)
    return np.concatenate([w, w])


# ---------------------------------------------------------------------------- solvers
def _ratio(x, thr):
    if thr == 0.0:
        return 0.0 if x == 0.0 else np.inf
    return float(x / thr)


def _row(q, t, cost, status, radius):
    return np.r_[q, t, cost, status, radius]


def solve_lm(po, pa, n, q0, t0, max_iter=8, edges=None):
    """Ceres 1.14 TrustRegionMinimizer + LevenbergMarquardtStrategy with the options of :244-247
    (initial radius 1e4, max 1e16, min/max diagonal 1e-6 / 1e32, min relative decrease 1e-3,
    function / parameter / gradient tolerance 1e-6 / 1e-8 / 1e-10, Jacobi scaling
    1 / (1 + sqrt(column norm^2)) taken once, at most 5 consecutive invalid steps), the step the
    least-squares solution of [J S; sqrt(D / radius)] y = [-r; 0].
    -> dict(q, t, log [rows, 10] (q, t, cost, status, radius), margins [rows] of dicts
    (mcc, step, fcost, rho, grad: tested quantity / threshold, NaN where not tested), rank,
    J (at the final pose), grad0 (the gradient max-norm at the start))."""
    q, t = np.array(q0, np.float64), np.array(t0, np.float64)
    cost, J, r = evaluate(po, pa, n, q, t, edges)
    rank = int(np.linalg.matrix_rank(J)) if len(J) else 0
    S = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    radius, dec, invalid = 1e4, 2.0, 0
    log, margins = [], []

    def gradient_max_norm(qq, g):
        return max(np.abs(qq - plus(qq, -g[:3])).max(), np.abs(g[3:]).max())

    grad0 = gradient_max_norm(q, J.T @ r)
    for _ in range(max_iter):
        mg = dict(mcc=np.nan, step=np.nan, fcost=np.nan, rho=np.nan, grad=np.nan)
        Jsc = J * S
        D = np.sqrt(np.clip((Jsc * Jsc).sum(0), 1e-6, 1e32) / radius)
        y = np.linalg.lstsq(np.concatenate([Jsc, np.diag(D)]), np.r_[-r, np.zeros(6)], rcond=None)[0]
        Jy = Jsc @ y
        mcc = -float(Jy @ (r + 0.5 * Jy))
        # mcc > 0 is decided against the rounding of its two terms, ~2^-52 cost each
        mg["mcc"] = _ratio(mcc, 2.0 ** -40 * cost)
        if not mcc > 0.0:
            radius /= dec
            dec *= 2.0
            log.append(_row(q, t, cost, INVALID, radius)); margins.append(mg)
            invalid += 1
            if invalid > 5:
                break
            continue
        invalid = 0
        delta = y * S
        qc, tc = plus(q, delta[:3]), t + delta[3:]
        cc, Jc, rc = evaluate(po, pa, n, qc, tc, edges)
        xn = np.sqrt(q @ q + t @ t)
        sn = np.sqrt(((q - qc) ** 2).sum() + ((t - tc) ** 2).sum())
        mg["step"] = _ratio(sn, 1e-8 * (xn + 1e-8))
        if not sn > 1e-8 * (xn + 1e-8):
            log.append(_row(q, t, cost, PARAM_TOL, radius)); margins.append(mg)
            break
        dcost = cost - cc
        mg["fcost"] = _ratio(abs(dcost), 1e-6 * cost)
        if not abs(dcost) > 1e-6 * cost:
            log.append(_row(q, t, cost, FUNC_TOL, radius)); margins.append(mg)
            break
        rho = dcost / mcc
        mg["rho"] = _ratio(rho, 1e-3)
        if rho > 1e-3:
            q, t, cost, J, r = qc, tc, cc, Jc, rc
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            dec = 2.0
            gm = gradient_max_norm(q, J.T @ r)
            mg["grad"] = _ratio(gm, 1e-10)
            conv = gm <= 1e-10
            log.append(_row(q, t, cost, GRAD_TOL if conv else ACCEPTED, radius)); margins.append(mg)
            if conv:
                break
        else:
            radius /= dec
            dec *= 2.0
            log.append(_row(q, t, cost, REJECTED, radius)); margins.append(mg)
    return dict(q=q, t=t, log=np.array(log).reshape(-1, 10), margins=margins, rank=rank, J=J, grad0=grad0)


def solve_gn(po, pa, n, q0, t0, max_iter=10, edges=None):
    """Gauss-Newton: y = lstsq(J, -r); an iteration whose J is rank-deficient
    (np.linalg.matrix_rank) logs status 2 and ends the solve.
    -> dict(q, t, log, sv_ratio [rows]: smallest / largest singular value of each J, rank, J)."""
    q, t = np.array(q0, np.float64), np.array(t0, np.float64)
    cost, J, r = evaluate(po, pa, n, q, t, edges)
    log, svr = [], []
    rank0 = int(np.linalg.matrix_rank(J)) if len(J) else 0
    for _ in range(max_iter):
        sv = np.linalg.svd(J, compute_uv=False) if len(J) else np.zeros(6)
        sv = np.r_[sv, np.zeros(6 - len(sv))]
        svr.append(float(sv[5] / sv[0]) if sv[0] > 0 else 0.0)
        if not len(J) or np.linalg.matrix_rank(J) < 6:
            log.append(_row(q, t, cost, INVALID, 0.0))
            break
        y = np.linalg.lstsq(J, -r, rcond=None)[0]
        q, t = plus(q, y[:3]), t + y[3:]
        cost, J, r = evaluate(po, pa, n, q, t, edges)
        log.append(_row(q, t, cost, GN_STEP, 0.0))
    return dict(q=q, t=t, log=np.array(log).reshape(-1, 10), sv_ratio=np.array(svr), rank=rank0, J=J)


def clear_rows(margins, lo=0.1, hi=10.0):
    """number of leading log rows all of whose decisions are clear: every tested margin
    >= hi or <= lo"""
    k = 0
    for m in margins:
        v = np.array([x for x in m.values() if not np.isnan(x)])
        if np.any((v > lo) & (v < hi)):
            break
        k += 1
    return k

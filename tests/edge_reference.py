"""Independent yardstick for the edge path's line table: numpy only.

The project's edge features are its own (the reference has none), so the only statement of what
a line table IS is the definition in the header comment of oracle/edge_oracle.c.  This file is
written from that definition -- not from the oracle's functions and not from the kernels, and it
imports nothing of either: a partition / lexsort 5-NN where they scan and insert, np.linalg.eigh
where they run cyclic Jacobi.

    per last-frame edge point a: exact 5-NN among the frame's edges in (d2, index) order, the
    point its own first neighbour; d2 in float32, one rounding per operation,
    (dx*dx + dy*dy) + dz*dz; centroid c and covariance (divided by 5) of the five in float64;
    u the unit eigenvector of the largest eigenvalue, its sign fixed so that its largest-|.|
    component is positive; valid iff d2[4] < max_nn_d2 and lambda1 > line_ratio * lambda2
    (lambda2 the second largest); m < 5: six zeros, valid 0.

max_nn_d2 and line_ratio are float32 parameters of the product; line_ratio enters the float64
comparison as that float32's value.

Points with NaN coordinates are out of scope: (d2, index) order is undefined for them.

Every rule is also reachable as a deliberately WRONG variant through a keyword (LINE_VARIANTS);
tests/test_edge_host.py shows that each changes the asserted result of a named case of
tests/edge_cases.py.
"""
import numpy as np

F32 = np.float32
K = 5


def dist2(q, P):
    """float32 squared distances of q [3] to the rows of P [n, 3]: (dx*dx + dy*dy) + dz*dz"""
    with np.errstate(all="ignore"):
        d = F32(q)[None, :] - P
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def nearest(X, k, ties_high=False, chunk=512):
    """the k nearest of every point among all points (itself included) in (d2, index) order
    -> (idx [m, k] int64, d2 [m, k] float32); k <= m.  Exact under ties: every candidate whose
    d2 does not exceed the k-th smallest value of its row takes part in the (d2, index) sort.
    WRONG variant: ties_high orders ties by descending index."""
    m = len(X)
    idx = np.zeros((m, k), np.int64)
    d2k = np.zeros((m, k), F32)
    for lo in range(0, m, chunk):
        q = X[lo:lo + chunk]
        with np.errstate(all="ignore"):
            d = q[:, None, :] - X[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        kth = np.partition(d2, k - 1, axis=1)[:, k - 1]
        rows, cols = np.nonzero(d2 <= kth[:, None])
        v = d2[rows, cols]
        order = np.lexsort((-cols if ties_high else cols, v, rows))
        rows, cols, v = rows[order], cols[order], v[order]
        first = np.searchsorted(rows, np.arange(len(q)))
        take = first[:, None] + np.arange(k)[None, :]
        assert np.all(rows[take] == np.arange(len(q))[:, None])
        idx[lo:lo + chunk] = cols[take]
        d2k[lo:lo + chunk] = v[take]
    return idx, d2k


def line_table(edges, max_nn_d2, line_ratio, exclude_self=False, ties_high=False, cov_div=5.0, gate_rank=4,
               ratio_ge=False, l2_smallest=False, sign_on_0=False):
    """-> dict(line [m, 6] float32: centroid, direction; valid [m] uint8; and per point:
    idx [m, 5], d2 [m, 5] (float32, rank order), lam [m, 3] (descending, float64),
    gap5: (d2[5] - d2[4]) / d2[5], the room between the 5th and the 6th neighbour (inf when
          m == 5, 0 for a tie and for 0 / 0),
    ratio: lambda1 / (line_ratio * lambda2),
    aniso: (lambda1 - lambda2) / lambda1,
    sign_gap: the difference of the two largest |u| components).
    WRONG variants: exclude_self, ties_high, cov_div = 4, gate_rank = 3, ratio_ge, l2_smallest,
    sign_on_0."""
    E = np.ascontiguousarray(edges, F32).reshape(-1, 4)
    X = E[:, :3]
    m = len(X)
    out = dict(line=np.zeros((m, 6), F32), valid=np.zeros(m, np.uint8), idx=np.zeros((m, K), np.int64),
               d2=np.zeros((m, K), F32), lam=np.zeros((m, 3)), gap5=np.full(m, np.inf), ratio=np.full(m, np.nan),
               aniso=np.full(m, np.nan), sign_gap=np.full(m, np.nan))
    if m < K:
        return out
    exclude_self = exclude_self and m > K           # (five points: nothing else to take)
    kk = min(m, K + 2 if exclude_self else K + 1)
    idx, d2 = nearest(X, kk, ties_high)
    if exclude_self:                                # WRONG: the point is not its own neighbour
        keep = idx != np.arange(m)[:, None]
        keep[keep.all(1), -1] = False               # (among more than kk copies of itself)
        idx = idx[keep].reshape(m, kk - 1)
        d2 = d2[keep].reshape(m, kk - 1)
    if idx.shape[1] > K:
        d5, d6 = d2[:, K - 1].astype(np.float64), d2[:, K].astype(np.float64)
        with np.errstate(all="ignore"):
            out["gap5"] = np.where(d6 > 0, (d6 - d5) / np.where(d6 > 0, d6, 1.0), 0.0)
    idx, d2 = idx[:, :K], d2[:, :K]
    out["idx"], out["d2"] = idx, d2
    nb = X[idx].astype(np.float64)                                       # [m, 5, 3], rank order
    cen = np.zeros((m, 3))
    for k in range(K):
        cen = cen + nb[:, k]
    cen = cen / 5.0
    v = nb - cen[:, None, :]
    A = np.zeros((m, 3, 3))
    for k in range(K):
        A = A + v[:, k, :, None] * v[:, k, None, :]
    A = A / cov_div
    w, V = np.linalg.eigh(A)                                             # ascending
    l1, l2 = w[:, 2], (w[:, 0] if l2_smallest else w[:, 1])
    u = V[:, :, 2].copy()
    au = np.abs(u)
    big = np.zeros(m, np.int64) if sign_on_0 else np.argmax(au, axis=1)  # ties: the lower index
    flip = u[np.arange(m), big] < 0
    u[flip] = -u[flip]
    rl = np.float64(F32(line_ratio))
    gate = d2[:, gate_rank] < F32(max_nn_d2)
    line_ok = (l1 >= rl * l2) if ratio_ge else (l1 > rl * l2)
    out["valid"] = (gate & line_ok).astype(np.uint8)
    out["line"][:, :3] = cen.astype(F32)
    out["line"][:, 3:] = u.astype(F32)
    out["lam"] = w[:, ::-1].copy()
    sa = np.sort(au, axis=1)
    out["sign_gap"] = sa[:, 2] - sa[:, 1]
    with np.errstate(all="ignore"):
        out["ratio"] = l1 / (rl * w[:, 1])
        out["aniso"] = (l1 - w[:, 1]) / l1
    return out


LINE_VARIANTS = {
    "the point excluded from its own 5-NN": dict(exclude_self=True),
    "ties broken to the higher index": dict(ties_high=True),
    "covariance divided by 4": dict(cov_div=4.0),
    "the gate on d2[3]": dict(gate_rank=3),
    ">= in the ratio test": dict(ratio_ge=True),
    "the second-largest eigenvalue taken as the smallest": dict(l2_smallest=True),
    "the sign fixed on component 0": dict(sign_on_0=True),
}

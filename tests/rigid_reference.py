"""numpy float64 yardstick of the single-lane algebra every published pose ends in: the Kabsch
of slove_RT_by_SVD (scripts/PointCloudOdometry_noSeg.py:19-37), pyquaternion's trace method,
Eigen 3.3 umeyama without scaling and PCL 1.10 IterativeClosestPoint as
src/mapOptmization.cpp:224-236 sets it up.  The yardstick of tests/test_rigid_host.py (which
pins the CPU oracle's 3x3 algebra to it) and tests/test_gpu_rigid_tails.py (the device).

numpy only, and independent of oracle/*.c: the SVD is np.linalg.svd (LAPACK), the nearest
neighbour is a brute-force argmin.  Nothing here is tuned to what the code under test returns.
"""
from __future__ import annotations

import numpy as np

ICP_STATES = ("not_converged", "iterations", "transform", "abs_mse", "rel_mse", "no_correspondences")
BRANCHES = ("x", "y", "z", "w")          # the component the trace method takes the root of


def kabsch(src, dst, mask=None, reflection=False, dtype=np.float64):
    """R (3, 3), t (3,), det minimising |R src + t - dst| over the rows with mask != 0: the lines
    of slove_RT_by_SVD on arrays of `dtype` (float64 by default; float32 is numpy's own float32
    run of the same lines).  det is that of Vt.T @ U.T before any fix; with reflection=True a
    det < 0 flips the last row of Vt (the evident intent of :30-33, which raise TypeError)."""
    src = np.asarray(src, dtype)
    dst = np.asarray(dst, dtype)
    if mask is not None:
        keep = np.asarray(mask) != 0
        src, dst = src[keep], dst[keep]
    sm = src.mean(axis=0, keepdims=True)
    dm = dst.mean(axis=0, keepdims=True)
    H = (src - sm).T @ (dst - dm)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    det = float(np.linalg.det(R))
    if det < 0 and reflection:
        Vt = Vt.copy()
        Vt[2, :] *= -1
        R = Vt.T @ U.T
    t = -R @ sm.T + dm.T
    return R, t.ravel(), det


def quat_xyzw(R, dtype=np.float64):
    """pyquaternion Quaternion(matrix=R)._from_matrix: the trace method on m = R.T.
    -> (q [x, y, z, w], branch in BRANCHES, margins (|m22|, |m00 - m11| or |m00 + m11|)): the
    distances of the two comparisons that chose the branch from their thresholds.
    dtype float32: numpy's float32 run of the same lines on a float32 matrix (the scale
    0.5 / sqrt(t) is a Python float that numpy rounds to the array's float32)."""
    m = np.asarray(R, dtype).T
    if m[2, 2] < 0:
        margin = abs(m[0, 0] - m[1, 1])
        if m[0, 0] > m[1, 1]:
            t = 1 + m[0, 0] - m[1, 1] - m[2, 2]
            w, x, y, z = m[1, 2] - m[2, 1], t, m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]
            branch = "x"
        else:
            t = 1 - m[0, 0] + m[1, 1] - m[2, 2]
            w, x, y, z = m[2, 0] - m[0, 2], m[0, 1] + m[1, 0], t, m[1, 2] + m[2, 1]
            branch = "y"
    else:
        margin = abs(m[0, 0] + m[1, 1])
        if m[0, 0] < -m[1, 1]:
            t = 1 - m[0, 0] - m[1, 1] + m[2, 2]
            w, x, y, z = m[0, 1] - m[1, 0], m[2, 0] + m[0, 2], m[1, 2] + m[2, 1], t
            branch = "z"
        else:
            t = 1 + m[0, 0] + m[1, 1] + m[2, 2]
            w, x, y, z = t, m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]
            branch = "w"
    q = np.array([x, y, z, w], dtype) * dtype(0.5 / np.sqrt(np.float64(t)))
    return q.astype(np.float64), branch, (abs(float(m[2, 2])), float(margin))


def rot_from_quat(q):
    """Rotation matrix of a unit quaternion [x, y, z, w] (the textbook formula, not an inverse
    of quat_xyzw's branches)."""
    x, y, z, w = np.asarray(q, np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rot_angle(Ra, Rb):
    """Rotation angle of Ra^T Rb from |Ra - Rb|_F = 2 sqrt(2) sin(theta / 2) (no arccos near 1)."""
    return float(2.0 * np.arcsin(min(1.0, np.linalg.norm(np.asarray(Ra) - np.asarray(Rb)) / (2.0 * np.sqrt(2.0)))))


def axis_angle(axis, angle):
    """Rodrigues: rotation by `angle` rad about `axis`."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def umeyama(src, dst):
    """Eigen 3.3 umeyama(src, dst, with_scaling=false) on rows: sigma = (dst - dm)^T (src - sm) / n,
    R = U diag(1, 1, S2) V^T with S2 = -1 when det(U) det(V) < 0, t = dm - R sm.  -> 4x4 f64."""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    sm, dm = src.mean(axis=0), dst.mean(axis=0)
    sigma = (dst - dm).T @ (src - sm) / src.shape[0]
    U, _, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = dm - R @ sm
    return T


def nn1(tgt, q):
    """Exact 1-NN of every row of q in tgt, float64, ties to the lower index.
    -> (index [n], d2 [n], second-smallest d2 [n] (inf with one target))"""
    tgt = np.asarray(tgt, np.float64)
    q = np.asarray(q, np.float64)
    idx = np.zeros(q.shape[0], np.int64)
    d2 = np.zeros(q.shape[0])
    d2b = np.full(q.shape[0], np.inf)
    for a in range(0, q.shape[0], 256):
        d = ((q[a:a + 256, None, :] - tgt[None, :, :]) ** 2).sum(axis=2)
        j = np.argmin(d, axis=1)                      # the first minimum: the lower index
        r = np.arange(d.shape[0])
        idx[a:a + 256], d2[a:a + 256] = j, d[r, j]
        if tgt.shape[0] > 1:
            d[r, j] = np.inf
            d2b[a:a + 256] = d.min(axis=1)
    return idx, d2, d2b


def _tf32(T, p):
    """Matrix4f * point in float32, ((r0 x + r1 y) + r2 z) + t (Eigen's lazy product order)."""
    T = np.asarray(T, np.float32)
    p = np.asarray(p, np.float32)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return ((T[None, :3, 0] * x + T[None, :3, 1] * y) + T[None, :3, 2] * z) + T[None, :3, 3]


def _mul32(A, B):
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    return ((A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]) + A[:, 3:4] * B[3:4, :]


def icp(src, tgt, max_corr_dist=50.0, max_iter=100, trans_eps=1e-6, fit_eps=1e-6, guess=None):
    """pcl::IterativeClosestPoint (PCL 1.10) with TransformationEstimationSVD and
    DefaultConvergenceCriteria, then getFitnessScore().  src / tgt: rows of x, y, z(, intensity).
    The clouds and the 4x4 incremental / final transforms are float32 as PCL holds them; the
    nearest neighbour, the gate (d2 > max_d^2 drops the pair), umeyama and the criteria are float64.
    -> dict(T, fitness, converged, iterations, state, n_corr, trace); trace holds one dict per
    iteration (n_corr, mse, prev_mse, cos_a, tr2, d2, d2_second) for the margin checks of tests."""
    src = np.asarray(src, np.float32)[:, :3]
    tgt = np.asarray(tgt, np.float32)[:, :3]
    fin = np.eye(4, dtype=np.float32) if guess is None else np.array(guess, np.float32).reshape(4, 4)
    cur = _tf32(fin, src)
    max_d2 = float(np.float32(max_corr_dist)) ** 2
    prev_mse = np.finfo(np.float64).max
    it, converged, state, c = 0, False, "not_converged", 0
    trace = []
    while True:
        if tgt.shape[0] == 0:
            c = 0
        else:
            j, d2, d2b = nn1(tgt, cur)
            keep = ~(d2 > max_d2)
            c = int(keep.sum())
        if c < 3:                          # fewer than 3 pairs: PCL stops with no correspondences
            state, converged = "no_correspondences", False
            break
        inc = umeyama(cur[keep], tgt[j[keep]]).astype(np.float32)
        cur = _tf32(inc, cur)
        fin = _mul32(inc, fin)
        it += 1
        mse = float(d2[keep].sum() / c)
        cos_a = 0.5 * (float(inc[0, 0]) + float(inc[1, 1]) + float(inc[2, 2]) - 1.0)
        tr2 = float((inc[:3, 3].astype(np.float64) ** 2).sum())
        trace.append(dict(n_corr=c, mse=mse, prev_mse=prev_mse, cos_a=cos_a, tr2=tr2, d2=d2, d2_second=d2b))
        if it >= max_iter:                 # DefaultConvergenceCriteria::hasConverged, in its order
            state, converged = "iterations", True
            break
        if cos_a >= 1.0 - trans_eps and tr2 <= trans_eps:
            state, converged = "transform", True
            break
        if abs(mse - prev_mse) < 1e-12:
            state, converged = "abs_mse", True
            break
        if abs(mse - prev_mse) / prev_mse < fit_eps:
            state, converged = "rel_mse", True
            break
        prev_mse = mse
    if tgt.shape[0] and src.shape[0]:
        fitness = float(nn1(tgt, _tf32(fin, src))[1].mean())
    else:
        fitness = np.finfo(np.float64).max
    return dict(T=fin, fitness=fitness, converged=converged, iterations=it, state=state, n_corr=c, trace=trace)

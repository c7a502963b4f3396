"""Seeded inputs shared by tests/test_rigid_host.py (CPU oracle vs the numpy yardstick) and
tests/test_gpu_rigid_tails.py (device vs the same yardstick): the rotation set that reaches the
four branches of the quaternion trace method, Kabsch frames, and the ICP problems.  Everything is
generated from seeds; the yardstick results are computed once and cached here, never changed.
"""
from __future__ import annotations

import functools

import numpy as np

import rigid_reference as RR

DEG = np.pi / 180.0

# Every entry clears both comparisons of the trace method by >= 1e-3 (asserted in
# test_rigid_host.py).  A rotation of exactly 120 deg about (1, 1, 1) is a permutation matrix
# with a zero diagonal, on both thresholds at once, so the (1, 1, 1) case turns by 110 deg.
ROTATIONS = [
    ("x170", RR.axis_angle([1, 0, 0], 170 * DEG)),
    ("y170", RR.axis_angle([0, 1, 0], 170 * DEG)),
    ("z170", RR.axis_angle([0, 0, 1], 170 * DEG)),
    ("x170_tilted", RR.axis_angle([1, 0.15, -0.1], 170 * DEG)),
    ("y170_tilted", RR.axis_angle([-0.1, 1, 0.2], -170 * DEG)),
    ("z170_tilted", RR.axis_angle([0.12, -0.2, 1], 170 * DEG)),
    ("d110", RR.axis_angle([1, 1, 1], 110 * DEG)),
    ("small", RR.axis_angle([0.3, -0.5, 0.8], 0.03)),
    ("identity", np.eye(3)),
]
MASK_POSE_N = (3, 4, 63, 64, 65, 257)
KABSCH_F32_N = MASK_POSE_N + (2047, 2048, 2049, 4097)      # the 2048-point chunk edge


def kabsch_frames(sizes, seed=7, extent=12.0, noise=1e-3):
    """One frame per (rotation, n): src ~ N(0, extent) m, dst = R src + t + noise.
    -> list of (name, n, R_true, src [n, 3] f64, dst [n, 3] f64)"""
    rng = np.random.default_rng(seed)
    out = []
    for name, R in ROTATIONS:
        for n in sizes:
            src = rng.standard_normal((n, 3)) * extent
            t = rng.uniform(-3, 3, 3)
            dst = src @ R.T + t + rng.standard_normal((n, 3)) * noise
            out.append((name, n, R, src, dst))
    return out


def chunk_mask(n):
    """Keeps rows; drops rows on both sides of the 2048-row chunk edges (and a few others) once a
    frame is large enough to spare them."""
    m = np.ones(n, np.uint8)
    if n > 8:
        m[1] = 0
        m[5::7] = 0
        for e in (2048, 4096):
            m[max(0, min(n, e - 2)):min(n, e + 2)] = 0
    return m


@functools.lru_cache(maxsize=None)
def kabsch_f32_cases():
    """The float32 tail's frames (KABSCH_F32_N): float32 dst and flow, src = f32(dst + flow) so that
    the src= and flow= forms of the kernel read the same values, a mask, and for mask None / mask
    the yardstick in float64 (R, t, q, branch) and numpy's float32 run of the same lines (R32, t32,
    q32) on those float32 values.  -> list of dicts"""
    out = []
    for name, n, _, src, dst in kabsch_frames(KABSCH_F32_N, seed=8):
        d32 = dst.astype(np.float32)
        f32 = (src - dst).astype(np.float32)
        s32 = d32 + f32
        c = dict(name=f"{name}-n{n}", n=n, dst=d32, flow=f32, src=s32, mask=chunk_mask(n), ref={})
        for key, m in (("all", None), ("mask", c["mask"])):
            R, t, _ = RR.kabsch(s32.astype(np.float64), d32.astype(np.float64), mask=m, reflection=True)
            q, branch, margins = RR.quat_xyzw(R)
            R32, t32, _ = RR.kabsch(s32, d32, mask=m, reflection=True, dtype=np.float32)
            q32, _, _ = RR.quat_xyzw(R32, np.float32)
            c["ref"][key] = dict(R=R, t=t, q=q, branch=branch, margins=margins, R32=R32.astype(np.float64),
                                 t32=t32.astype(np.float64), q32=q32, n_bg=n if m is None else int(m.sum()))
        out.append(c)
    return out


def far_frame(seed=11):
    """A 40 m cloud whose centroid lies 5 km out, turned by 170 deg about its own centre."""
    rng = np.random.default_rng(seed)
    c = np.array([3000.0, -4000.0, 50.0])
    local = rng.uniform(-20, 20, (500, 3))
    R = RR.axis_angle([0.2, 1, -0.1], 170 * DEG)
    src = local + c
    dst = local @ R.T + c + np.array([0.7, -0.4, 0.1]) + rng.standard_normal((500, 3)) * 1e-3
    return R, src, dst


# --------------------------------------------------------------------------- ICP, one step
ICP_NS = (3, 255, 256, 257, 1025)
ICP_NT = (3, 2047, 2048, 2049, 4100)      # the 2048-point target tile of the 1-NN kernel
GRID = 0.25                               # coordinates are small integers / 4: every f32 d2 is exact
BOX = 64                                  # |k| <= 64: a 32 m box


def _xyzi(p):
    return np.concatenate([p, np.ones((p.shape[0], 1))], axis=1).astype(np.float32)


def _grid_points(rng, n, box=BOX):
    """n distinct points with integer / 4 coordinates"""
    k = np.unique(rng.integers(-box, box + 1, (3 * n + 16, 3)), axis=0)
    assert k.shape[0] >= n
    return rng.permutation(k)[:n] * GRID


def _to_grid(p):
    return np.round(p / GRID) * GRID


def _sources(rng, tgt, ns, R, t, guess=None, min_gap=0.0):
    """ns grid points: jittered targets moved back by (R, t) and then by the guess, kept only
    where the nearest and the second nearest target of the point the ICP starts from (the source
    through the guess) differ by more than min_gap in d2."""
    nt = tgt.shape[0]
    m = 3 * ns + 64
    base = tgt[rng.integers(0, nt, m)] + rng.integers(-6, 7, (m, 3)) * GRID
    cand = (base - t) @ R                                       # rows R^T (b - t)
    if guess is not None:
        g = np.asarray(guess, np.float64)
        cand = (cand - g[:3, 3]) @ g[:3, :3]
    cand = rng.permutation(np.unique(_to_grid(cand), axis=0))
    start = cand if guess is None else RR._tf32(guess, cand)
    j, d2, d2b = RR.nn1(tgt, np.asarray(start, np.float32))
    ok = d2b - d2 > min_gap
    if ns <= min(nt, 16):              # a handful of pairs: distinct targets, so H keeps rank 2
        ok &= np.concatenate([[True], [j[i] not in j[:i][ok[:i]] for i in range(1, len(j))]])
    cand = cand[ok]
    assert cand.shape[0] >= ns, (cand.shape[0], ns)
    return cand[:ns]


def _T(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


@functools.lru_cache(maxsize=None)
def icp_step_problems():
    """The one-iteration problems (max_iter = 1).  -> list of dicts: name, src, tgt (x, y, z, 1
    float32), guess (4x4 float32), max_corr_dist, min_gap (the least d2 gap between the nearest and
    the second nearest target at the start), ties (source rows whose two nearest targets tie)."""
    rng = np.random.default_rng(2024)
    R5 = RR.axis_angle([0.2, -0.3, 1.0], 5 * DEG)
    R170 = RR.axis_angle([0.1, 0.2, 1.0], 170 * DEG)
    t5 = np.array([0.5, -0.25, 0.25])
    eye = np.eye(4, dtype=np.float32)
    P = []

    def add(name, src, tgt, guess=eye, gate=50.0, min_gap=0.0, ties=()):
        P.append(dict(name=name, src=_xyzi(src), tgt=_xyzi(tgt), guess=np.array(guess, np.float32),
                      max_corr_dist=gate, min_gap=min_gap, ties=tuple(ties)))

    for nt in ICP_NT:
        tgt = _grid_points(rng, nt)
        for ns in ICP_NS:
            add(f"rot5_ns{ns}_nt{nt}", _sources(rng, tgt, ns, R5, t5), tgt)
    # 170 deg, handed over as the guess: the ICP starts from float32 points off the grid, so the
    # nearest target must win by a d2 gap far above the float32 rounding of d2 (~1e-4 here)
    g170 = _T(R170, [0.25, 0.5, -0.25])
    for ns, nt in ((257, 2049), (1025, 4100)):
        tgt = _grid_points(rng, nt)
        add(f"guess170_ns{ns}_nt{nt}", _sources(rng, tgt, ns, R5, t5, guess=g170, min_gap=0.05),
            tgt, guess=g170, min_gap=0.05)
    # mirrored target: a slab thin in x on a 2 m lattice in y, z; the source is its mirror image,
    # at most 1 m from its own target, so the best orthogonal fit is a reflection (S(2) = -1)
    n = 2048
    iy, iz = np.divmod(rng.permutation(46 * 46)[:n], 46)
    slab = np.stack([rng.choice([-0.5, -0.25, 0.25, 0.5], n), 2.0 * iy - 45.0, 2.0 * iz - 45.0], axis=1)
    add("mirror_ns256_nt2048", (slab * [-1, 1, 1])[rng.permutation(n)[:256]], slab)
    # coplanar target (z = 0 exactly), sources off the plane
    tgt = _grid_points(rng, 2047)
    tgt[:, 2] = 0.0
    tgt = np.unique(tgt, axis=0)
    tgt = np.concatenate([tgt, np.stack([np.arange(2047 - tgt.shape[0]) * 1.0 + 40.0,
                                         np.full(2047 - tgt.shape[0], 40.0),
                                         np.zeros(2047 - tgt.shape[0])], axis=1)])
    add("coplanar_ns255_nt2047", _sources(rng, tgt, 255, R5, t5), rng.permutation(tgt))
    # ties across the tile edge: source (40, 0, 0) is 1 m from targets 2047 (+x) and 2048 (-x),
    # source (-40, 0, 0) is 1 m from targets 4095 (-x) and 4096 (+x); each goes to the lower index
    tgt = _grid_points(rng, 4100)
    tgt[2047], tgt[2048] = [41, 0, 0], [39, 0, 0]
    tgt[4095], tgt[4096] = [-41, 0, 0], [-39, 0, 0]
    src = np.concatenate([[[40.0, 0, 0], [-40.0, 0, 0]], _sources(rng, tgt, 6, R5, t5)])
    add("tie_ns8_nt4100", src, tgt, ties=(0, 1))
    # the gate between two exact d2 values
    tgt = _grid_points(rng, 2049)
    src = _sources(rng, tgt, 257, R5, t5)
    d2 = np.sort(RR.nn1(tgt, src)[1])
    k = np.flatnonzero(np.diff(d2) > 0)
    k = k[np.argmin(np.abs(k - 128))]                      # about half the pairs pass
    add("gate_ns257_nt2049", src, tgt, gate=float(np.sqrt(0.5 * (d2[k] + d2[k + 1]))))
    return P


@functools.lru_cache(maxsize=None)
def icp_step_reference():
    return [RR.icp(p["src"], p["tgt"], max_corr_dist=p["max_corr_dist"], max_iter=1, guess=p["guess"])
            for p in icp_step_problems()]


# --------------------------------------------------------------------------- ICP, every outcome
def _scene(seed=5):
    """A jittered 2 m lattice (384 targets) and a 150-point subset of it."""
    rng = np.random.default_rng(seed)
    lat = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(6), indexing="ij"), -1).reshape(-1, 3)
    tgt = _xyzi(lat * 2.0 - 7.0 + rng.uniform(-0.4, 0.4, lat.shape))
    return rng, tgt, tgt[rng.permutation(len(tgt))[:150]].copy()


def _moved(xyzi, R=np.eye(3), t=(0, 0, 0), noise=None):
    out = xyzi.copy()
    p = xyzi[:, :3].astype(np.float64) @ np.asarray(R).T + np.asarray(t, np.float64)
    out[:, :3] = (p if noise is None else p + noise).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def icp_outcome_batches():
    """Batches of problems that share one parameter set (ssf_icp_batch takes one per launch), each
    with a problem that stops early beside one that runs on, reaching every ICP state on purpose.
    -> list of (params dict, [dict(name, src, tgt, expect)])"""
    rng, tgt, sub = _scene()
    shift = [0.3, -0.2, 0.1]
    subset = _moved(sub, t=shift)                         # iteration 1 lands on the targets
    R12 = RR.axis_angle([0.1, 0.2, 1], 12 * DEG)
    sub2 = tgt[np.random.default_rng(1).permutation(len(tgt))[:200]]
    slow = _moved(sub2, R12, [0.5, 0.2, -0.3])            # several iterations of wrong pairs first
    noisy = _moved(sub, t=shift, noise=np.random.default_rng(1).standard_normal((150, 3)) * 0.3)
    far = _moved(sub, t=[1000.0, 0, 0])                   # nothing inside the 50 m gate
    two = subset[:2]                                      # two pairs: fewer than three
    # exactly collinear clouds (17 points on k (1, 1, 0), the target 0.25 m along x): the
    # cross-covariance has rank 1 exactly, so the rotation about the line is free.  The points, the
    # MSE and (centroid at the origin) the first translation do not depend on it, the transform
    # criterion of later iterations does: under max_iter = 2 the outcome is determined (expect
    # "iterations"), under the default limit only what does not depend on the free angle is
    # compared (expect None: LAPACK's choice gives abs_mse after 3 iterations, R = I gives
    # transform after 2).
    line = np.arange(-8, 9)[:, None] * np.array([[1.0, 1.0, 0.0]])
    line_s, line_t = _xyzi(line), _xyzi(line + [0.25, 0.0, 0.0])
    P = lambda name, src, t, expect: dict(name=name, src=src, tgt=t, expect=expect)
    return [
        (dict(max_iter=2, trans_eps=1e-6, fit_eps=1e-6),
         [P("limit_slow", slow, tgt, "iterations"), P("limit_far", far, tgt, "no_correspondences"),
          P("limit_subset", subset, tgt, "iterations"), P("collinear", line_s, line_t, "iterations")]),
        (dict(max_iter=100, trans_eps=1e-6, fit_eps=1e-6),
         [P("subset", subset, tgt, "transform"), P("slow", slow, tgt, "transform"),
          P("two_points", two, tgt, "no_correspondences"), P("far", far, tgt, "no_correspondences"),
          P("collinear_free", line_s, line_t, None)]),
        (dict(max_iter=100, trans_eps=1e-30, fit_eps=1e-3),
         [P("abs_mse", subset, tgt, "abs_mse"), P("rel_mse", noisy, tgt, "rel_mse"),
          P("far_eps", far, tgt, "no_correspondences")]),
    ]


@functools.lru_cache(maxsize=None)
def icp_outcome_reference():
    return [[RR.icp(p["src"], p["tgt"], max_corr_dist=50.0, **prm) for p in probs]
            for prm, probs in icp_outcome_batches()]


def check_outcome_margins(ref, prm):
    """Every comparison of DefaultConvergenceCriteria the yardstick made on this problem is clear
    of its threshold by a factor of 10: the criteria ahead of the deciding one miss by 10 at the
    stopping iteration and all of them at every iteration before it, the deciding one is met
    with a factor of 10 to spare.  So float32 / summation-order differences cannot change the
    outcome.  (The iteration limit and the pair count are integers.)"""
    te, fe = prm["trans_eps"], prm["fit_eps"]
    n = len(ref["trace"])
    for k, t in enumerate(ref["trace"]):
        last = k == n - 1 and ref["state"] != "no_correspondences"
        state = ref["state"] if last else None
        if last and state == "iterations":
            assert n == prm["max_iter"]
            break
        d = abs(t["mse"] - t["prev_mse"])
        tests = [("transform", max(1.0 - t["cos_a"], t["tr2"]), te),
                 ("abs_mse", d, 1e-12), ("rel_mse", d / t["prev_mse"] if t["prev_mse"] > 0 else np.inf, fe)]
        for name, value, thr in tests:
            if name == state:
                assert value <= thr / 10, (k, name, value, thr)
                break
            assert value >= thr * 10, (k, name, value, thr)
    if ref["state"] == "no_correspondences":
        assert ref["n_corr"] < 3


def _apply(T, xyzi):
    T = np.asarray(T, np.float64)
    return xyzi[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]


def check_icp(got, ref, compare_rotation=True):
    """The bars of _check_icp in tests/test_gpu_loop.py: state, iteration count and converged
    equal, T within 1e-5 (rotation) / 1e-4 m, fitness within 1e-6 relative."""
    assert got["state"] == ref["state"], (got["state"], ref["state"])
    assert got["iterations"] == ref["iterations"], (got["iterations"], ref["iterations"])
    assert got["converged"] == ref["converged"]
    if compare_rotation:
        assert np.abs(got["T"][:3, :3] - ref["T"][:3, :3]).max() < 1e-5, (got["T"], ref["T"])
        assert np.abs(got["T"][:3, 3] - ref["T"][:3, 3]).max() < 1e-4, (got["T"], ref["T"])
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-6 * max(1.0, abs(ref["fitness"]))


def check_icp_free_rotation(got, ref, p):
    """A collinear problem whose outcome depends on the free angle about the line: what does not
    depend on it.  T is rigid to 1e-5, carries the source onto the yardstick's result within
    1e-4 m, converged, fitness as in check_icp."""
    R = got["T"][:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and np.linalg.det(R) > 0, R
    assert np.abs(_apply(got["T"], p["src"]) - _apply(ref["T"], p["src"])).max() < 1e-4
    assert got["converged"] and ref["converged"] and got["n_corr"] == ref["n_corr"]
    assert abs(got["fitness"] - ref["fitness"]) <= 1e-6 * max(1.0, abs(ref["fitness"]))


# --------------------------------------------------------------------------- rank-deficient Kabsch
def rank_cases():
    """Rows whose cross-covariance is exactly zero or exactly of rank 1 (coordinates are
    integers / 4, so the centred rows and H are exact in float32 and float64).
    -> {name: (src [n, 3], dst [n, 3])}"""
    k = np.arange(17)[:, None] * 0.25
    x, xy, yx = np.array([[1.0, 0, 0]]), np.array([[1.0, 1.0, 0]]), np.array([[-1.0, 1.0, 0]])
    shift = np.array([0.25, -1.0, 2.0])
    one = np.array([[1.5, -2.0, 0.25]])
    return {
        "zero_single": (one, one + shift),
        "zero_coincident": (np.repeat(one, 5, axis=0), np.repeat(one + shift, 5, axis=0)),
        "line_x_shift": (k * x, k * x + shift),
        "line_x_turned": ((k - 2.0) * x, (k - 2.0) * np.array([[0, 1.0, 0]]) + shift),
        "line_xy_shift": (k * xy, k * xy + [0.25, 0, 0]),
        "line_xy_turned": ((k - 2.0) * xy, k * yx + shift),
    }


def check_rank_case(name, src, dst, R, t, tol=1e-9):
    """tol: 1e-9 for the float64 tails; float32 outputs state their own (see the caller)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    if name.startswith("zero"):
        assert np.array_equal(R, np.eye(3)), R
        assert np.abs(t - (md - ms)).max() <= tol
        return
    assert np.abs(R @ R.T - np.eye(3)).max() <= tol, R
    assert np.linalg.det(R) > 0
    extent = np.abs(src - ms).max()
    assert np.abs((src - ms) @ R.T - (dst - md)).max() <= tol * extent
    assert np.abs(R @ ms + t - md).max() <= tol * max(1.0, np.abs(md).max())

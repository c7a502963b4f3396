"""Seeded inputs of the registration-stage tests, shared by tests/test_registration_host.py (the
CPU oracle against the yardstick) and tests/test_gpu_solve_yardstick.py (the device against it).

A solve case is a last frame [m, 4] with a HAND-MADE plane table (normal, valid), a current
frame, a warm start, the solver and max_iter: the correspondences are whatever the 1-NN
association at the warm start gives.  A case is admitted only on the yardstick's own evidence
(admit()): every association gap >= 1e-3 relative, and every solver decision up to the last
compared row clear of its threshold by 10x.  Where a docstring names a status, the seed was found
by searching until the yardstick logged it (python tests/registration_cases.py search).
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import registration_reference as ref

LM, GN = "ceres_lm", "gn"
ITERS = {LM: 8, GN: 10}


@dataclass
class Case:
    name: str
    family: str
    last: np.ndarray          # [m, 4] f32
    normal: np.ndarray        # [m, 3] f32
    valid: np.ndarray         # [m] u8
    curr: np.ndarray          # [c, 4] f32
    pose0: np.ndarray         # [7] f64: q xyzw, t
    solver: str
    max_iter: int
    edges: tuple = None       # (last_e [me, 4], line [me, 6], lvalid [me] u8, curr_e [ce, 4])
    rank_deficient: bool = False
    open_end: bool = False    # the last decision is a toss-up between exits 3 and 4 (same pose)
    asserted: bool = True
    note: dict = field(default_factory=dict)


# ---------------------------------------------------------------------------- helpers
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def axis_angle_quat(axis, angle):
    return np.r_[np.sin(angle / 2.0) * unit(axis), np.cos(angle / 2.0)]


def _xyzi(xyz):
    k = np.arange(len(xyz))
    return np.c_[xyz, k + (k % 64) / 100.0].astype(np.float32)


def _pads(centre, k=12):
    """k invalid last-frame points far from everything (a last frame has > 10 points, :158)"""
    return np.asarray(centre) + 1000.0 + 7.0 * np.arange(k)[:, None] * np.array([1.0, 0.3, -0.2])


def build(name, family, solver, po, normals, q_true, t_true, resid, pose0, max_iter=None, mask=None,
          shift=None, **kw):
    """last = the points pa_i = R po_i + t - resid_i n_i (+ an in-plane shift), so that the
    residual of pair i at the true pose is resid_i; plus invalid pads.  mask: valid flag per pair."""
    po = np.asarray(po, np.float64)
    normals = np.asarray(normals, np.float32)
    pa = ref.quat_rotate(q_true, po) + t_true - np.asarray(resid)[:, None] * normals.astype(np.float64)
    if shift is not None:
        pa = pa + shift
    c = len(po)
    pads = _pads(pa.mean(0) if c else np.zeros(3))
    last = _xyzi(np.concatenate([pa, pads]))
    nrm = np.concatenate([normals, np.zeros((len(pads), 3), np.float32)])
    valid = np.r_[np.ones(c, np.uint8) if mask is None else np.asarray(mask, np.uint8), np.zeros(len(pads), np.uint8)]
    return Case(name, family, last, nrm, valid, _xyzi(po), np.asarray(pose0, np.float64), solver,
                ITERS[solver] if max_iter is None else max_iter, **kw)


def spread(rng, c, box=20.0):
    """c well-spread points and random unit normals"""
    return rng.uniform(-box, box, (c, 3)), unit(rng.normal(size=(c, 3)))


def tangent_shift(rng, normals, amount=0.2):
    """moves pa inside its plane (the residual is unchanged)"""
    a = np.cross(normals, unit(rng.normal(size=3)))
    return a * rng.uniform(-amount, amount, (len(normals), 1))


TRUTH_Q = axis_angle_quat([0.1, -0.2, 1.0], 0.02)
TRUTH_T = np.array([0.8, -0.1, 0.05])


def near(rng, q, t, rot, trans):
    """a warm start rot rad / trans m (per axis at most) from (q, t)"""
    return np.r_[ref.quat_mul(axis_angle_quat(rng.normal(size=3), rot), q), t + rng.uniform(-trans, trans, 3)]


# ---------------------------------------------------------------------------- solve families
# Every base case is a generator g(rng, solver) run with its committed seed SEEDS[base], once per
# solver (the LM case and its GN twin share the inputs).  WANT[base] is what the search required
# of the yardstick's LM log beyond admit().
def _named(base, family, solver, *a, **kw):
    return build(f"{base}_{'lm' if solver == LM else 'gn'}", family, solver, *a, **kw)


def g_clean(rng, solver, base="clean"):
    po, nr = spread(rng, 400)
    return _named(base, "status", solver, po, nr, TRUTH_Q, TRUTH_T, np.zeros(400),
                  near(rng, TRUTH_Q, TRUTH_T, 0.003, 0.1), shift=tangent_shift(rng, nr, 0.05))


def g_outliers(rng, solver):
    po, nr = spread(rng, 400)
    resid = rng.normal(0, 0.02, 400)
    o = rng.choice(400, 40, replace=False)
    resid[o] = rng.uniform(0.3, 1.0, 40) * rng.choice([-1, 1], 40)          # beyond the Huber knee
    return _named("outliers", "status", solver, po, nr, TRUTH_Q, TRUTH_T, resid, near(rng, TRUTH_Q, TRUTH_T, 0.003, 0.1))


def g_knee(rng, solver):
    po, nr = spread(rng, 400)
    resid = rng.normal(0, 0.002, 400)
    k = rng.choice(400, 40, replace=False)
    resid[k] = 0.1 * (1.0 + rng.uniform(-1e-3, 1e-3, 40)) * rng.choice([-1, 1], 40)       # at the knee
    return _named("knee", "status", solver, po, nr, TRUTH_Q, TRUTH_T, resid, near(rng, TRUTH_Q, TRUTH_T, 0.003, 0.1))


def g_at_solution(rng, solver):
    po, nr = spread(rng, 400)
    return _named("at_solution", "status", solver, po, nr, TRUTH_Q, TRUTH_T, rng.normal(0, 0.002, 400),
                  np.r_[TRUTH_Q, TRUTH_T], open_end=True)


def g_six_noisy(rng, solver):
    """six noisy correspondences: the gradient-tolerance exit (5) in LM"""
    po, nr = spread(rng, 6, 5.0)
    return _named("six_noisy", "status", solver, po, nr, TRUTH_Q, TRUTH_T, rng.normal(0, 0.01, 6),
                  near(rng, TRUTH_Q, TRUTH_T, 0.003, 0.05), max_iter=12 if solver == LM else None)


def g_far(rng, solver, base="far"):
    """rejected steps and a shrinking radius: 6 .. 11 correspondences, the truth 2.6 .. 3.14 rad
    off, a random-axis warm start"""
    c = int(rng.integers(6, 12))
    po, nr = spread(rng, c, 5.0)
    qt = axis_angle_quat(rng.normal(size=3), rng.uniform(2.6, 3.14))
    return _named(base, "status", solver, po, nr, qt, TRUTH_T, np.zeros(c),
                  np.r_[axis_angle_quat(rng.normal(size=3), rng.uniform(0, 0.5)), 0, 0, 0],
                  max_iter=12 if solver == LM else None)


def g_zero_residual(rng, solver):
    """one exactly zero-residual pair (po == pa at the identity warm start): six invalid steps"""
    return _named("zero_residual", "status", solver, np.array([[1.5, -2.25, 0.75]]), np.float32([[0.0, 0.6, 0.8]]),
                  np.array([0, 0, 0, 1.0]), np.zeros(3), np.zeros(1), [0, 0, 0, 1, 0, 0, 0],
                  rank_deficient=True)


def g_none_valid(rng, solver):
    po, nr = spread(rng, 40)
    return _named("none_valid", "status", solver, po, nr, TRUTH_Q, TRUTH_T, np.zeros(40),
                  near(rng, TRUTH_Q, TRUTH_T, 0.003, 0.1), mask=np.zeros(40), rank_deficient=True)


def g_quat(half, base):
    """first step on one side of theta = |d| = 2^-7 (x2 = |d|^2 against 2^-14), clear by 10x"""
    def g(rng, solver):
        po, nr = spread(rng, 400)
        q0 = ref.quat_mul(axis_angle_quat(rng.normal(size=3), 2.0 * half), TRUTH_Q)
        return _named(base, "quat", solver, po, nr, TRUTH_Q, TRUTH_T, rng.normal(0, 0.002, 400),
                      np.r_[q0, TRUTH_T + 0.02])
    return g


OBLIQUE = np.float32(unit([0.3, -0.5, 0.81]))


def g_rank(kind):
    def g(rng, solver):
        po, nr = spread(rng, 300)
        ws = near(rng, TRUTH_Q, TRUTH_T, 0.003, 0.1)
        resid = rng.normal(0, 0.003, 300)
        asserted = True
        if kind == "par_z":
            nr = np.tile(np.float32([0, 0, 1]), (300, 1))
        elif kind == "two_family":
            nr = np.tile(np.float32([0, 0, 1]), (300, 1))
            nr[::2] = np.float32([1, 0, 0])
        elif kind == "par_oblique":
            nr = np.tile(OBLIQUE, (300, 1))
            asserted = solver == LM        # GN: the Cholesky pivot is rounding noise of either sign
        else:                              # every po on one line through the origin
            po = np.outer(rng.uniform(-20, 20, 300), unit([1.0, 0.5, -0.25]))
            asserted = solver == LM        # GN: no exactly zero column either
        return _named(kind, "rank", solver, po, nr, TRUTH_Q, TRUTH_T, resid, ws, rank_deficient=True,
                      asserted=asserted)
    return g


def g_far5km(rng, solver):
    """a scene 5 km from the origin (float32 ulp 2.4e-4 .. 4.9e-4 m); the true motion turns it
    about its own centre"""
    c = np.array([3000.0, -4000.0, 20.0])
    po, nr = spread(rng, 400)
    t = c - ref.quat_rotate(TRUTH_Q, c) + TRUTH_T
    return _named("far5km", "scale", solver, po + c, nr, TRUTH_Q, t, rng.normal(0, 0.002, 400),
                  near(rng, TRUTH_Q, t, 1e-6, 0.05))


def g_tiny(rng, solver):
    po, nr = spread(rng, 200, 5e-4)                                         # |po| < 1e-3
    return _named("tiny", "scale", solver, po, nr, TRUTH_Q, TRUTH_T, rng.normal(0, 2e-7, 200),
                  near(rng, TRUTH_Q, TRUTH_T, 1e-4, 2e-6), open_end=True)


def g_norm(e, base, asserted):
    """a warm start off the unit sphere by e.  The scene carries 2 mm of noise: on a noise-free
    one the cost after the first step is ~1e-8 while its gradient is not yet small, and ONE ulp of
    the pose (2^-52) moves that cost by 0.5 .. 2e-9 of itself -- the 1e-9 bound on the cost would
    compare the roundings of two steps, not two solvers (clean_* keeps the noise-free scene)."""
    def g(rng, solver):
        po, nr = spread(rng, 400)
        ws = near(rng, TRUTH_Q, TRUTH_T, 0.003, 0.1)
        ws[:4] *= 1.0 + e
        return _named(base, "norm", solver, po, nr, TRUTH_Q, TRUTH_T, rng.normal(0, 0.002, 400), ws,
                      asserted=asserted)
    return g


def g_edge(n_pl, n_e, base):
    """the project's point-to-line blocks with a hand-made line table"""
    def g(rng, solver):
        po, nr = spread(rng, max(n_pl, 1))
        ws = near(rng, TRUTH_Q, TRUTH_T, 0.003, 0.1)
        cs = _named(base, "edge", solver, po, nr, TRUTH_Q, TRUTH_T, rng.normal(0, 0.002, len(po)), ws,
                    mask=None if n_pl else np.zeros(1))
        epo, u = spread(rng, max(n_e, 1))
        u = np.float32(u)
        off = np.cross(u, unit(rng.normal(size=3))) * rng.normal(0, 0.01, (len(u), 1))     # off the line
        cen = ref.quat_rotate(TRUTH_Q, epo) + TRUTH_T + u * rng.uniform(-0.3, 0.3, (len(u), 1)) + off
        last_e = _xyzi(np.concatenate([cen, _pads(cen.mean(0), 6)]))
        line = np.concatenate([np.c_[last_e[:len(cen), :3], u], np.zeros((6, 6))]).astype(np.float32)
        lvalid = np.r_[np.full(len(cen), 1 if n_e else 0, np.uint8), np.zeros(6, np.uint8)]
        cs.edges = (last_e, line, lvalid, _xyzi(epo))
        return cs
    return g


EDGE_LDS_CAP = 8192            # kEdgeLdsMax of edges.hip: a larger last edge cloud is read from global memory


def edge_lds_cap():
    """kEdgeLdsMax as edges.hip states it, so a changed cap cannot leave the fallback untested
    without a test saying so"""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ssf-slam_amd", "csrc", "edges.hip")
    return int(re.search(r"constexpr int kEdgeLdsMax = (\d+);", open(src).read()).group(1))


def g_edge_big_last(rng, solver):
    """edge_both with a last edge cloud of more than EDGE_LDS_CAP points: k_edge_associate's
    global-memory fallback (ml > lds_cap).  The extra points are invalid filler kilometres away on a
    line of its own, half of it before the real points and half after, so the real ones sit at
    indices from 4100 on and no filler point is ever one of a query's two nearest (the gap that
    admit() requires is the real points')."""
    cs = g_edge(200, 60, "edge_big_last")(rng, solver)
    last_e, line, lvalid, curr_e = cs.edges
    n_fill = EDGE_LDS_CAP + 8
    fill = last_e[:, :3].astype(np.float64).mean(0) + 3000.0 + 3.0 * np.arange(n_fill)[:, None] * np.array([1.0, -0.4, 0.25])
    h = n_fill // 2
    z = lambda k, w: np.zeros((k, w), np.float32)                                               # noqa: E731
    cs.edges = (_xyzi(np.concatenate([fill[:h], last_e[:, :3], fill[h:]])),
                np.concatenate([z(h, 6), line, z(n_fill - h, 6)]),
                np.r_[np.zeros(h, np.uint8), lvalid, np.zeros(n_fill - h, np.uint8)], curr_e)
    assert len(cs.edges[0]) > EDGE_LDS_CAP
    return cs


def g_edge_pair(empty_last):
    """A launch of its own (max_iter one above its solver's, so the family test batches the two
    together and apart from the rest): edge_pair_first is edge_both again; edge_pair_empty_last,
    the batch's LAST pair, has an empty last edge cloud and 60 current edge points -- no edge
    record is valid, and its last-frame offset is the line table's row count."""
    def g(rng, solver):
        cs = g_edge(200, 60, "edge_pair_empty_last" if empty_last else "edge_pair_first")(rng, solver)
        cs.max_iter = ITERS[solver] + 1
        if empty_last:
            cs.edges = (np.zeros((0, 4), np.float32), np.zeros((0, 6), np.float32), np.zeros(0, np.uint8), cs.edges[3])
        return cs
    return g


def _has(status):
    return lambda y: status in y["sol"]["log"][:, 8]


def steps_x2(y, pose0):
    """|d|^2 of the rotation step of every accepted / GN row of the yardstick's log"""
    log, prev, out = y["sol"]["log"], np.asarray(pose0), []
    for row in log:
        if row[8] in (ref.ACCEPTED, ref.GRAD_TOL, ref.GN_STEP):
            d = ref.local_delta(row[:4], row[4:7], prev[:4], prev[4:7])
            out.append(float(d[:3] @ d[:3]))
            prev = row[:7]
    return np.array(out)


def quat_paths_clear(y, pose0, large):
    """the first step on the named side of x2 = 2^-14, every step clear of it by 10x"""
    x2 = steps_x2(y, pose0) / 2.0 ** -14
    return bool(len(x2) and (x2[0] > 10 if large else 0 < x2[0] < 0.1) and np.all((x2 > 10) | (x2 < 0.1))
                and np.any((x2 > 0) & (x2 < 0.1)))


GEN = dict(clean=g_clean, outliers=g_outliers, knee=g_knee, at_solution=g_at_solution, six_noisy=g_six_noisy,
           far_a=lambda r, s: g_far(r, s, "far_a"), far_b=lambda r, s: g_far(r, s, "far_b"),
           far_c=lambda r, s: g_far(r, s, "far_c"), zero_residual=g_zero_residual, none_valid=g_none_valid,
           quat_small=g_quat(0.002, "quat_small"), quat_large=g_quat(0.03, "quat_large"),
           par_z=g_rank("par_z"), two_family=g_rank("two_family"), par_oblique=g_rank("par_oblique"),
           po_line=g_rank("po_line"), far5km=g_far5km, tiny=g_tiny,
           norm_p1e12=g_norm(1e-12, "norm_p1e12", True), norm_m1e12=g_norm(-1e-12, "norm_m1e12", True),
           norm_p1e3=g_norm(1e-3, "norm_p1e3", False), norm_m1e3=g_norm(-1e-3, "norm_m1e3", False),
           edge_both=g_edge(200, 60, "edge_both"), edge_only=g_edge(0, 80, "edge_only"),
           edge_none=g_edge(200, 0, "edge_none"), edge_big_last=g_edge_big_last,
           edge_pair_first=g_edge_pair(False), edge_pair_empty_last=g_edge_pair(True))
WANT = dict(six_noisy=_has(ref.GRAD_TOL), far_a=_has(ref.REJECTED), far_b=_has(ref.REJECTED),
            far_c=_has(ref.REJECTED), zero_residual=_has(ref.INVALID), none_valid=_has(ref.INVALID))
# the first seed (from the base's own start) that admit() and WANT accept: `search` prints them.
# far_b: 702 skipped -- its GN twin wanders (steps of 1.4 km), and the oracle's poses there are
# 5e-8 from the yardstick's, over the tenth of the bars tests/test_registration_host.py allows;
# 705 is the next admitted one
SEEDS = dict(clean=100, outliers=201, knee=301, at_solution=400, six_noisy=506, far_a=605, far_b=705, far_c=801,
             zero_residual=900, none_valid=1000, quat_small=1100, quat_large=1201, par_z=1300, two_family=1400,
             par_oblique=1500, po_line=1601, far5km=1700, tiny=1800, norm_p1e12=1900, norm_m1e12=2001,
             norm_p1e3=2100, norm_m1e3=2201, edge_both=2306, edge_only=2477, edge_none=2500,
             edge_big_last=2603, edge_pair_first=2710, edge_pair_empty_last=2802)


COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097)


def run_mask(rng, nv):
    """~50 % valid in runs of 1..40 records, runs straddling records 63|64, 511|512 and
    2047|2048 (a valid run over the first two, an invalid one over the third), exactly nv valid"""
    m = []
    v = 1
    while sum(m) < nv + 200 or len(m) < 2:
        m += [v] * int(rng.integers(1, 41))
        v ^= 1
    m = np.array(m, np.uint8)
    for lo, hi, val in ((56, 72, 1), (504, 520, 1), (2040, 2056, 0)):
        if hi <= len(m):
            m[lo:hi] = val
    cut = int(np.searchsorted(np.cumsum(m), nv)) + 1                # the nv-th valid record ends it
    m = m[:cut]
    assert int(m.sum()) == nv
    return m


def solve_lds_cap():
    """kSolveLdsCap as solve.hip states it (ssf.register_plan does not expose the solve's cap): the
    count tests assert that COUNTS brackets it, so a changed cap cannot leave the LDS / global
    boundary uncovered without a test saying so"""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ssf-slam_amd", "csrc", "solve.hip")
    return int(re.search(r"constexpr int kSolveLdsCap = (\d+);", open(src).read()).group(1))


@functools.lru_cache(maxsize=None)
def count_cases(solver):
    """nv valid records on the kernel's edges (wave, block, kSolveStep T, the kCmpPer T compaction
    pass, kSolveLdsCap), all valid and under a ~50 % mask.  Record i of the current frame pairs
    with last-frame point i, so the mask is the record order's."""
    out = []
    s = "lm" if solver == LM else "gn"
    for masked in (False, True):
        for nv in COUNTS:
            rng = np.random.default_rng(1000 + nv + (7 if masked else 0))
            mask = run_mask(rng, nv) if masked else np.ones(nv, np.uint8)
            c = len(mask)
            po, nr = spread(rng, c, 60.0)
            out.append(build(f"nv{nv}_{'mask' if masked else 'all'}_{s}", "count", solver, po, nr, TRUTH_Q, TRUTH_T,
                             rng.normal(0, 0.002, c), near(rng, TRUTH_Q, TRUTH_T, 1e-4, 0.005), mask=mask,
                             note=dict(nv=nv), rank_deficient=nv < 6,
                             # GN on fewer than 6 records: the Cholesky pivots are rounding noise
                             asserted=not (nv < 6 and solver == GN)))
    return out


@functools.lru_cache(maxsize=None)
def solve_cases():
    """every solve case except the count family, LM cases and their GN twins"""
    return tuple(GEN[b](np.random.default_rng(SEEDS[b]), s) for b in GEN for s in (LM, GN))


# ---------------------------------------------------------------------------- the yardstick's run
_CACHE = {}


def yardstick(case):
    """The yardstick's association and solve of a case (computed once, shared): dict(nn, gap,
    keep, po, pa, n, edges (records or None), enn, egap, sol)."""
    if case.name in _CACHE:
        return _CACHE[case.name]
    q0, t0 = case.pose0[:4], case.pose0[4:]
    nn, gap, keep = ref.associate(case.last, case.curr, q0, t0, case.valid)
    po, pa, n = case.curr[keep, :3], case.last[nn[keep], :3], case.normal[nn[keep]]
    edges = egap = None
    if case.edges is not None:
        last_e, line, lvalid, curr_e = case.edges
        enn, egap, ekeep = ref.associate(last_e, curr_e, q0, t0, lvalid)
        edges = (curr_e[ekeep, :3], line[enn[ekeep], :3], line[enn[ekeep], 3:])
    solve = ref.solve_lm if case.solver == LM else ref.solve_gn
    sol = solve(po, pa, n, q0, t0, case.max_iter, edges)
    out = dict(nn=nn, gap=gap, keep=keep, po=po, pa=pa, n=n, edges=edges, egap=egap, sol=sol)
    _CACHE[case.name] = out
    return out


def compared_rows(case, y):
    """log rows a test compares: all of them, or for a rank-deficient case those before the first
    unclear decision (the final status there may be 3 or 4)"""
    sol = y["sol"]
    if case.solver == GN:
        return len(sol["log"])
    k = ref.clear_rows(sol["margins"])
    return k if case.rank_deficient or case.open_end else len(sol["log"])


def admit(case, y):
    """the checks on the yardstick alone; returns the list of what fails (empty: admitted)"""
    bad = []
    if len(y["gap"]) and y["gap"].min() < 1e-3:
        bad.append(f"association gap {y['gap'].min():.2e}")
    if y["egap"] is not None and len(y["egap"]) and y["egap"].min() < 1e-3:
        bad.append(f"edge association gap {y['egap'].min():.2e}")
    if case.solver == LM and not (case.rank_deficient or case.open_end):
        k = ref.clear_rows(y["sol"]["margins"])
        if k < len(y["sol"]["log"]):
            bad.append(f"unclear decision in row {k}: {y['sol']['margins'][k]}")
    return bad


# ---------------------------------------------------------------------------- comparison
TOL_T, TOL_R = 1e-5, 1e-6          # the project's per-step pose bars (m, rad)


COST_CUT = 1e-12                   # below it a cost is rounding of its own residuals


def cost_floor(y, q, t):
    """What float64 itself leaves uncertain in a cost: each residual is a difference of
    coordinates of size |po| + |pa| + |t| and carries ~16 roundings of 2^-53 of that, so the cost
    sum_i rho'_i |r_i| d r_i cannot be known better.  compare() uses it only where a solve has
    driven the cost itself below COST_CUT (the exactly determined six- and one/two-record cases,
    costs of 7e-14 and less): there a relative bound has nothing else to stand on.  Everywhere
    else the bound is the plain relative one."""
    r = ref._raw_residual(y["po"], y["pa"], y["n"], q, t, y["edges"])
    if not len(r):
        return 0.0
    w = ref._weights(y["po"], y["pa"], y["n"], q, t, y["edges"]) ** 2
    size = lambda a, b: np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1) + np.linalg.norm(t)  # noqa: E731
    mag = size(np.float64(y["po"]), np.float64(y["pa"]))
    if y["edges"] is not None and len(y["edges"][0]):
        mag = np.r_[mag, np.repeat(size(np.float64(y["edges"][0]), np.float64(y["edges"][1])), 3)]
    return float((w * np.abs(r) * 16.0 * 2.0 ** -53 * np.r_[mag, mag]).sum())


def compare(case, y, log, pose, tol_t, tol_r, cost_rtol=1e-9):
    """A solver's log [rows, 10] and final pose [7] for `case` against the yardstick's run y.
    Full-rank cases: the same number of rows and statuses, every row's cost within cost_rtol
    relative (a cost below COST_CUT: within cost_floor(), float64's own uncertainty of it) and
    pose within (tol_t, tol_r).  Rank-deficient cases: cost, statuses through the last clear row,
    and the pose difference PROJECTED on the row space of the yardstick's J at that row's pose; the
    final status may be 3 or 4.  Open-ended cases (rank-deficient, or a last decision that is a
    toss-up): the log is as long as the yardstick's give or take one row, and the final pose is
    compared all the same -- a toss-up between two exits leaves the last accepted pose, and a step
    accepted instead of an exit is one the parameter or function tolerance calls converged.  -> dict(dt, dr, dcost: the worst gaps seen; null: the largest
    null-space displacement (local units), statuses)."""
    sol = y["sol"]
    ylog = sol["log"]
    rows = compared_rows(case, y)
    log = np.asarray(log, np.float64).reshape(-1, 10)
    st, yst = log[:, 8].astype(int).tolist(), ylog[:, 8].astype(int).tolist()
    out = dict(dt=0.0, dr=0.0, dcost=0.0, null=0.0, statuses=st)
    open_end = case.rank_deficient or case.open_end
    if not open_end:
        assert st == yst, (case.name, st, yst)
    else:
        assert st[:rows] == yst[:rows], (case.name, st, yst, rows)
        assert abs(len(st) - len(yst)) <= 1, (case.name, st, yst)
        if case.solver == LM and yst and yst[-1] in (ref.PARAM_TOL, ref.FUNC_TOL):
            assert st[-1] in (ref.PARAM_TOL, ref.FUNC_TOL), (case.name, st, yst)

    def pose_gap(q, t, yq, yt):
        if not case.rank_deficient:
            return float(np.abs(t - yt).max()), ref.quat_angle(q, yq), 0.0
        _, J, _ = ref.evaluate(y["po"], y["pa"], y["n"], yq, yt, y["edges"])
        d = ref.local_delta(q, t, yq, yt)
        if len(J):
            _, sv, Vt = np.linalg.svd(J, full_matrices=False)
            V = Vt[:int((sv > sv[0] * 1e-10).sum())] if sv[0] > 0 else Vt[:0]
        else:
            V = np.zeros((0, 6))
        pr = V.T @ (V @ d)
        return float(np.abs(pr[3:]).max()), 2.0 * float(np.linalg.norm(pr[:3])), float(np.linalg.norm(d - pr))

    def check(q, t, yq, yt, what):
        dt, dr, null = pose_gap(np.asarray(q), np.asarray(t), yq, yt)
        out["dt"], out["dr"], out["null"] = max(out["dt"], dt), max(out["dr"], dr), max(out["null"], null)
        assert dt < tol_t and dr < tol_r, (case.name, what, dt, dr)

    for k in range(rows):
        dc = abs(log[k, 7] - ylog[k, 7])
        if ylog[k, 7] > COST_CUT:
            out["dcost"] = max(out["dcost"], dc / ylog[k, 7])
            assert dc <= cost_rtol * ylog[k, 7], (case.name, k, log[k, 7], ylog[k, 7])
        else:
            floor = cost_floor(y, ylog[k, :4], ylog[k, 4:7])
            assert dc <= cost_rtol * ylog[k, 7] + floor, (case.name, k, log[k, 7], ylog[k, 7], floor)
        check(log[k, :4], log[k, 4:7], ylog[k, :4], ylog[k, 4:7], f"row {k}")
    check(pose[:4], pose[4:], sol["q"], sol["t"], "final pose")
    if yst and all(s == ref.INVALID for s in yst):            # no step taken: the warm start, bit for bit
        assert np.array_equal(np.asarray(pose, np.float64), case.pose0), (case.name, pose)
    return out


def check_unasserted(case, y, log, pose):
    """the little that holds for a case whose decisions are rounding noise (asserted=False): the
    pose is finite, and where the yardstick's solve ends on an invalid step, so does this one"""
    log = np.asarray(log, np.float64).reshape(-1, 10)
    assert np.all(np.isfinite(pose)) and np.all(np.isfinite(log)), (case.name, pose)
    ylog = y["sol"]["log"]
    if len(ylog) and ylog[-1, 8] == ref.INVALID:
        assert len(log) and log[-1, 8] == ref.INVALID, (case.name, log[:, 8])


# ---------------------------------------------------------------------------- plane-fit families
# angle(n_float32_fit, n_yardstick) <= FIT_C * kappa(A) * 2^-24 on full-rank sets: four times (the
# GPU host's libm and compiler) the worst ratio measured with the CPU oracle over fit_frames()
# (FIT_WORST, printed by tests/test_registration_host.py)
FIT_WORST = 1.634
FIT_C = 4.0 * FIT_WORST


def _frame6(A, rng):
    """a 6-point last frame whose point 0 fits exactly the rows of A: the five points, then a
    sixth of the same scan row 0.9 m from A[0] (the gated 6th neighbour, d2 = 0.81 < 1)"""
    A = np.asarray(A, np.float64)
    far = A[0] + 0.9 * unit(rng.normal(size=3))
    xyz = np.concatenate([A, far[None]])
    return np.c_[xyz, np.arange(6) + 0.07].astype(np.float32)


def _on_plane(rng, n, d, k=5, spread_m=0.25):
    """k points within spread_m of a point of the plane n . x + d = 0"""
    n = unit(n)
    c = -d * n + np.cross(n, unit(rng.normal(size=3))) * rng.uniform(0, 3)
    a = unit(np.cross(n, rng.normal(size=3)))
    b = np.cross(n, a)
    uv = rng.uniform(-spread_m, spread_m, (k, 2))
    return c + uv[:, :1] * a + uv[:, 1:] * b


def _fit_of(frame, plane_max):
    pk = ref.plane_pick(frame, 0)
    return pk, ref.plane_fit5(frame[pk["pick"], :3], plane_max)


@functools.lru_cache(maxsize=None)
def fit_frames():
    """[(name, last [6, 4] f32, plane_max, kind)] for point 0 of each frame: kind full (rank 3:
    planes 2 .. 80 m and 1 cm from the origin), rank2 (collinear), rank1 (five copies), edge (the
    largest |dd| 10x the float32 error of a dd either side of plane_max, 0.05 and the 16-row 0.15)."""
    out = []
    rng = np.random.default_rng(201)
    for d in (2.0, 5.0, 10.0, 20.0, 40.0, 80.0):
        for j in range(3):
            A = _on_plane(rng, rng.normal(size=3), d) + rng.normal(0, 0.004, (5, 3))
            out.append((f"plane_{int(d)}m_{j}", _frame6(A, rng), 0.05, "full"))
    for j in range(3):
        out.append((f"plane_1cm_{j}", _frame6(_on_plane(rng, rng.normal(size=3), 0.01), rng), 0.05, "full"))
    p0, dirn = np.array([4.0, -3.0, 1.5]), unit([1.0, 2.0, -0.5])
    out.append(("collinear", _frame6(p0 + np.outer([0.0, 0.05, -0.1, 0.2, -0.3], dirn), rng), 0.05, "rank2"))
    out.append(("collinear_dyadic", _frame6(np.array([8.0, -4.0, 2.0]) + np.outer([0, 1, -2, 3, -4], [0.0625, 0.125, -0.03125]),
                                            rng), 0.05, "rank2"))
    out.append(("five_copies", _frame6(np.tile([[6.5, -2.25, 1.125]], (5, 1)), rng), 0.05, "rank1"))
    def edge_frame(base, n, far, h, pm):
        A = base + np.outer([1.0, -1.0, 1.0, -1.0, 1.0], n) * h      # alternate sides of the plane
        fr = np.c_[np.concatenate([A, (A[0] + 0.9 * far)[None]]), np.arange(6) + 0.07].astype(np.float32)
        pk, fit = _fit_of(fr, pm)
        P = fr[pk["pick"], :3].astype(np.float64)
        # float32 error of a dd: the normal's, kappa 2^-24, times the 0.5 m the points span
        return fr, np.abs((P[:4] - P[1:]) @ fit["normal"]).max(), fit["kappa"] * 2.0 ** -24 * 0.5

    for pm in (0.05, 0.15):
        for side in (-1, 1):
            for j in range(2):
                while True:                              # a configuration whose max |dd| crosses plane_max
                    n = unit(rng.normal(size=3))
                    base = _on_plane(rng, n, 10.0)
                    far = unit(np.cross(n, rng.normal(size=3)))
                    hs = np.linspace(0.0, 0.3, 61)
                    dd = np.array([edge_frame(base, n, far, h, pm)[1] for h in hs])
                    up = np.nonzero((dd[:-1] < 0.98 * pm) & (dd[1:] > 1.02 * pm))[0]
                    if len(up):
                        break
                lo, hi = hs[up[0]], hs[up[0] + 1]
                for _ in range(60):                      # bisect to max |dd| = plane_max + side * 10 err
                    h = 0.5 * (lo + hi)
                    fr, d, err = edge_frame(base, n, far, h, pm)
                    miss = d - (pm + side * 10.0 * err)
                    if abs(miss) < 2.0 * err:
                        break
                    lo, hi = (lo, h) if miss > 0 else (h, hi)
                assert abs(miss) < 2.0 * err, (pm, side, j, miss, err)
                out.append((f"edge_{pm}_{'above' if side > 0 else 'below'}_{j}", fr, pm, "edge"))
    return out


@functools.lru_cache(maxsize=None)
def pick_frames():
    """last frames for the pick logic (:173-205): m in {4, 5, 11, 29, 30, 31} points; 0, 1 and 2
    other-row points found at ranks 5..29; a 6th-neighbour d2 just inside / outside 1 m^2.
    -> [(name, last [m, 4] f32, plane_max)]."""
    out = []
    rng = np.random.default_rng(211)
    for m in (4, 5, 11, 29, 30, 31):
        xyz = np.c_[rng.uniform(0, 1.5, (m, 2)) + 8.0, np.full(m, -1.7) + rng.normal(0, 0.002, m)]
        rows = rng.integers(0, 4, m)
        out.append((f"m{m}", np.c_[xyz, np.arange(m) + rows / 100.0].astype(np.float32), 0.05))
    for other in (0, 1, 2):
        m = 40
        xyz = np.c_[8.0 + 0.02 * np.arange(m), np.full(m, 3.0), np.full(m, -1.7)] + rng.normal(0, 0.001, (m, 3))
        rows = np.full(m, 7)
        for k in range(other):
            rows[9 + 8 * k] = 9
        xyz[rows == 9, 1] += 0.01
        out.append((f"other{other}", np.c_[xyz, np.arange(m) + rows / 100.0].astype(np.float32), 0.05))
    for tag, d in (("inside", 0.999), ("outside", 1.001)):
        xyz = np.array([[5.0, 0, 0], [5.1, 0.05, 0.01], [5.0, 0.12, 0], [4.9, 0.03, -0.01], [5.05, -0.1, 0],
                        [5.0 + np.sqrt(d), 0, 0]] + [[50.0 + 3 * k, 0, 0] for k in range(6)])
        out.append((f"gate_{tag}", np.c_[xyz, np.arange(len(xyz)) + 0.07].astype(np.float32), 0.05))
    return out


def wall_scene(seed=0):
    """A last / current frame pair of three orthogonal walls (scan rows along one axis of each),
    for orc_register_pair / Frontend.register with the frame's OWN plane table."""
    rng = np.random.default_rng(seed)
    pts, rows = [], []
    for axis, level in ((2, -1.7), (0, 9.0), (1, -7.0)):
        u, v = np.meshgrid(np.arange(14) * 0.31, np.arange(14) * 0.37)
        g = np.zeros((u.size, 3))
        a, b = [k for k in range(3) if k != axis]
        g[:, a] = u.ravel() + (2.0 if axis else 3.0)
        g[:, b] = v.ravel() - 2.0
        g[:, axis] = level
        g += rng.normal(0, 0.02, g.shape) * (np.arange(3) != axis) + rng.normal(0, 0.002, g.shape) * (np.arange(3) == axis)
        pts.append(g)
        rows.append(np.repeat(np.arange(14), 14) % 64)
    xyz, rows = np.concatenate(pts), np.concatenate(rows)
    last = np.c_[xyz, np.arange(len(xyz)) + rows / 100.0].astype(np.float32)
    moved = xyz + rng.normal(0, 0.01, xyz.shape)
    curr_xyz = ref.quat_rotate(ref.quat_conj(TRUTH_Q), moved - TRUTH_T)
    curr = np.c_[curr_xyz, last[:, 3]].astype(np.float32)
    return last, curr, near(rng, TRUTH_Q, TRUTH_T, 0.002, 0.03)


def wall_edges(seed=1):
    """edge clouds to go with wall_scene(): the walls' three corner lines, 36 points each 0.17 m
    apart with 5 mm of jitter, and the current frame's copy moved back by the true pose"""
    rng = np.random.default_rng(seed)
    pts = []
    for p0, d in (([9.0, -7.0, -1.7], [0, 0, 1.0]), ([9.0, -2.0, -1.7], [0, 1.0, 0]), ([3.0, -7.0, -1.7], [1.0, 0, 0])):
        pts.append(np.asarray(p0) + np.outer(0.17 * np.arange(36), d) + rng.normal(0, 0.005, (36, 3)))
    xyz = np.concatenate(pts)
    last_e = np.c_[xyz, np.arange(len(xyz)) + 0.03].astype(np.float32)
    moved = xyz + rng.normal(0, 0.01, xyz.shape)
    curr_e = np.c_[ref.quat_rotate(ref.quat_conj(TRUTH_Q), moved - TRUTH_T), last_e[:, 3]].astype(np.float32)
    return last_e, curr_e


def _search(base, start, tries=400):
    for seed in range(start, start + tries):
        _CACHE.clear()
        ok = True
        for solver in (LM, GN):
            cs = GEN[base](np.random.default_rng(seed), solver)
            y = yardstick(cs)
            ok = ok and not admit(cs, y)
            if solver == LM and ok:
                ok = WANT.get(base, lambda y: True)(y)
            if ok and cs.family == "quat":
                ok = quat_paths_clear(y, cs.pose0, base == "quat_large")
        if ok:
            return seed
    raise RuntimeError(f"no seed for {base}")


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["search"]:
        print("SEEDS = dict(" + ", ".join(f"{b}={_search(b, 100 * (k + 1))}" for k, b in enumerate(GEN)) + ")")
    else:
        for cs in solve_cases() + tuple(count_cases(LM)) + tuple(count_cases(GN)):
            y = yardstick(cs)
            print(cs.name, len(y["po"]), y["sol"]["log"][:, 8].astype(int).tolist(), y["sol"]["rank"],
                  compared_rows(cs, y), admit(cs, y))

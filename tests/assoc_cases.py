"""Seeded inputs that pin the plane association's 1-NN search (k_associate_strips and the brute
k_associate) to tests/registration_reference.associate_exact, shared by tests/test_assoc_host.py
(the CPU oracle against the yardstick) and tests/test_gpu_assoc_yardstick.py (the device).

A case is one pair as a registration_cases.Case (GN, max_iter 1): a last cloud [m, 4], m > 10
(the :158 gate), with seeded unit normals and a seeded valid mask (~30 % zeros) for its plane
table, a current cloud and a warm start.  The last cloud is shuffled, so index order is never
spatial order.  Queries are designed in the last frame (where the search runs) and moved back
through the inverse of the warm start.

Admission is the yardstick's alone: every query's gap (second-best d2 - best d2) / second-best d2
is >= 1e-3 (registration_cases.admit's rule); a query that misses it is REDRAWN, never dropped --
more than 25 % of a case's queries redrawn, or 5 rounds that do not suffice, raise.  The tie
family is the exception: its gap is exactly 0 by construction (small integers and halves, identity
rotation, integer translation: float32 and float64 arithmetic are both exact) and the lowest
original index must win.  All coordinates stay inside +-20 km.

Families (FAMILIES): levels (a 1-NN at 0.98 R and 1.02 R of every search radius R = 2 .. 4096 m
and beyond, along x, along y and diagonally, with rejected candidates in many strips and a z-decoy
per query), hole (an annulus scan with a masked sector), edges (points exactly on the strip
boundaries), empty (two y bands 150 m apart), extent (one y, one x, 800 m and 30 km of y, a
12-point frame), far (a scene 5.8 km out), ties.
"""
import functools
import os
import re

import numpy as np

import registration_cases as rc
import registration_reference as ref

GAP = 1e-3                 # registration_cases.admit's association rule
BOX = 20000.0              # every coordinate inside +-BOX
FAMILIES = ("levels", "hole", "edges", "empty", "extent", "far", "ties")
IDENT = np.array([0.0, 0.0, 0.0, 1.0])
F32 = np.float32


def _const(name):
    """a constexpr of reg_strips.hpp as the header states it"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ssf-slam_amd", "csrc", "reg_strips.hpp")
    return int(re.search(r"constexpr int " + name + r" = (\d+);", open(src).read()).group(1))


STRIP_MAX = _const("kStripMax")                # strips per frame
STRIP_W = F32(1.001)                           # the narrowest strip (strips_build)
IMAGE_MIN = (STRIP_MAX + 1) + 2 * STRIP_MAX + 4   # kStripHeadWords: the smallest imaged last frame
IMAGE_MAX = _const("kAssocStripF4Max")         # the largest frame staged as float4 (and imaged)
SOA_MAX = _const("kAssocStripSoaMax")          # the LDS staging capacity; a larger last frame is walked in global memory


# ---------------------------------------------------------------------------- the strip layout
def strip_geometry(y):
    """(y0, W, invW, ns) of a last frame as strips_build states them, in float32: where the strip
    boundaries of a case fall is the layout's arithmetic, so the cases that sit ON a boundary
    compute it the same way.  Nothing of the search itself is restated here."""
    y = np.asarray(y, F32)
    y0, y1 = y.min(), y.max()
    W = max(STRIP_W, F32(F32(y1 - y0) / F32(STRIP_MAX - 1)))
    invW = F32(F32(1.0) / W)
    ns = min(STRIP_MAX, int(F32(F32(y1 - y0) * invW)) + 1)
    return y0, W, invW, ns


def strip_of(y, geo):
    y0, _, invW, ns = geo
    return np.clip((F32(np.asarray(y, F32) - y0) * invW).astype(np.int64), 0, ns - 1)


def nominal_edge(k, geo):
    """y0 + k W as the search's ring stop computes it"""
    return F32(geo[0] + F32(F32(k) * geo[1]))


# ---------------------------------------------------------------------------- building a case
def _to_curr(S, pose0):
    q, t = pose0[:4], pose0[4:]
    return ref.quat_rotate(ref.quat_conj(q), np.asarray(S, np.float64) - t)


_Y = {}


def finish(name, family, last_xyz, make, nq, pose0, seed, tie=False):
    """Shuffle the last cloud, draw the table (normals, valid), draw the queries with
    make(rng, slots) -> [len(slots), 3] (last-frame coordinates) and redraw those the yardstick
    does not admit.  note: redrawn (queries redrawn at least once), rounds, nq."""
    rng = np.random.default_rng(seed)
    last_xyz = np.asarray(last_xyz, np.float64)
    m = len(last_xyz)
    assert m > 10, name
    last = rc._xyzi(last_xyz[rng.permutation(m)])
    normal = rc.unit(rng.normal(size=(m, 3))).astype(F32)
    valid = (rng.random(m) >= 0.3).astype(np.uint8)
    pose0 = np.asarray(pose0, np.float64)
    S = np.asarray(make(rng, np.arange(nq)), np.float64)
    redrawn = np.zeros(nq, bool)
    rounds = 0
    while True:
        curr = rc._xyzi(_to_curr(S, pose0))
        nn, gap, keep = ref.associate_exact(last, curr, pose0[:4], pose0[4:], valid)
        bad = np.zeros(nq, bool) if tie else gap < GAP
        if not bad.any():
            break
        if rounds == 5:
            raise RuntimeError(f"{name}: 5 rounds of redraws do not suffice ({int(bad.sum())} queries left)")
        redrawn |= bad
        if redrawn.sum() > 0.25 * nq:
            raise RuntimeError(f"{name}: {int(redrawn.sum())} of {nq} queries redrawn")
        S[bad] = make(rng, np.flatnonzero(bad))
        rounds += 1
    case = rc.Case(name, family, last, normal, valid, curr, pose0, rc.GN, 1,
                   note=dict(redrawn=int(redrawn.sum()), rounds=rounds, nq=nq, tie=tie))
    assert max(np.abs(last[:, :3]).max(), np.abs(curr[:, :3]).max()) < BOX, name
    _Y[name] = dict(nn=nn, gap=gap, keep=keep)
    return case


def yardstick(case):
    """associate_exact's run of a case (computed at admission, shared) and, on demand, one
    Gauss-Newton step on its records: dict(nn, gap, keep, po, pa, n, sol)."""
    y = _Y[case.name]
    if "sol" not in y:
        nn, keep = y["nn"], y["keep"]
        y["po"], y["pa"], y["n"] = case.curr[keep, :3], case.last[nn[keep], :3], case.normal[nn[keep]]
        y["edges"] = None
        y["sol"] = ref.solve_gn(y["po"], y["pa"], y["n"], case.pose0[:4], case.pose0[4:], 1)
    return y


def admit(case):
    """the checks on the yardstick alone; the list of what fails (empty: admitted)"""
    y, bad = _Y[case.name], []
    if case.note["tie"]:
        if np.any(y["gap"] != 0.0):
            bad.append(f"tie case with gap {y['gap'].max():.2e}")
    elif y["gap"].min() < GAP:
        bad.append(f"association gap {y['gap'].min():.2e}")
    if case.note["redrawn"] > 0.25 * case.note["nq"] or case.note["rounds"] > 5:
        bad.append(f"{case.note['redrawn']} redrawn in {case.note['rounds']} rounds")
    if not len(case.last) > 10:
        bad.append("last frame of at most 10 points")
    return bad


SOLVE_REACH = 300.0        # m: the one-step solve is compared on cases within this of the origin
SOLVE_SV = 1e-3            # ... whose Jacobian is this well conditioned in the yardstick's run


def solve_compared(case):
    """'' when the one-step solve of this case is compared with the yardstick's, else the reason
    it is not (admission on the reference alone)"""
    reach = max(np.abs(case.last[:, :3]).max(), np.abs(case.curr[:, :3]).max())
    if reach > SOLVE_REACH:
        return f"coordinates to {reach:.0f} m"
    sv = yardstick(case)["sol"]["sv_ratio"]
    if not (len(sv) and sv[0] >= SOLVE_SV):
        return f"sv_ratio {sv[0] if len(sv) else 0.0:.1e}"
    return ""


def _box(rng, n, lo, hi):
    return rng.uniform(np.asarray(lo, np.float64), np.asarray(hi, np.float64), (n, 3))


SMALL_Q = rc.axis_angle_quat([0.1, -0.2, 1.0], 0.03)
SMALL_POSE = np.r_[SMALL_Q, 0.8, -0.1, 0.05]


# ---------------------------------------------------------------------------- levels
DIRS = rc.unit(np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0]], np.float64))
LEVELS = tuple(range(1, 14))       # R = 2^e: the levels 2 .. 4096 m, and 8192 (the unbounded pass)


def g_level(e, seed):
    """Two cells 7 R apart in x (20 km from R = 4096 on).  Cell A: eight last points at 0.98 R
    from its centre (+-x: the query's own strip; +-y: strips away; the diagonals), cell B the same
    at 1.02 R.  Sixteen queries per cell, 0.006 R off the centre towards one of the eight -- its
    1-NN, 0.3 % of d2 clear of the two next to it.  Under (over) every query a z-decoy, a last
    point at dx = dy = 0 and |dz| = 1.1 .. 1.9 R: its strip lower bound is 0, the level R visits it
    first and must go on.  e <= 5 adds a third cell like A, 6 R up in z (three query clusters: the
    one-step solve is well conditioned).  380 (250 with three cells) more last points per cell at 1.1 .. 2.5 R in all directions: many
    strips hold candidates to reject.  e <= 6: |dy| <= 1.9 R keeps the y extent under 255 m
    (W = 1.001 m, up to 64 rings); larger e widen W.  e = 13: no level holds the 1-NN (the
    unbounded pass); cell A's decoys sit at 0.985 .. 0.995 R, inside the last level's 2 x 4096 m."""
    R = 2.0 ** e
    rng = np.random.default_rng(seed)
    cx = min(3.5 * R, 10000.0)
    centres = [np.array([-cx, 0.0, 0.0]), np.array([cx, 0.0, 0.0])]
    if e <= 5:                     # a third cell off the line of the two: a well-conditioned one-step solve
        centres.append(np.array([0.0, 0.0, 6.0 * R]))
    per = 380 if e > 5 else 250
    pts, spots = [], []
    for C, f in zip(centres, (0.98, 1.02, 0.98)):
        pts.append(C + f * R * DIRS)
        for u in DIRS:
            for _ in range(2):
                spot = C + 0.006 * R * rng.uniform(0.8, 1.2) * u + 0.0001 * R * rng.normal(size=3) * [1, 1, 0]
                spot = spot.astype(F32).astype(np.float64)              # dx = dy = 0 exactly
                lo, hi = (0.985, 0.995) if (e == 13 and f < 1) else (1.1, 1.9)
                spots.append(spot)
                pts.append((spot + [0, 0, R * rng.uniform(lo, hi) * rng.choice([-1, 1])])[None])
        got = np.zeros((0, 3))
        while len(got) < per:
            p = C + R * rng.uniform(1.1, 2.5, (2000, 1)) * rc.unit(rng.normal(size=(2000, 3)))
            ok = np.all(np.abs(p) <= BOX - 500.0, axis=1)
            for C2 in centres:
                ok &= np.linalg.norm(p - C2, axis=1) >= 1.1 * R
            if e <= 6:
                ok &= np.abs(p[:, 1]) <= 1.9 * R
            got = np.concatenate([got, p[ok]])
        pts.append(got[:per])
    spots = np.array(spots)

    def make(rng, slots):
        return spots[slots] + np.c_[np.zeros((len(slots), 2)), 0.001 * R * rng.uniform(-1, 1, len(slots))]
    return finish(f"level_{int(R)}", "levels", np.concatenate(pts), make, len(spots), np.r_[IDENT, 0, 0, 0], seed + 1)


# ---------------------------------------------------------------------------- hole
SECTOR = (0.5, 1.9)                # the masked azimuths (rad)


def _annulus(rng, n):
    out = np.zeros((0, 3))
    while len(out) < n:
        r, az = np.sqrt(rng.uniform(25.0, 3600.0, 2 * n)), rng.uniform(0, 2 * np.pi, 2 * n)
        keep = (az < SECTOR[0]) | (az > SECTOR[1])
        out = np.concatenate([out, np.c_[r * np.cos(az), r * np.sin(az), rng.uniform(-2, 2, 2 * n)][keep]])
    return out[:n]


def g_hole(name, m, nq, seed):
    """an annulus scan r = 5 .. 60 m with a masked sector; queries in the centre (r < 3.5 m), in
    the sector (r = 10 .. 55 m, 0.15 rad off its sides) and outside the rim (r = 62 .. 200 m)"""
    last = _annulus(np.random.default_rng(seed), m)

    def make(rng, slots):
        k = len(slots)
        kind = slots % 3
        r = np.where(kind == 0, rng.uniform(0, 3.5, k), np.where(kind == 1, rng.uniform(10, 55, k), rng.uniform(62, 200, k)))
        az = np.where(kind == 1, rng.uniform(SECTOR[0] + 0.15, SECTOR[1] - 0.15, k), rng.uniform(0, 2 * np.pi, k))
        return np.c_[r * np.cos(az), r * np.sin(az), rng.uniform(-2, 2, k)]
    return finish(name, "hole", last, make, nq, SMALL_POSE, seed + 1)


# ---------------------------------------------------------------------------- strip edges
def g_edges(seed):
    """20 last points on each of y0 + k fl(1.001), k = 0 .. 39 (float32, as the ring stop forms
    them); queries on the edges and 0.45 m either side, 0.3 m and 5 m below y0 and above y1, and
    300 m outside the extent (the clamp of strip_of).  Identity rotation and no y translation:
    every y arrives exactly."""
    rng = np.random.default_rng(seed)
    y0 = F32(-20.0)
    yk = np.array([F32(y0 + F32(F32(k) * STRIP_W)) for k in range(40)], F32)
    # x stratified (2 m cells, 0.8 m and more apart), so that a query far outside has one nearest corner
    last = np.c_[np.tile(-20.0 + 2.0 * np.arange(20), 40) + rng.uniform(0, 1.2, 800), np.repeat(yk, 20).astype(np.float64),
                 rng.uniform(-2, 2, 800)]
    ys = [F32(y + F32(d)) for y in yk for d in (0.0, -0.45, 0.45)]
    for d in (0.3, 5.0, 300.0):
        ys += [F32(yk[0] - F32(d))] * 4 + [F32(yk[-1] + F32(d))] * 4
    ys = np.array(ys, np.float64)

    far = np.abs(ys - float(y0)) > 200.0       # 300 m out: off in x as well, or no neighbour stands clear

    def make(rng, slots):
        x = np.where(far[slots], rng.uniform(250, 350, len(slots)) * rng.choice([-1, 1], len(slots)), rng.uniform(-20, 20, len(slots)))
        return np.c_[x, ys[slots], rng.uniform(-2, 2, len(slots))]
    return finish("strip_edges", "edges", last, make, len(ys), np.r_[IDENT, 0.5, 0.0, -0.25], seed + 1)


# ---------------------------------------------------------------------------- empty strips
def g_empty(seed):
    """two y bands 150 m apart (~150 empty strips between them); queries everywhere between and
    a few metres beyond"""
    rng = np.random.default_rng(seed)
    last = np.concatenate([_box(rng, 450, [-30, 0, -2], [30, 3, 2]), _box(rng, 450, [-30, 153, -2], [30, 156, 2])])

    def make(rng, slots):
        return _box(rng, len(slots), [-30, -5, -2], [30, 161, 2])
    return finish("empty_strips", "empty", last, make, 96, SMALL_POSE, seed + 1)


# ---------------------------------------------------------------------------- extent
def g_box(name, family, lo, hi, qlo, qhi, m, nq, pose0, seed, fix=None):
    """m last points uniform in [lo, hi] (fix = (axis, value): one coordinate shared by all),
    nq queries uniform in [qlo, qhi]"""
    rng = np.random.default_rng(seed)
    last = _box(rng, m, lo, hi)
    if fix is not None:
        last[:, fix[0]] = fix[1]

    def make(rng, slots):
        return _box(rng, len(slots), qlo, qhi)
    return finish(name, family, last, make, nq, pose0, seed + 1)


Y30_FAR = 56               # strip boundaries at the far end of the 30 km case


def y30_boundaries(geo):
    """[(su, lowest float32 y of strip su)] for the Y30_FAR boundaries below the top strip's"""
    out = []
    for su in range(geo[3] - 1 - Y30_FAR, geo[3] - 1):
        y = nominal_edge(su, geo)
        while strip_of(y, geo) >= su:
            y = np.nextafter(y, F32(-np.inf))
        while strip_of(y, geo) < su:
            y = np.nextafter(y, F32(np.inf))
        out.append((su, y))
    return out


def g_y30km(seed):
    """y extent 30 km (W = 117.6 m; the float32 ulp of y is ~1 mm at the far end, and the strip a
    point falls in is decided by fl(fl(y - y0) invW)).  The extent is set by two last points at
    y = -+15000 and every other point lies strictly inside, so the layout used here is the layout
    of the finished cloud (tests/test_assoc_host.py asserts it).  For each of Y30_FAR strip
    boundaries at the far end, found by strip_geometry / strip_of: the LOWEST float32 y the layout
    puts in strip su, as a last point P, a query 1 .. 1.4 m below it (in strip su - 1) and a
    competitor C below the query, farther than P by the gap rule (d2 1.05e-3 relative) and no
    more; and the mirror image -- the HIGHEST y of strip su - 1, a query above it (in strip su), a
    competitor above the query.  P, C share x and z; the query is up to 2 cm off them.  600 more
    last points fill the extent 50 m and more away in x."""
    rng = np.random.default_rng(seed)
    fill = np.concatenate([_box(rng, 598, [-50, -14990, -5], [50, 14990, 5]), [[0, -15000.0, 0], [0, 15000.0, 0]]])
    geo = strip_geometry(fill[:, 1])
    pts, anchors = [], []
    for j, (su, y) in enumerate(y30_boundaries(geo)):
        for sign, py in ((-1.0, y), (1.0, np.nextafter(y, F32(-np.inf)))):
            x, z = 100.0 + 3.0 * (2 * j + (sign > 0)), float(rng.uniform(-5, 5))
            qy = F32(py + F32(sign * rng.uniform(1.0, 1.4)))
            d = abs(float(qy) - float(py))
            cy = F32(float(qy) + sign * d * 1.0004)
            gap_of = lambda dc: (dc * dc - d * d) / (dc * dc)                                   # noqa: E731
            while gap_of(abs(float(cy) - float(qy))) < 1.05 * GAP:
                cy = np.nextafter(cy, F32(sign * np.inf))
            pts += [[x, float(py), z], [x, float(cy), z]]
            anchors.append([x, float(qy), z])
    anchors = np.array(anchors)
    assert np.abs(np.array(pts)[:, 1]).max() < 15000.0

    def make(rng, slots):
        return anchors[slots] + np.c_[rng.uniform(-0.02, 0.02, len(slots)), np.zeros(len(slots)), rng.uniform(-0.02, 0.02, len(slots))]
    cs = finish("y30km", "extent", np.concatenate([fill, pts]), make, len(anchors), np.r_[IDENT, 0, 0, 0], seed + 1)
    assert strip_geometry(cs.last[:, 1]) == geo
    return cs


# ---------------------------------------------------------------------------- ties
def _lattice(step, nx, ny, nz, x0):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g * float(step) + [x0, 0.0, 0.0]


# (A, B) offsets from a query: |A|^2 = |B|^2 = 9, 9, 25, 36, 17, 65; planar A: 0 or 1 (level 2);
# planar B: 8, 5 (level 4), 25, 32, 17 (level 8), 65 (level 16)
CROSS = [(np.array(a, np.float64), np.array(b, np.float64)) for a, b in
         (((0, 0, 3), (2, 2, 1)), ((0, 0, 3), (1, 2, 2)), ((0, 0, 5), (3, 4, 0)), ((0, 0, 6), (4, 4, 2)),
          ((1, 0, 4), (1, 4, 0)), ((0, 1, 8), (7, 4, 0)))]


def g_ties(seed):
    """Three integer lattices side by side in x, spacing 2 m (10 x 10 x 8), 4 m and 8 m, and 24
    exact duplicates of points of the first.  Queries at cell centres (8-way ties), face centres
    (4-way), edge midpoints (2-way; next to a duplicate 3-way) and on duplicated points (d2 = 0
    twice).  Tied candidates lie two and more strips apart in y (W = 1.001 m), so the group mode
    finds them in different lanes; the tied d2 are 1, 2, 3 (level 2), 4 (= the level's R^2), 8, 12
    (level 4), 16 (= R^2), 32, 48 (level 8).  24 more queries have two tied candidates that become
    reachable at DIFFERENT levels (CROSS).  The lowest original index wins; the shuffle decides
    which point that is."""
    rng = np.random.default_rng(seed)
    lat = [(_lattice(2, 10, 10, 8, 0.0), 2, (10, 10, 8), 0.0), (_lattice(4, 4, 5, 4, 40.0), 4, (4, 5, 4), 40.0),
           (_lattice(8, 4, 3, 3, 100.0), 8, (4, 3, 3), 100.0)]
    dup = lat[0][0][rng.choice(800, 24, replace=False)]
    last = np.concatenate([lat[0][0], lat[1][0], lat[2][0], dup])
    qs = []
    for _, step, n, x0 in lat:
        for half in ((1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            for _ in range(8):
                cell = np.array([rng.integers(0, n[k] - half[k]) for k in range(3)])
                qs.append((cell + 0.5 * np.array(half)) * step + [x0, 0.0, 0.0])
    for p in dup[:12]:
        qs.append(p)                                                    # on a duplicated point
        qs.append(p + [1.0, 0.0, 0.0] if p[0] < 18 else p - [1.0, 0.0, 0.0])   # an edge midpoint next to it
    # ties across levels: two candidates of equal d2 and unequal planar offsets, alone around
    # their query -- A is reachable (dx^2 + dy^2 <= R^2) at level 2 with d2 beyond that level, B
    # only one to three levels later, where the tie is met
    cross = []
    for k, (a, b) in enumerate(CROSS * 4):
        c = np.array([160.0 + 25.0 * (k % 6), 8.0, 40.0 + 30.0 * (k // 6)])
        sa, sb = rng.choice([-1.0, 1.0], 3), rng.choice([-1.0, 1.0], 3)
        cross += [c + sa * a, c + sb * b]
        qs.append(c)
    last = np.concatenate([last, cross])
    qs = np.array(qs)

    def make(rng, slots):
        return qs[slots]
    return finish("ties", "ties", last, make, len(qs), np.r_[IDENT, 4.0, -6.0, 2.0], seed + 1, tie=True)


def first_level(planar2):
    """the first search radius R = 2, 4, ... whose R^2 holds a planar offset dx^2 + dy^2"""
    R = 2.0
    while planar2 > R * R:
        R *= 2.0
    return R


# ---------------------------------------------------------------------------- the registry
FAR_C = np.array([5000.0, -3000.0, 100.0])


def _far_pose():
    """the small rotation about the far scene's own centre"""
    return np.r_[SMALL_Q, FAR_C - ref.quat_rotate(SMALL_Q, FAR_C) + [0.8, -0.1, 0.05]]


@functools.lru_cache(maxsize=None)
def cases():
    """every case whose frames fit 1024 points (every launch shape takes them)"""
    out = [g_level(e, 3000 + 10 * e) for e in LEVELS]
    out.append(g_hole("hole", 900, 192, 3200))
    out.append(g_edges(3300))
    out.append(g_empty(3400))
    out.append(g_box("one_y", "extent", [-50, 0, -5], [50, 0, 5], [-60, 1.25, -6], [60, 13.25, 6], 800, 96, SMALL_POSE, 3500, fix=(1, 7.25)))
    out.append(g_box("one_x", "extent", [0, -40, -5], [0, 40, 5], [-2.5, -45, -6], [9.5, 45, 6], 800, 96, SMALL_POSE, 3510, fix=(0, 3.5)))
    out.append(g_box("y800", "extent", [-30, -400, -3], [30, 400, 3], [-35, -420, -4], [35, 420, 4], 900, 96, SMALL_POSE, 3520))
    out.append(g_y30km(3530))
    out.append(g_box("tiny12", "extent", [-5, -5, -5], [5, 5, 5], [-8, -8, -8], [8, 8, 8], 12, 24, SMALL_POSE, 3540))
    out.append(g_box("far_origin", "far", FAR_C - 30, FAR_C + 30, FAR_C - 35, FAR_C + 35, 800, 96, _far_pose(), 3600))
    out.append(g_ties(3700))
    assert {c.family for c in out} == set(FAMILIES)
    assert all(max(len(c.last), len(c.curr)) <= 1024 for c in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hole_big():
    """the hole scan with more than 1024 queries (the lane mode's second work-group of a pair)"""
    return g_hole("hole_big", 900, 1500, 3210)


@functools.lru_cache(maxsize=None)
def hole_dense():
    """the hole scan densified to one point more than the LDS staging holds: the global-memory walk"""
    return g_hole("hole_dense", SOA_MAX + 1, 300, 3220)


def family(name, big=False):
    return [c for c in cases() if c.family == name] + ([hole_big()] if big and name == "hole" else [])


def tile(cs, P):
    return [cs[p % len(cs)] for p in range(max(P, len(cs)))]


def rows(name):
    """The launch shapes one family goes through, the smallest that reach each path of the
    association: (row, cases, table mode of the launch helper, max_points bound or None for the
    largest frame, what ssf.register_plan must say).  The bound may exceed the real frames."""
    small, big = family(name), family(name, big=True)
    assert any(IMAGE_MIN <= len(c.last) <= IMAGE_MAX for c in small), name
    assert len(small) <= 16
    return [("group_f4_own", small, "own_strips", None, dict(strip_path=True, group_mode=True, soa=False)),
            ("group_image", small, "sorted", None, dict(strip_path=True, group_mode=True, soa=False)),
            ("group_soa", small, "sorted", IMAGE_MAX + 1, dict(strip_path=True, group_mode=True, soa=True)),
            ("lane_split", tile(big, 17), "sorted", 2048, dict(strip_path=True, group_mode=False, soa=False, qsplit=2, compacted=False)),
            ("lane_compacted", tile(small, 17), "sorted", 1024, dict(strip_path=True, group_mode=False, soa=False, qsplit=1, compacted=True)),
            ("lane_soa", tile(small, 17), "sorted", IMAGE_MAX + 1, dict(strip_path=True, group_mode=False, soa=True, compacted=False)),
            ("brute", small, "brute", None, None)]


def global_rows():
    """the hole family densified: a last frame one point above the staging capacity, walked in
    global memory, in group mode (alone) and in lane mode (with the hole case 16 times)"""
    d = hole_dense()
    want = dict(strip_path=True, soa=True, lds_cap=SOA_MAX)
    return [("global_group", [d], "sorted", None, dict(want, group_mode=True)),
            ("global_lane", [d] + tile(family("hole"), 16), "sorted", None, dict(want, group_mode=False))]


def bound_of(cases_, bound):
    return bound or max(max(len(c.last), len(c.curr)) for c in cases_)


def check_plan(plan, want, what):
    for k, v in (want or {}).items():
        assert plan[k] == v, (what, k, plan)


if __name__ == "__main__":
    for cs in cases() + (hole_big(), hole_dense()):
        y = yardstick(cs)
        d = np.sqrt(((ref.transform_to_last(cs.curr[:, :3], cs.pose0[:4], cs.pose0[4:]).astype(np.float64)
                      - cs.last[y["nn"], :3]) ** 2).sum(1))
        print(f"{cs.name:14s} m {len(cs.last):5d} c {len(cs.curr):4d} redrawn {cs.note['redrawn']:2d} in {cs.note['rounds']} "
              f"rounds, min gap {y['gap'].min():.2e}, 1-NN {d.min():.3g} .. {d.max():.3g} m, kept {int(y['keep'].sum())}, "
              f"solve: {solve_compared(cs) or 'compared'}  {admit(cs)}")

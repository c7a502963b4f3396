"""Seeded case builders for tests/test_feature_host.py, test_gpu_feature_yardstick.py and
test_gpu_voxel_yardstick.py: the smallest clouds that still reach each rule of
src/frameFeature.cpp:45-123 and of pcl::VoxelGrid (tests/feature_reference.py states both).

Every finite point sits on a bin-centre elevation of its profile (ssf.synth.elevations_deg), so
its row does not depend on the precision of atan / sqrt; the host test requires a margin of
1e-3 deg to the nearest bin edge for every finite kept point of every case.

A feature case is a Case: the cloud in row-major order (runs of rows ascending, points that
belong to no row embedded in a run) and, per point, the run it was built into.  layout() turns
one into every input order that launch_extract_planes (features.hip) routes differently.
"""
import functools
from dataclasses import dataclass

import numpy as np

import feature_reference as ref

F32 = np.float32
RANGE_M = 10.0
AZ_STEP = 2 * np.pi / 4200                       # 1.5 cm between neighbours at 10 m
NOISE_M = {64: 0.008, 16: 0.024}                 # range noise: about two thirds are candidates
ZERO_ROW = {64: 6, 16: 8}                        # the row of angle 0 (an overflowed x*x + y*y)
BINNED_POINTS = 128 * 2048                       # frames above this take the binned stage


@dataclass(frozen=True)
class Case:
    name: str
    n_rows: int
    pts: np.ndarray          # [n, 3] float32, row-major
    run: np.ndarray          # [n] the row whose run holds the point (also for dropped points)
    equal_rows: bool = False  # every row the same length: the interleaved order is regular


def _elev(n_rows):
    from ssf import synth
    return synth.elevations_deg(n_rows).numpy()


def polar(n_rows, row, az, rng_m):
    """points of `row` at azimuths az [rad] and ranges rng_m [m], float32"""
    e = np.radians(_elev(n_rows)[row])
    az = np.asarray(az, np.float64)
    r = np.broadcast_to(np.asarray(rng_m, np.float64), az.shape)
    return np.stack([r * np.cos(e) * np.cos(az), r * np.cos(e) * np.sin(az), r * np.sin(e)], 1).astype(F32)


def noisy_row(rng, n_rows, row, n, az0=None):
    az0 = rng.uniform(0, 2 * np.pi) if az0 is None else az0
    return polar(n_rows, row, az0 + AZ_STEP * np.arange(n), RANGE_M + rng.normal(0, NOISE_M[n_rows], n))


def flat_row(n_rows, row, n, az0=0.3):
    """a smooth arc: every point a candidate"""
    return polar(n_rows, row, az0 + AZ_STEP * np.arange(n), RANGE_M)


def _case(name, n_rows, rows, **kw):
    """rows: list of (row, [k, 3] points) in ascending row order"""
    rows = [(r, p) for r, p in rows if len(p)]
    pts = np.concatenate([p for _, p in rows]).astype(F32)
    run = np.concatenate([np.full(len(p), r, np.int64) for r, p in rows])
    assert np.all(np.diff(run) >= 0)
    return Case(name, n_rows, pts, run, **kw)


def in_range(n_rows):
    pr = ref.PROFILES[n_rows]
    return range(pr["row_start"], n_rows - pr["row_end"])


# ------------------------------------------------------------------------------- lengths
def row_lengths(n_rows):
    """the row lengths the family must hold: the j in [5, size - 5) edge (10, 11, 12), the span,
    one candidate word (64)"""
    span = ref.PROFILES[n_rows]["span"]
    return sorted(set(list(range(14)) + [span - 1, span, span + 1, 2 * span + 1, 63, 64, 65]))


def lengths(n_rows):
    """In-range rows of every length of row_lengths(); noisy, so rows that have stencils hold
    candidates and non-candidates.  64 rows: rows 3, 4, 59 and 60 (outside rowIndexStart /
    rowIndexEnd) hold flat 40-point runs that a row skip off by one would select.  16 rows have
    fewer rows than lengths: two clouds."""
    rng = np.random.default_rng(100 + n_rows)
    L = row_lengths(n_rows)
    rows_in = list(in_range(n_rows))
    out = []
    n_clouds = -(-len(L) // len(rows_in))
    for c in range(n_clouds):
        rows = []
        for r in range(n_rows):
            if r in rows_in:
                # shifted so that the first and the last in-range row are not empty
                n = L[(rows_in.index(r) + 5 + c * len(rows_in)) % len(L)]
                if c and r in (rows_in[0], rows_in[-1]) and n == 0:
                    n = 65
                rows.append((r, noisy_row(rng, n_rows, r, n)))
            elif r in (3, 4, 59, 60):
                rows.append((r, flat_row(n_rows, r, 40)))
            else:
                rows.append((r, noisy_row(rng, n_rows, r, 7)))
        out.append(_case(f"lengths{'_abc'[c + 1] if n_clouds > 1 else ''}", n_rows, rows))
    have = set()
    for cs in out:
        have |= {int(np.count_nonzero(cs.run == r)) for r in rows_in}
    assert have >= set(L), sorted(set(L) - have)
    return out


# ------------------------------------------------------------------------------- threshold
def threshold_targets(n_rows):
    t = F32(ref.PROFILES[n_rows]["plane_min"])
    return {"below": np.nextafter(t, F32(0)), "equal": t, "above": np.nextafter(t, F32(1))}


def centre_index(n_rows):
    """the first multiple of the span with a full stencil: the greedy rule tests exactly the
    multiples of the span while all of them are candidates"""
    span = ref.PROFILES[n_rows]["span"]
    return span * -(-5 // span)


def _search_centre(P, target, t):
    """centre point C = P + (a, y, 0) whose curvature among ten copies of P is exactly `target`:
    a slightly short of sqrt(planeMin) / 10, y scanned float by float (one step of y moves the
    exact value by far less than a float of planeMin, so every float near it is met)"""
    a = np.sqrt(0.9 * float(t)) / 10.0
    cx = F32(P[0] + F32(a))
    u = lambda p, c, k: [np.full(k, p, F32)] * 5 + [c] + [np.full(k, p, F32)] * 5     # noqa: E731
    dx = ref.stencil(u(P[0], np.full(1, cx, F32), 1))
    dz = ref.stencil(u(P[2], np.full(1, P[2], F32), 1))
    left = float(t) - float(dx[0]) ** 2 - float(dz[0]) ** 2
    if left <= 0:
        return None
    y0 = F32(P[1] + F32(np.sqrt(left) / 10.0))
    K = 20000
    ys = (np.int32(y0.view(np.int32)) + np.arange(-K, K + 1, dtype=np.int32)).view(F32)
    dy = ref.stencil(u(P[1], ys, ys.size))
    v = ref.value(np.full(ys.size, dx[0], F32), dy, np.full(ys.size, dz[0], F32))
    hit = np.nonzero(v.view(np.uint32) == target.view(np.uint32))[0]
    if hit.size == 0:
        return None
    return np.array([cx, ys[hit[0]], P[2]], F32)


def threshold(n_rows):
    """Every row the same length: ten coincident neighbours P around a centre at index
    centre_index(); in the in-range rows the centre is displaced so that its curvature is the
    float just below planeMin, planeMin itself or the float just above, in turn.  Every other
    point of a row is a candidate (value 0 or |C - P|^2), so the greedy rule tests the centre:
    taken, the next pick is one span on; not taken, every later pick of the row moves by one."""
    tg = threshold_targets(n_rows)
    t = tg["equal"]
    c = centre_index(n_rows)
    n = c + 1 + 2 * ref.PROFILES[n_rows]["span"] + 5
    rows, kinds = [], {}
    order = ["below", "equal", "above"]
    for r in range(n_rows):
        P = polar(n_rows, r, [0.0], RANGE_M)[0]
        p = np.tile(P, (n, 1))
        if r in in_range(n_rows):
            kind = order[len(kinds) % 3]
            C = _search_centre(P, tg[kind], t)
            if C is not None:
                p[c] = C
                kinds[r] = kind
        rows.append((r, p))
    cs = _case("threshold", n_rows, rows, equal_rows=True)
    y = ref.extract_planes(cs.pts, n_rows)
    got = {k: 0 for k in tg}
    for r, kind in kinds.items():
        assert y["cv"][y["off"][r] + c].view(np.uint32) == tg[kind].view(np.uint32), (r, kind)
        got[kind] += 1
    assert all(got.values()), f"threshold values not all found for {n_rows} rows: {got}"
    return [cs], kinds


# ------------------------------------------------------------------------------- dense
DENSE_ROWS = {64: {4: 300, 5: 300, 10: 300, 18: 300, 20: 2049, 30: 4097, 53: 300, 58: 300, 59: 300},
              16: {0: 300, 2: 300, 7: 2049, 12: 4097, 15: 300}}


def candidate_share(case):
    y = ref.extract_planes(case.pts, case.n_rows)
    pm = F32(ref.PROFILES[case.n_rows]["plane_min"])
    a, b = y["off"][in_range(case.n_rows)[0]], y["off"][in_range(case.n_rows)[-1] + 1]
    return float(np.mean(y["cv"][a:b] < pm))


def dense(n_rows):
    """Rows of 300, 2049 and 4097 noisy points (a row across the 2048-point chunk edge once and
    twice), 40-70 % of them candidates, so the greedy rule meets irregular candidate bits at
    every word and chunk edge; the rows next to rowIndexStart / rowIndexEnd on both sides are
    among them.  dense_equal: every row 300 points, so the interleaved order is a regular scan."""
    rng = np.random.default_rng(200 + n_rows)
    a = _case("dense", n_rows, [(r, noisy_row(rng, n_rows, r, n)) for r, n in sorted(DENSE_ROWS[n_rows].items())])
    b = _case("dense_equal", n_rows, [(r, noisy_row(rng, n_rows, r, 300, az0=0.1)) for r in range(n_rows)],
              equal_rows=True)
    for cs in (a, b):
        s = candidate_share(cs)
        assert 0.40 <= s <= 0.70, (cs.name, n_rows, s)
    return [a, b]


# ------------------------------------------------------------------------------- nonfinite
def nonfinite(n_rows):
    """The row of angle 0 holds 90 noisy points and, placed by hand: a lone +inf x at index 20
    (infinite curvature across its 11 taps), +inf and -inf x at 40 and 43 (NaN where a stencil
    holds both), an x whose square overflows float at 62 and a +inf y at 80 -- sqrt(inf) makes
    their angle 0, so they are kept, in this row.  Points that are dropped sit inside the runs:
    NaN coordinates, the origin, x = y = 0, an infinite z, inf / inf.  Four more rows hold 30
    points each."""
    rng = np.random.default_rng(300 + n_rows)
    zr = ZERO_ROW[n_rows]
    inf, nan = np.inf, np.nan
    row = noisy_row(rng, n_rows, zr, 90)
    for i, p in [(20, (inf, 1.0, 0.5)), (40, (inf, -2.0, 0.0)), (43, (-inf, 3.0, 1.0)), (62, (3e19, 0.0, 1.0)),
                 (80, (2.0, inf, -1.0))]:
        row[i] = p
    dropped = np.array([(nan, 1, 1), (1, nan, 1), (1, 1, nan), (nan, nan, nan), (0, 0, 0), (0, 0, 2.5), (0, 0, -1),
                        (1, 2, inf), (1, 2, -inf), (inf, 0, inf)], F32)
    rows = []
    others = [zr - 1, zr + 1, in_range(n_rows)[0], in_range(n_rows)[-1]]
    for r in sorted(set(others + [zr])):
        p = row if r == zr else noisy_row(rng, n_rows, r, 30)
        at = np.sort(rng.integers(1, len(p), len(dropped)))
        rows.append((r, np.insert(p, at, dropped, axis=0)))
    cs = _case("nonfinite", n_rows, rows)
    y = ref.extract_planes(cs.pts, n_rows)
    a, b = y["off"][zr], y["off"][zr + 1]
    assert zr in in_range(n_rows) and b - a == 90
    assert np.isnan(y["cv"][a:b]).any() and np.isinf(y["cv"][a:b]).any()
    return [cs]


FAMILIES = ("lengths", "threshold", "dense", "nonfinite")


@functools.lru_cache(maxsize=None)
def cases(n_rows):
    """every feature case of a profile, in a fixed order"""
    out = lengths(n_rows) + threshold(n_rows)[0] + dense(n_rows) + nonfinite(n_rows)
    for cs in out:
        cs.pts.setflags(write=False)
        cs.run.setflags(write=False)
    return tuple(out)


# ------------------------------------------------------------------------------- edge rows
# Row cases of the project's edge selection (tests/edge_cases.py runs them after cases(); they
# are not part of cases(), whose plane tests they would only lengthen).
LONG_ROW = {64: 31, 16: 9}
LONG_ROW_POINTS = 4200                           # more than 4097: a row over three 2048-point chunks
EDGE_MIN_ROW = {64: 20, 16: 7}                   # the 2049-point row of "dense"


@functools.lru_cache(maxsize=None)
def edge_rows(n_rows):
    """long_row: one in-range row of 4200 noisy points (at edge_span 1 every candidate word of
    it is walked bit by bit) between two short rows.  flat: smooth arcs only -- no curvature
    exceeds any edge_min the tests use, the frame's edge list is empty."""
    rng = np.random.default_rng(500 + n_rows)
    r = LONG_ROW[n_rows]
    a = _case("long_row", n_rows, [(r - 1, noisy_row(rng, n_rows, r - 1, 70)),
                                   (r, noisy_row(rng, n_rows, r, LONG_ROW_POINTS, az0=0.2)),
                                   (r + 1, noisy_row(rng, n_rows, r + 1, 33))])
    b = _case("flat", n_rows, [(q, flat_row(n_rows, q, 90)) for q in range(n_rows)], equal_rows=True)
    for cs in (a, b):
        cs.pts.setflags(write=False)
        cs.run.setflags(write=False)
    return (a, b)


# ------------------------------------------------------------------------------- layouts
LAYOUTS =("rowmajor", "descending", "interleaved", "shuffled", "masked", "stride4")


def _pos_in_run(run):
    first = np.concatenate([[0], np.nonzero(np.diff(run))[0] + 1])
    start = np.repeat(first, np.diff(np.concatenate([first, [run.size]])))
    return np.arange(run.size) - start


def layout(case, which):
    """-> (pts [n, stride] float32, keep [n] uint8 or None).  The cloud the stage sees is
    pts[keep != 0][:, :3].

    rowmajor     runs of rows ascending, one run per row in a chunk: k_feat_wave_run.
    descending   runs of rows descending: k_feat_wave_run moves its bit planes run by run, so own
                 slots are not in input order.
    interleaved  the k-th point of every row, row after row (a spinning sensor's order).  With
                 equal row lengths and 64 rows these are the regular windows of k_feat_wave_reg;
                 ragged rows break the columns, and the flagged chunks go to k_feat_chunk.
    shuffled     no order at all: almost every stencil is left open by the chunk kernels and
                 resolved by k_feat_select through the chunk-major index.
    masked       the same cloud inside a superset, keep = 0 on the rest: the masked entry point
                 (no k_feat_wave_reg; every masked point is a gap in a run).
    stride4      the padded PCL point layout: x, y, z and a fourth float the stage must skip.
    """
    rng = np.random.default_rng(sum(map(ord, case.name + which)) + case.n_rows)
    pts, run = case.pts, case.run
    keep = None
    if which == "rowmajor":
        out = pts
    elif which == "descending":
        out = pts[np.argsort(-run, kind="stable")]
    elif which == "interleaved":
        out = pts[np.lexsort((run, _pos_in_run(run)))]
    elif which == "shuffled":
        out = pts[rng.permutation(len(pts))]
    elif which == "masked":
        n, extra = len(pts), max(8, len(pts) // 3)
        fin = pts[np.isfinite(pts).all(1)]
        decoy = fin[rng.integers(0, len(fin), extra)] * rng.uniform(0.5, 1.5, (extra, 1)).astype(F32)
        decoy[:, 2] += rng.normal(0, 1.0, extra).astype(F32)
        at = np.sort(rng.integers(0, n + 1, extra))
        out = np.insert(pts, at, decoy, axis=0)
        keep = np.ones(n + extra, np.uint8)
        keep[at + np.arange(extra)] = 0
        assert np.array_equal(out[keep != 0].view(np.uint32), pts.view(np.uint32))
    elif which == "stride4":
        out = np.full((len(pts), 4), 7.0, F32)
        out[:, :3] = pts
    else:
        raise ValueError(which)
    return np.ascontiguousarray(out, F32), keep


def binned(case, pieces=8):
    """The cloud cut into `pieces` runs with blocks of NaN points between them, more than
    BINNED_POINTS in all: a launch with such a frame takes the binned stage (k_bin_count /
    k_bin_scan / k_bin_curv / k_select, feat_bin.hip) for every frame.  NaN points are dropped,
    so the yardstick's work does not grow."""
    cut = np.linspace(0, len(case.pts), pieces + 1).astype(int)
    pad = -(-(BINNED_POINTS + 1 - len(case.pts)) // (pieces - 1)) + 3
    parts = []
    for k in range(pieces):
        parts.append(case.pts[cut[k]:cut[k + 1]])
        if k < pieces - 1:
            parts.append(np.full((pad, 3), np.nan, F32))
    out = np.concatenate(parts)
    assert len(out) > BINNED_POINTS
    return out


# ------------------------------------------------------------------------------- voxel grid
VOXEL_LEAVES = (0.1, 0.4)
VOXEL_BATCH_SIZES = (1, 2, 3, 4, 5, 8, 9)


@functools.lru_cache(maxsize=None)
def voxel_clouds():
    """name -> [n, 4] float32"""
    rng = np.random.default_rng(400)
    w = lambda xyz: np.concatenate([xyz, rng.uniform(0, 64, (len(xyz), 1))], 1).astype(F32)   # noqa: E731
    g = np.stack(np.meshgrid(np.arange(-8, 9), np.arange(-4, 5), np.arange(-2, 3), indexing="ij"), -1)
    lattice = np.concatenate([g.reshape(-1, 3) * 0.1, rng.uniform(-1, 1, (500, 3))])
    lattice = lattice[rng.permutation(len(lattice))]
    dup = np.repeat(rng.uniform(-2, 2, (50, 3)), 3, axis=0)
    c = {
        # multiples of 0.1 from -0.8 to 0.8 (as floats: on, just below and just above the voxel
        # boundaries of both leaves, on both sides of zero) plus random points
        "lattice": w(lattice),
        "one_point": np.array([[-0.35, 0.2, 7.0, 3.0]], F32),
        # one voxel at both leaves; its run spans three 256-thread blocks of k_vg_heads / reduce
        "one_voxel_700": w(rng.uniform(0.41, 0.49, (700, 3))),
        "duplicates": w(dup[rng.permutation(len(dup))]),
        "empty": np.zeros((0, 4), F32),
        # a cloud that ends in voxel index 0 followed by one that starts in voxel index 0: only
        # the cloud bits of the sort key separate the two runs
        "adjacent_a": w(rng.uniform(-0.29, -0.21, (5, 3))),
        "adjacent_b": w(np.concatenate([[[0.01, 0.01, 0.01]], rng.uniform(0, 3, (300, 3))])),
        "negative": w(rng.uniform(-5, -1, (400, 3))),
        "wide": w(rng.uniform(-20, 20, (2000, 3))),
    }
    for v in c.values():
        v.setflags(write=False)
    return c


PASSTHROUGH = np.array([[0, 0, 0, 1], [1000, 1000, 1000, 2], [3, 4, 5, 3]], F32)


VOXEL_BATCHES = {
    1: ["one_point"],
    2: ["adjacent_a", "adjacent_b"],
    3: ["one_voxel_700", "empty", "lattice"],
    4: ["empty", "duplicates", "negative", "empty"],
    5: ["lattice", "adjacent_a", "adjacent_b", "one_point", "wide"],
    8: ["wide", "empty", "one_point", "one_voxel_700", "adjacent_a", "adjacent_b", "lattice", "duplicates"],
    9: ["lattice", "adjacent_a", "adjacent_b", "empty", "one_point", "one_voxel_700", "duplicates", "negative",
        "wide"],
}
assert tuple(VOXEL_BATCHES) == VOXEL_BATCH_SIZES and all(len(v) == k for k, v in VOXEL_BATCHES.items())

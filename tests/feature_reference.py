"""Independent yardstick for the feature stage and the voxel grid: numpy only.

Written from the reference's src/frameFeature.cpp:45-123 (ring binning, curvature, greedy planar
selection) and from DESIGN.md's statement of PCL 1.10 pcl::VoxelGrid -- not from oracle/ and not
from the kernels, and it imports nothing of either.  The source evaluates float expressions in a
written order; a numpy float32 element-wise operation rounds once, as each C operation does, so a
row is evaluated with shifted float32 arrays and the results are comparable bit for bit.

The project's own edge selection (select_edges, extract_features) has no reference source: it is
written from the definition in the header comment of oracle/edge_oracle.c, and reuses this
file's ring ids, binning and curvature.

Every rule is also reachable as a deliberately WRONG variant through a keyword (VARIANTS at the
end).  They exist for one purpose: tests/test_feature_host.py (tests/test_edge_host.py for the
edge rules) shows that for each of them some case of tests/feature_cases.py changes its output,
so the cases do reach the rule.
"""
import numpy as np

F32 = np.float32
INT32_MAX = 2 ** 31 - 1

# main() of frameFeature.cpp:141-152: planeMin, planeSpan, rowIndexStart, rowIndexEnd
PROFILES = {16: dict(plane_min=0.05, span=3, row_start=0, row_end=0),
            64: dict(plane_min=0.005, span=25, row_start=5, row_end=5)}


def _profile(n_rows):
    if n_rows not in PROFILES:
        raise ValueError("N_SCAN_ROW is 16 or 64")
    return PROFILES[n_rows]


# ------------------------------------------------------------------------------- :57-73
def ring_ids(pts, n_rows):
    """scanID of every point (-1: dropped) and margin_deg, the distance of its angle to the
    nearest value at which int() steps (or to the -8.83 switch); NaN for a NaN angle.
    x*x + y*y is formed in float32 as the source does (inf above |x| ~ 1.8e19: the angle is then
    0); the rest in float64.  The margin says how far a point is from the only places where the
    precision of atan / sqrt could matter; tests/test_ring_table.py owns those."""
    _profile(n_rows)
    p = np.asarray(pts, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        s = x * x + y * y                                                 # float32, :57
        angle = np.arctan(z.astype(np.float64) / np.sqrt(s.astype(np.float64))) * 180 / np.pi
        ids = np.full(p.shape[0], -1, np.int64)
        if n_rows == 16:
            ok = (angle >= -15) | (angle <= 15)                            # true unless NaN
            f = (angle + 15) / 2 + 0.5
            scale = np.full(p.shape[0], 0.5)
            switch = np.full(p.shape[0], np.inf)
        else:
            ok = (angle >= -24.33) | (angle <= 2)                          # true unless NaN
            up = angle >= -8.83
            f = np.where(up, (2 - angle) * 3.0 + 0.5, (-8.83 - angle) * 2.0 + 0.5)
            scale = np.where(up, 3.0, 2.0)
            switch = np.abs(angle + 8.83)
        t = np.trunc(np.where(ok, f, 0.0)).astype(np.int64)               # int(): toward zero
        if n_rows == 64:
            t = np.where(up, t, n_rows // 2 + t)
        ids = np.where(ok, t, -1)
        ids = np.where((ids > -1) & (ids < n_rows), ids, -1)
        margin = np.minimum(np.abs(f - np.round(f)) / scale, switch)
    return ids.astype(np.int64), np.where(ok, margin, np.nan)


# ------------------------------------------------------------------------------- :73-80
def bin_rows(pts, ids, n_rows, intensity_f32=False, unstable=False):
    """v_scan_row as one ring-ordered [kept, 4] float32 cloud and its row offsets [n_rows + 1]:
    a stable partition in arrival order, intensity = float(indexInRow + row / 100.0) with the sum
    formed in double (:77).  -> (rx, off, src) with src the input index of every kept point."""
    p = np.asarray(pts, F32)
    ids = np.asarray(ids, np.int64)
    kept = np.nonzero(ids >= 0)[0]
    src = kept[np.argsort(ids[kept], kind="stable")]
    off = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(ids[kept], minlength=n_rows), out=off[1:])
    if unstable:                        # WRONG: arrival order within a row not kept (reversed)
        src = np.concatenate([src[off[r]:off[r + 1]][::-1] for r in range(n_rows)] + [src[:0]])
    row = ids[src]
    idx = np.arange(src.size, dtype=np.int64) - off[row]
    rx = np.zeros((src.size, 4), F32)
    rx[:, :3] = p[src, :3]
    if intensity_f32:                   # WRONG: float(indexInRow) + float(row / 100.0)
        rx[:, 3] = idx.astype(F32) + (row / 100.0).astype(F32)
    else:
        rx[:, 3] = (idx.astype(np.float64) + row / 100.0).astype(F32)
    return rx, off, src


# ------------------------------------------------------------------------------- :84-107
def stencil(u):
    """((((u0+u1)+u2)+u3)+u4) - 10*u5, then + u6 ... + u10 left to right; u: 11 float32 arrays"""
    with np.errstate(all="ignore"):
        a = u[0] + u[1]
        a = a + u[2]
        a = a + u[3]
        a = a + u[4]
        a = a - F32(10) * u[5]
        for k in range(6, 11):
            a = a + u[k]
    return a


def value(dx, dy, dz):
    """:105  diffX * diffX + diffY * diffY + diffZ * diffZ"""
    with np.errstate(all="ignore"):
        return (dx * dx + dy * dy) + dz * dz


def _row_range(n_rows, row_lo, row_hi):
    pr = _profile(n_rows)
    return max(0, pr["row_start"] + row_lo), min(n_rows, n_rows - pr["row_end"] + row_hi)


def curvature(rx, off, n_rows, row_lo=0, row_hi=0, edge=5):
    """value of every ring-ordered point: rows rowIndexStart <= r < N - rowIndexEnd, j in
    [5, size - 5); 0 everywhere else (:75).
    WRONG variants: row_lo / row_hi shift the row range's ends, edge = 4 or 6 computes j in
    [edge, size - edge) (with edge 4 the outermost taps fall into the neighbouring rows of the
    ring-ordered cloud, as an unguarded flat array would have it)."""
    rx = np.asarray(rx, F32)
    n = rx.shape[0]
    cv = np.zeros(n, F32)
    r0, r1 = _row_range(n_rows, row_lo, row_hi)
    for r in range(r0, r1):
        a, b = int(off[r]), int(off[r + 1])
        lo, hi = a + edge, b - edge
        if hi <= lo:
            continue
        j = np.arange(lo, hi)
        d = [stencil([rx[np.clip(j + k, 0, n - 1), c] for k in range(-5, 6)]) for c in range(3)]
        cv[lo:hi] = value(*d)
    return cv


# ------------------------------------------------------------------------------- :110-123
def select(rx, cv, off, n_rows, row_lo=0, row_hi=0, span_delta=0, le=False):
    """the greedy jstart rule: a point is taken when j >= jstart and value < float(planeMin), and
    jstart = j + planeSpan.  -> (plane list [m, 4], ring positions [m]).
    WRONG variants: span_delta, le (<= for <), row_lo / row_hi."""
    pr = _profile(n_rows)
    rx = np.asarray(rx, F32)
    pm, span = F32(pr["plane_min"]), pr["span"] + span_delta
    r0, r1 = _row_range(n_rows, row_lo, row_hi)
    sel = []
    for r in range(r0, r1):
        a, b = int(off[r]), int(off[r + 1])
        v = cv[a:b]
        with np.errstate(invalid="ignore"):
            cand = np.nonzero((v <= pm) if le else (v < pm))[0]          # NaN: never
        jstart = 0
        for j in cand.tolist():
            if j >= jstart:
                sel.append(a + j)
                jstart = j + span
    sel = np.array(sel, np.int64)
    return rx[sel], sel


def extract_planes(pts, n_rows, **wrong):
    """cloudHandler up to framePlanePtr -> dict(ids, margin, rx, off, src, cv, planes, sel)."""
    kw = lambda *names: {k: wrong[k] for k in names if k in wrong}      # noqa: E731
    unknown = set(wrong) - {"intensity_f32", "unstable", "row_lo", "row_hi", "edge", "span_delta", "le"}
    if unknown:
        raise TypeError(f"unknown variant keyword {sorted(unknown)}")
    ids, margin = ring_ids(pts, n_rows)
    rx, off, src = bin_rows(pts, ids, n_rows, **kw("intensity_f32", "unstable"))
    cv = curvature(rx, off, n_rows, **kw("row_lo", "row_hi", "edge"))
    planes, sel = select(rx, cv, off, n_rows, **kw("row_lo", "row_hi", "span_delta", "le"))
    return dict(ids=ids, margin=margin, rx=rx, off=off, src=src, cv=cv, planes=planes, sel=sel)


# ------------------------------------------------------------------------------- edges
# The project's own edge selection (the reference has none), from the definition in the header
# comment of oracle/edge_oracle.c -- not from its functions and not from the kernels: per row in
# [rowStart, N - rowEnd), greedy in index order, a point is emitted when j >= jstart and
# curvature > edge_min, and then jstart = j + edge_span.  The comparison is strict and in
# float32 (inf passes, NaN does not); the walk has its own jstart, apart from the plane walk's.
def select_edges(rx, cv, off, n_rows, edge_min, edge_span, row_lo=0, row_hi=0, span_delta=0, ge=False,
                 shared_jstart=False):
    """-> (edge list [m, 4], ring positions [m]).
    WRONG variants: ge (>= for >), span_delta, row_lo / row_hi, shared_jstart (ONE jstart for
    the plane walk and the edge walk of a row: either kind of pick pushes it on by its own span)."""
    pr = _profile(n_rows)
    rx = np.asarray(rx, F32)
    cv = np.asarray(cv, F32)
    em, span = F32(edge_min), int(edge_span) + span_delta
    pm, pspan = F32(pr["plane_min"]), pr["span"]
    r0, r1 = _row_range(n_rows, row_lo, row_hi)
    sel = []
    for r in range(r0, r1):
        a, b = int(off[r]), int(off[r + 1])
        v = cv[a:b]
        with np.errstate(invalid="ignore"):
            is_edge = (v >= em) if ge else (v > em)                      # NaN: never
            is_plane = v < pm
        jstart = 0
        if shared_jstart:
            for j in np.nonzero(is_edge | is_plane)[0].tolist():
                if j >= jstart:
                    if is_plane[j]:
                        jstart = j + pspan
                    else:
                        sel.append(a + j)
                        jstart = j + span
            continue
        for j in np.nonzero(is_edge)[0].tolist():
            if j >= jstart:
                sel.append(a + j)
                jstart = j + span
    sel = np.array(sel, np.int64)
    return rx[sel], sel


EDGE_SELECT_KEYS = ("row_lo", "row_hi", "span_delta", "ge", "shared_jstart")


def extract_features(pts, n_rows, edge_min, edge_span, **wrong):
    """extract_planes() plus the edge list: -> its dict with edges [m, 4] and esel [m] added.
    Keywords are select_edges' wrong variants; the planes are always the right ones.  A wrong
    row range is the curvature's too (outside the right one every value is 0 and nothing could
    be selected): the edge walk then sees the curvature of the rows it wrongly includes."""
    unknown = set(wrong) - set(EDGE_SELECT_KEYS)
    if unknown:
        raise TypeError(f"unknown variant keyword {sorted(unknown)}")
    y = dict(extract_planes(pts, n_rows))
    rows = {k: wrong[k] for k in ("row_lo", "row_hi") if k in wrong}
    cv = curvature(y["rx"], y["off"], n_rows, **rows) if rows else y["cv"]
    y["edges"], y["esel"] = select_edges(y["rx"], cv, y["off"], n_rows, edge_min, edge_span, **wrong)
    return y


# ------------------------------------------------------------------------------- VoxelGrid
def voxel_passthrough(xyzi, leaf):
    """PCL's overflow guard: (int64((max - min) * inv) + 1) over the three axes > INT32_MAX"""
    x = np.asarray(xyzi, F32).reshape(-1, 4)
    if x.shape[0] == 0:
        return False
    inv = F32(1) / F32(leaf)
    with np.errstate(all="ignore"):
        d = ((x[:, :3].max(0) - x[:, :3].min(0)) * inv).astype(np.int64) + 1
    return int(d[0]) * int(d[1]) * int(d[2]) > INT32_MAX


def voxel_grid(xyzi, leaf, truncate=False, sorted_sums=False):
    """pcl::VoxelGrid<PointXYZI>::filter (all fields averaged) in float32: [n, 4] -> [m, 4].
    inv = 1 / leaf; bounds floor(min * inv), floor(max * inv); div = max - min + 1; a point's
    index i + j * div0 + k * div0 * div1; voxels in ascending index, each the float32 sum of its
    points in input order from zero, divided by the float32 count.
    WRONG variants: truncate (int() for floor), sorted_sums (a voxel's points summed in sorted
    coordinate order)."""
    x = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    n = x.shape[0]
    if n == 0 or voxel_passthrough(x, leaf):
        return x.copy()
    inv = F32(1) / F32(leaf)
    rnd = np.trunc if truncate else np.floor
    minb = rnd(x[:, :3].min(0) * inv).astype(np.int64)
    maxb = rnd(x[:, :3].max(0) * inv).astype(np.int64)
    div = maxb - minb + 1
    ijk = rnd(x[:, :3] * inv).astype(np.int64) - minb
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    if sorted_sums:
        order = np.lexsort((x[:, 3], x[:, 2], x[:, 1], x[:, 0], idx))
    else:
        order = np.argsort(idx, kind="stable")
    key = idx[order]
    head = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
    cnt = np.diff(np.concatenate([head, [n]]))
    acc = np.zeros((head.size, 4), F32)
    for k in range(int(cnt.max())):                 # the k-th point of every voxel that has one
        m = cnt > k
        acc[m] = acc[m] + x[order[head[m] + k]]
    return acc / cnt.astype(F32)[:, None]


# ------------------------------------------------------------------------------- the wrong rules
FEATURE_VARIANTS = {
    "span+1": dict(span_delta=1), "span-1": dict(span_delta=-1), "<= for <": dict(le=True),
    "row range starts one early": dict(row_lo=-1), "row range starts one late": dict(row_lo=1),
    "row range ends one early": dict(row_hi=-1), "row range ends one late": dict(row_hi=1),
    "stencil range [4, size-4)": dict(edge=4), "stencil range [6, size-6)": dict(edge=6),
    "intensity summed in float32": dict(intensity_f32=True),
    "unstable partition": dict(unstable=True),
}
EDGE_VARIANTS = {
    ">= for >": dict(ge=True), "jstart = j + span + 1": dict(span_delta=1), "jstart = j + span - 1": dict(span_delta=-1),
    "one jstart shared with the plane walk": dict(shared_jstart=True),
    "row range starts one early": dict(row_lo=-1), "row range starts one late": dict(row_lo=1),
    "row range ends one early": dict(row_hi=-1), "row range ends one late": dict(row_hi=1),
}
VOXEL_VARIANTS = {"truncation for floor": dict(truncate=True),
                  "sums in sorted-coordinate order": dict(sorted_sums=True)}

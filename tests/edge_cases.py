"""Seeded cases of the edge path's first half -- edge selection and the line table -- shared by
tests/test_edge_host.py (the CPU oracle against the yardstick) and
tests/test_gpu_edge_yardstick.py (the device against it).  The yardsticks are
tests/feature_reference.py (select_edges) and tests/edge_reference.py (line_table).

Selection runs reuse the feature cases (tests/feature_cases.py: cases() and edge_rows()) in every
input order; what is new is the run-time pair (edge_min, edge_span).

Line-table cases are hand-made edge clouds: no selection is needed to reach a rule.  Points with
NaN coordinates are out of scope: (d2, index) order is undefined for them.
"""
import functools
from dataclasses import dataclass

import numpy as np

import edge_reference as er
import feature_cases as fc
import feature_reference as ref

F32 = np.float32

# ------------------------------------------------------------------------------- selection
# one candidate word is 64 points: spans below, at and above it, and beyond one word
SPANS = (1, 3, 10, 63, 64, 65, 200)


def base_edge_min(n_rows):
    """planeMin as edge_min: the noisy rows of the feature cases hold 30-60 % edge candidates, and
    every point is a candidate of one of the two walks, so a shared jstart cannot hide"""
    return F32(ref.PROFILES[n_rows]["plane_min"])


def selection_cases(n_rows):
    return fc.cases(n_rows) + fc.edge_rows(n_rows)


@functools.lru_cache(maxsize=None)
def edge_min_targets(n_rows):
    """edge_min is a run-time parameter: the curvature of one point of the named row (the
    2049-point row of "dense", its point of median curvature among those above planeMin), read
    from the yardstick's curvature, and the float32 below and above it.
    -> (row, index in row, dict(below, equal, above))."""
    dense = next(c for c in fc.cases(n_rows) if c.name == "dense")
    y = ref.extract_planes(dense.pts, n_rows)
    r = fc.EDGE_MIN_ROW[n_rows]
    a, b = int(y["off"][r]), int(y["off"][r + 1])
    v = y["cv"][a:b]
    cand = np.nonzero(np.isfinite(v) & (v > base_edge_min(n_rows)))[0]
    j = int(cand[np.argsort(v[cand], kind="stable")[len(cand) // 2]])
    t = F32(v[j])
    assert np.count_nonzero(v == t) == 1                 # the value names one point of the row
    return r, j, {"below": np.nextafter(t, F32(0)), "equal": t, "above": np.nextafter(t, F32(np.inf))}


def selection_runs(n_rows):
    """[(tag, edge_min, edge_span)]: every span at the base edge_min, then edge_min at, below and
    above one curvature value with span 1 (no jstart ever blocks: the comparison alone decides)"""
    runs = [(f"span{s}", base_edge_min(n_rows), s) for s in SPANS]
    runs += [(f"edge_min_{k}", t, 1) for k, t in edge_min_targets(n_rows)[2].items()]
    return runs


# ------------------------------------------------------------------------------- line table
DEFAULT_D2, DEFAULT_RATIO = 1.0, 3.0
SIZES = (0, 1, 4, 5, 6, 1023, 1024, 1025, 8192, 8193)       # m < 5, m == 5, the 1024-thread stride, the LDS cap


def _xyzi(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    k = np.arange(len(xyz))
    return np.c_[xyz, k + (k % 64) / 100.0].astype(F32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _line(rng, p0, d, n, step=0.1, noise=0.005):
    return np.asarray(p0, np.float64) + np.outer(step * np.arange(n), _unit(d)) + rng.normal(0, noise, (n, 3))


def noisy_cloud(seed, m):
    """m edge points: noisy 32-point lines along random directions in a 60 m box, one in eight
    points an isotropic stray, in a shuffled order"""
    rng = np.random.default_rng(seed)
    parts, left = [], m
    while left > 0:
        n = min(left, 32)
        parts.append(_line(rng, rng.uniform(-30, 30, 3), rng.normal(size=3), n))
        left -= n
    xyz = np.concatenate(parts) if parts else np.zeros((0, 3))
    stray = rng.random(m) < 0.125
    xyz[stray] += rng.normal(0, 0.15, (int(stray.sum()), 3))
    return _xyzi(xyz[rng.permutation(m)])


@functools.lru_cache(maxsize=None)
def size_frames():
    return {m: noisy_cloud(600 + m, m) for m in SIZES}


@functools.lru_cache(maxsize=None)
def noisy_frames():
    """name -> [m, 4] float32, seeded noisy geometry"""
    rng = np.random.default_rng(700)
    blobs = lambda n, s: np.concatenate([c + rng.normal(0, 1.0, (8, 3)) * s                     # noqa: E731
                                         for c in rng.uniform(-20, 20, (n, 3))])
    rnd = np.concatenate([_line(rng, rng.uniform(-20, 20, 3), rng.normal(size=3), 30) for _ in range(10)])
    far = np.concatenate([_line(rng, np.array([3000.0, -4000.0, 20.0]) + rng.uniform(-10, 10, 3), rng.normal(size=3), 30)
                          for _ in range(6)])
    par = np.concatenate([_line(rng, [0, 0, 0], [1, 0.5, 0.2], 40, noise=0.002),
                          _line(rng, np.cross(_unit([1, 0.5, 0.2]), [0, 0, 1.0]) * 0.02 / np.linalg.norm(
                              np.cross(_unit([1, 0.5, 0.2]), [0, 0, 1.0])), [1, 0.5, 0.2], 40, noise=0.002)])
    out = {
        "axes": np.concatenate([_line(rng, [5, 0, 0], [1, 0, 0], 40), _line(rng, [0, 25, 0], [0, 1, 0], 40),
                                _line(rng, [0, 0, 45], [0, 0, 1], 40)]),
        # |u0| = |u1| (= |u2|) up to the noise: the sign rule's largest component is a toss-up
        "diagonals": np.concatenate([_line(rng, [0, 0, 0], [1, -1, 0], 40, noise=0.001),
                                     _line(rng, [50, 0, 0], [1, 1, 1], 40, noise=0.001)]),
        "random_lines": rnd,
        "planar_blobs": blobs(20, np.array([0.15, 0.15, 0.002])),
        "isotropic_blobs": blobs(20, np.array([0.1, 0.1, 0.1])),
        "parallel_2cm": par,
        "far_5km": far,
    }
    return {k: _xyzi(v) for k, v in out.items()}


# Hand-made geometry on integer / 4 coordinates: every float32 d2 and every float64 sum is exact.
# Clusters stand 64 m apart along y, so a point's five nearest are in its own cluster.
def _clusters(cl):
    return _xyzi(np.concatenate([np.asarray(c, np.float64) * 0.25 + [0.0, 64.0 * k, 0.0] for k, c in enumerate(cl)]))


def _on_x(xs):
    return [[x, 0, 0] for x in xs]


GATE_D2 = 1.0                                       # d2[4] of the gate cluster's end points: (4 * 0.25)^2
EXACT_DIAG_CLUSTERS = (
    "tie_low", "tie_reversed", "tie_after", "tie_before", "five_copies", "collinear", "ratio4_at", "ratio4_above", "ratio3_rounding",
    "gate")


@functools.lru_cache(maxsize=None)
def exact_frames():
    """exact_diag: every covariance is diagonal or zero, so its eigenvalues are its diagonal in
    any eigensolver and every rule is asserted without a margin.  Its clusters, in order:
      tie_low / tie_reversed / tie_after / tie_before   x = -3, -2, -1, 0, 1, 3 (quarter metres):
                    for the point at 0 the 5th neighbour is a tie between -3 and +3 (d2 = 9/16),
                    and the centroid says which was taken.  The lower index wins: -3 below the
                    query's index against +3 above it, +3 below against -3 above, +3 before -3
                    with both above the query, and +3 before -3 with both below it.
      five_copies   five copies of one point: A = 0.
      collinear     six points of one axis-parallel line: lambda2 = 0.
      ratio4_at     (+-a, 0, 0), (0, +-b, 0), the centre, a = 2 b: lambda1 = 4 lambda2 exactly;
                    with line_ratio = 4 the strict > decides (invalid).
      ratio4_above  a one lattice step larger: valid.
      ratio3_rounding  x = 3, -3, 0, 0, 0 and y = 0, 0, 1, 1, -2: the sums are 18 and 6, and
                    fl(18 / 5) > 3 fl(6 / 5) in float64 (3 * fl(1.2) is a tie that rounds down),
                    so with line_ratio = 3 the point is valid under the division by 5 the
                    definition states; divided by 4 the two sides are 4.5 and 4.5.
      gate          x = 0, 1, 2, 3, 4: for the end points d2[3] = 9/16 and d2[4] = 1 = GATE_D2.
    exact_oblique: exactly collinear lattice points along (1, 1, 0), (1, -1, 0) and (1, 1, 1):
    lambda2 = 0 up to the eigensolver's rounding, the two (three) largest |u| components equal."""
    tie = [-3, -2, -1, 0, 1, 3]
    diag = _clusters([
        _on_x(tie), _on_x(tie[::-1]), _on_x([0, 1, -1, -2, 3, -3]), _on_x([3, -3, -2, -1, 1, 0]),
        [[5, 3, 1]] * 5,
        [[0, 0, z] for z in (0, 1, 2, 4, 5, 7)],
        [[8, 0, 0], [-8, 0, 0], [0, 4, 0], [0, -4, 0], [0, 0, 0]],
        [[9, 0, 0], [-9, 0, 0], [0, 4, 0], [0, -4, 0], [0, 0, 0]],
        [[3, 0, 0], [-3, 0, 0], [0, 1, 0], [0, 1, 0], [0, -2, 0]],
        _on_x([0, 1, 2, 3, 4]),
    ])
    obl = _clusters([[[k, k, 0] for k in range(6)], [[k, -k, 0] for k in range(6)], [[k, k, k] for k in range(6)]])
    return {"exact_diag": diag, "exact_oblique": obl}


def exact_cluster_rows(name):
    """the rows of exact_diag that belong to the named cluster"""
    sizes = [6, 6, 6, 6, 5, 6, 5, 5, 5, 5]
    k = EXACT_DIAG_CLUSTERS.index(name)
    return np.arange(sum(sizes[:k]), sum(sizes[:k + 1]))


@dataclass(frozen=True)
class LineBatch:
    name: str
    frames: tuple            # of (frame name, [m, 4] float32)
    max_nn_d2: float
    line_ratio: float
    exact: bool = False      # integer / 4 geometry: centroid bits; exact_diag frames: no margins


@functools.lru_cache(maxsize=None)
def line_batches():
    sz, nz, ex = size_frames(), noisy_frames(), exact_frames()
    sizes = tuple((f"m{m}", sz[m]) for m in SIZES)
    noisy = tuple(nz.items())
    exact = tuple(ex.items())
    above = float(np.nextafter(F32(GATE_D2), F32(np.inf)))
    return (
        LineBatch("sizes", sizes + noisy, DEFAULT_D2, DEFAULT_RATIO),
        # the global-memory path and the LDS path in one launch, around an empty frame
        LineBatch("mixed", (("m8193", sz[8193]), ("m6", sz[6]), ("m0", sz[0]), ("m1025", sz[1025])), DEFAULT_D2,
                  DEFAULT_RATIO),
        LineBatch("exact_ratio4", exact, 100.0, 4.0, exact=True),
        LineBatch("exact_ratio3", exact, 100.0, 3.0, exact=True),
        LineBatch("exact_gate_at", exact, GATE_D2, 4.0, exact=True),
        LineBatch("exact_gate_above", exact, above, 4.0, exact=True),
    )


_TABLES = {}


def yardstick_table(fname, frame, max_nn_d2, line_ratio, variant=None):
    """tests/edge_reference.py's table of a frame, computed once per (frame, parameters)"""
    key = (fname, float(max_nn_d2), float(line_ratio), variant)
    if key not in _TABLES:
        kw = er.LINE_VARIANTS[variant] if variant else {}
        _TABLES[key] = er.line_table(frame, max_nn_d2, line_ratio, **kw)
    return _TABLES[key]


# ------------------------------------------------------------------------------- the bars
RATIO_CLEAR = 1e-9            # |lambda1 / (line_ratio lambda2) - 1| above it: the ratio test is asserted
ANISO_MIN = 0.5               # (lambda1 - lambda2) / lambda1 from which the direction is compared
DIR_TOL = 2.0 ** -23          # per component: two casts of values <= 1 that agree to ~1e-15 / gap
SIGN_CLEAR = 1e-6             # difference of the two largest |u| above it: the sign is asserted


def _adjacent(a, b):
    """equal or adjacent float32, element-wise"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a == b) | (a == np.nextafter(b, F32(np.inf))) | (a == np.nextafter(b, F32(-np.inf)))


def compare_table(line, valid, y, max_nn_d2, exact=False, always=False):
    """A line table (line [m, 6] float32, valid [m]) against the yardstick's y for one frame.
    -> (failures: list of str, stats: dict(asserted_ratio, unclear_ratio, dir_compared,
    sign_open, worst_dir, cen_differs: rows whose centroid is not the yardstick's bits,
    signs: [(row, got sign, yardstick sign)] of the rows compared up to sign)).

    valid: the gate (the same float32 d2 on both sides) on every point -- a closed gate means
    valid = 0 whatever the ratio; the ratio test where the yardstick's ratio is clear of 1 by
    RATIO_CLEAR, or everywhere when `always` (diagonal covariances).  Centroid: equal bits when
    `exact`, else equal or adjacent float32.  Direction: on the yardstick's valid rows and where
    aniso >= ANISO_MIN, per component within DIR_TOL; up to sign where sign_gap <= SIGN_CLEAR."""
    line = np.asarray(line, F32).reshape(-1, 6)
    valid = np.asarray(valid).reshape(-1).astype(np.uint8)
    m = len(y["valid"])
    bad = []
    stats = dict(asserted_ratio=0, unclear_ratio=0, dir_compared=0, sign_open=0, worst_dir=0.0, cen_differs=0,
                 signs=[])
    if line.shape[0] != m or valid.shape[0] != m:
        return [f"shape {line.shape} / {valid.shape} for {m} points"], stats
    if m < er.K:
        if np.any(line.view(np.uint32) != 0) or np.any(valid != 0):
            bad.append("m < 5: not all zeros")
        return bad, stats
    gate = y["d2"][:, er.K - 1] < F32(max_nn_d2)
    with np.errstate(invalid="ignore"):
        clear = np.abs(y["ratio"] - 1.0) > RATIO_CLEAR              # NaN (0 / 0): not clear
    if always:
        clear = np.ones(m, bool)
    stats["asserted_ratio"], stats["unclear_ratio"] = int(clear.sum()), int((~clear).sum())
    if np.any(valid[~gate] != 0):
        bad.append(f"valid with a closed gate at rows {np.nonzero(valid[~gate] != 0)[0][:5].tolist()}")
    w = np.nonzero(clear & (valid != y["valid"]))[0]
    if len(w):
        bad.append(f"valid differs at rows {w[:5].tolist()} (ratio {y['ratio'][w[:5]].tolist()})")
    # centroid
    gc, yc = line[:, :3], y["line"][:, :3]
    if exact:
        w = np.nonzero((gc.view(np.uint32) != yc.view(np.uint32)).any(1))[0]
    else:
        w = np.nonzero(~_adjacent(gc, yc).all(1))[0]
    stats["cen_differs"] = int((gc.view(np.uint32) != yc.view(np.uint32)).any(1).sum())
    if len(w):
        bad.append(f"centroid differs at rows {w[:5].tolist()}: {gc[w[0]].tolist()} / {yc[w[0]].tolist()}")
    # direction
    with np.errstate(invalid="ignore"):
        cmp_rows = (y["valid"] != 0) | (y["aniso"] >= ANISO_MIN)
    gu, yu = line[:, 3:].astype(np.float64), y["line"][:, 3:].astype(np.float64)
    same = np.abs(gu - yu).max(1)
    flipped = np.abs(gu + yu).max(1)
    with np.errstate(invalid="ignore"):
        sign_open = ~(y["sign_gap"] > SIGN_CLEAR)
    err = np.where(sign_open, np.minimum(same, flipped), same)
    stats["dir_compared"] = int(cmp_rows.sum())
    stats["sign_open"] = int((cmp_rows & sign_open).sum())
    if cmp_rows.any():
        stats["worst_dir"] = float(err[cmp_rows].max())
    for a in np.nonzero(cmp_rows & sign_open)[0][:8]:
        k = int(np.argmax(np.abs(yu[a])))
        stats["signs"].append((int(a), float(np.sign(gu[a, k])), float(np.sign(yu[a, k]))))
    w = np.nonzero(cmp_rows & ~(err <= DIR_TOL))[0]
    if len(w):
        bad.append(f"direction differs at rows {w[:5].tolist()}: {gu[w[0]].tolist()} / {yu[w[0]].tolist()} "
                   f"(aniso {y['aniso'][w[0]]:.3g}, sign gap {y['sign_gap'][w[0]]:.3g})")
    return bad, stats


def always_asserted(fname):
    return fname == "exact_diag"

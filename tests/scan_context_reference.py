"""numpy yardstick of ssf_scan_context_batch / ssf_scan_context_match (include/ssf_frontend.h,
DESIGN.md §6.12), written from the definitions alone: float64 geometry on the float32 points,
a float64 distance.  It does not import the product code.

  descriptor  a point with a non-finite coordinate or r = sqrt(x^2 + y^2) >= max_range is skipped;
              ring = min(floor(r / (max_range / 20)), 19), sector = min(floor(phi / (2 pi / 60)), 59),
              phi = atan2(y, x) in [0, 2 pi); desc[ring][sector] = max(0, max of the float32 sum
              z + lidar_height); an empty bin is 0.
  distance    valid columns (any bin > 0) scaled to unit length, invalid ones zero; J(s) the columns
              j where q[:, j] and c[:, (j + s) % 60] are both valid; d(s) = 1 - sum_J q_j . c_(j+s) / |J|,
              1 when J is empty; dist = min_s d(s), shift the smallest s that attains it.
  selection   the smallest (dist, index) of candidates 0 .. n_eligible - 1, index -1 without one.
"""
import numpy as np

RINGS, SECTORS = 20, 60
MAX_RANGE, LIDAR_HEIGHT = 80.0, 2.0
SECTOR_ANGLE = 2.0 * np.pi / SECTORS


def bins(pts, max_range=MAX_RANGE):
    """Per point of [n, >= 3] float32: (keep, ring, sector, ring_margin_m, sector_margin_rad) --
    keep: finite and r < max_range; the margins are the float64 distances to the nearest ring edge
    (the edge at max_range included, the one at 0 not: no point crosses it) and to the nearest
    sector edge (the wrap at 0 = 2 pi included); inf for a point with a non-finite coordinate."""
    p = np.asarray(pts, np.float32)[:, :3].astype(np.float64)
    fin = np.isfinite(p).all(axis=1)
    x, y = np.where(fin, p[:, 0], 0.0), np.where(fin, p[:, 1], 0.0)
    r = np.sqrt(x * x + y * y)
    ring_w = max_range / RINGS
    keep = fin & (r < max_range)
    ring = np.minimum(np.floor(r / ring_w), RINGS - 1).astype(np.int64)
    phi = np.arctan2(y, x)
    phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
    sector = np.minimum(np.floor(phi / SECTOR_ANGLE), SECTORS - 1).astype(np.int64)
    k = np.floor(r / ring_w)                          # the edges are k * ring_w, k = 1 .. 20
    below = np.where(k >= 1, np.abs(r - np.minimum(k, RINGS) * ring_w), np.inf)
    above = np.where(k + 1 <= RINGS, np.abs((k + 1) * ring_w - r), np.inf)
    ring_margin = np.minimum(below, above)
    sector_margin = np.abs(phi - np.round(phi / SECTOR_ANGLE) * SECTOR_ANGLE)
    ring_margin = np.where(fin, ring_margin, np.inf)
    sector_margin = np.where(fin, sector_margin, np.inf)
    return keep, ring, sector, ring_margin, sector_margin


def heights(pts, lidar_height=LIDAR_HEIGHT):
    """The float32 sum z + lidar_height per point."""
    z = np.asarray(pts, np.float32)[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return (z + np.float32(lidar_height)).astype(np.float32)


def describe(pts, max_range=MAX_RANGE, lidar_height=LIDAR_HEIGHT):
    """[n, >= 3] float32 -> desc [20, 60] float32."""
    pts = np.asarray(pts, np.float32)
    desc = np.zeros((RINGS, SECTORS), np.float32)
    if pts.size == 0:
        return desc
    keep, ring, sector, _, _ = bins(pts, max_range)
    h = heights(pts, lidar_height)
    np.maximum.at(desc, (ring[keep], sector[keep]), h[keep])       # desc starts at 0: the max(0, .)
    return desc


def describe_batch(pts, sizes, max_range=MAX_RANGE, lidar_height=LIDAR_HEIGHT):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.stack([describe(pts[off[k]:off[k + 1]], max_range, lidar_height) for k in range(len(sizes))]) \
        if len(sizes) else np.zeros((0, RINGS, SECTORS), np.float32)


def normalise(desc):
    """-> (unit columns [20, 60] float64, valid [60] bool)."""
    d = np.asarray(desc, np.float64)
    valid = (d > 0).any(axis=0)
    n = np.sqrt((d * d).sum(axis=0))
    out = np.zeros_like(d)
    out[:, valid] = d[:, valid] / n[valid]
    return out, valid


def shift_distances(q, c):
    """d(s) for s = 0 .. 59, float64."""
    qn, qv = normalise(q)
    cn, cv = normalise(c)
    d = np.ones(SECTORS, np.float64)
    for s in range(SECTORS):
        cs, cvs = np.roll(cn, -s, axis=1), np.roll(cv, -s)        # column j <- c[:, (j + s) % 60]
        J = qv & cvs
        if J.any():
            d[s] = 1.0 - (qn[:, J] * cs[:, J]).sum() / J.sum()
    return d


def distance(q, c):
    """-> (dist, shift): the minimum of d(s) and the smallest s that attains it."""
    d = shift_distances(q, c)
    s = int(np.argmin(d))                                          # the first minimum
    return float(d[s]), s


def match(queries, db):
    """-> dist [Q, N] float64, shift [Q, N] int64, dall [Q, N, 60] float64: shift_distances of
    every pair, a query against all candidates at once."""
    Q, N = len(queries), len(db)
    dall = np.ones((Q, N, SECTORS), np.float64)
    cand = [normalise(c) for c in db]
    cn = np.stack([c[0] for c in cand]) if N else np.zeros((0, RINGS, SECTORS))
    cv = np.stack([c[1] for c in cand]) if N else np.zeros((0, SECTORS), bool)
    for a in range(Q):
        qn, qv = normalise(queries[a])
        for s in range(SECTORS if N else 0):
            cs, cvs = np.roll(cn, -s, axis=2), np.roll(cv, -s, axis=1)
            J = qv[None, :] & cvs                                  # [N, 60]
            num = ((qn[None] * cs).sum(axis=1) * J).sum(axis=1)
            cnt = J.sum(axis=1)
            dall[a, :, s] = np.where(cnt > 0, 1.0 - num / np.maximum(cnt, 1), 1.0)
    shift = dall.argmin(axis=2) if N else np.zeros((Q, 0), np.int64)
    dist = dall.min(axis=2) if N else np.zeros((Q, 0), np.float64)
    return dist, shift, dall


def select(dist_row, n_eligible):
    """The smallest (dist, index) of the first n_eligible entries -> index, -1 without one."""
    n = int(n_eligible)
    if n == 0:
        return -1
    d = np.asarray(dist_row, np.float64)[:n]
    return int(np.lexsort((np.arange(n), d))[0])


def eligible_prefix(stamps, cur_stamp, time_gap):
    """Leading keyframes more than time_gap older than cur_stamp, up to the first that is not."""
    n = 0
    for s in stamps:
        if cur_stamp - s > time_gap:
            n += 1
        else:
            break
    return n


def rot_z(pts, deg):
    """Points rotated about z by deg (float64 arithmetic, float32 result; further columns kept)."""
    a = np.deg2rad(float(deg))
    c, s = np.cos(a), np.sin(a)
    out = np.array(pts, np.float32, copy=True)
    x, y = out[:, 0].astype(np.float64), out[:, 1].astype(np.float64)
    out[:, 0] = (c * x - s * y).astype(np.float32)
    out[:, 1] = (s * x + c * y).astype(np.float32)
    return out

"""Numpy yardstick of the TFlow point-set operators (csrc/pointnet2.hip, oracle/pn2_oracle.c),
written from the reference's torch text alone -- scripts/ActiveSceneFlow/utils/utils.py:48-108
(index_points, farthest_point_sample, knn_point) and :658-663 (the weighted 3-NN sum),
utils/soflow.py:1442-1470 (UpsampleFlow.forward) -- and built unlike the oracle and the kernels:
whole distance matrices, np.lexsort, fancy indexing; no insertion lists, no tiles.

Two layers per operator.

float32 layer: defines the bits.  Every numpy float32 elementwise operation rounds once, so the
order of the expression fixes the result:
  d2          = (dx*dx + dy*dy) + dz*dz of the float32 differences (utils.py:85 / :106)
  knn         = np.lexsort((index, d2))[:k]: ascending, ties to the lower index (what a stable
                top-k over ascending indices returns; torch.topk itself leaves ties open);
                distance = float32 sqrt (:108)
  fps         = the loop of :82-89: distance = 1e10, minimum, first-maximum argmax
  interpolate = (w0*f0 + w1*f1) + w2*f2 (:662)
  upsample    = d = max(sqrt(d2), 1e-10) (:1463), w = (1/d) / (sum of the 1/d in neighbour order)
                (:1464-1465), sum of w*f in neighbour order (:1471), clip to +-100 (:1475)

Project rules where the reference leaves the answer open or raises:
  * fps start: the reference draws it at random (:80).  Here it is an argument, default 0,
    clamped to [0, n-1]; the reference would raise an IndexError for a value outside.
  * knn with k > n: ranks >= n return index 0 and distance 0 (torch.topk raises).
  * upsample uses min(k, s) neighbours (the reference's top-k raises for k > s).
  * gather / group / group_relative / three_interpolate with an index outside [0, n): that
    element reads as 0 (0 - centre for group_relative's coordinates) and the `bad` flag is
    raised; every other element is untouched (torch raises, or wraps a negative index).
  * fps with npoint > n goes on as the loop does: every distance is 0, the first maximum is 0.

float64 layer: guards the definition.  d2 of the float32 inputs in float64 and, per (query,
rank), `gap`: the smaller of the relative gaps (b - a) / b to the neighbouring ranks of the
float64 order (the gap between ranks k-1 and k is the last rank's upper one).  A float32 d2
carries at most five roundings (a difference squared: 2u, the product's own: u, two sums: 2u;
u = 2^-24), so two candidates whose float64 gap is above 10u cannot change places; the bar is
GAP_BAR = 2^-20, and where gap > GAP_BAR the float32 index must be the float64 one.

Arithmetic bars (first order in u, denominators 1 - c u kept):
  three_interpolate: three products (u each) and two sums: |f32 - f64| <= 3u sum|w f|.
  upsample, per output, on the float32 layer's neighbour indices:
      d2 5u -> sqrt halves it and rounds: 3.5u -> 1/d: 4.5u = e_r
      norm = k-term sum of positive terms: e_r + (k-1)u
      w = r / norm: e_r + (e_r + (k-1)u) + u = (k + 9)u   (a worst case: r_j high, the rest low)
      w*f: +u; the k-term sum: +(k-1)u                   -> (2k + 9)u sum|w f|
  The issue's sketch of the bound, (2k + 7)u, counts e_r once; r_j and the norm are rounded
  apart, so the worst case has it twice and the constant here is 2k + 9.  max(., 1e-10) and the
  clip are 1-Lipschitz and add nothing.

Domain: finite coordinates, weights and features.  NaN inputs, and an upsample point whose
neighbours' float32 d2 are all infinite (weights 0 / 0), are outside the definition: asserted.

VARIANTS: deliberately wrong rules, each a switch of the float32 layer; tests/test_pn2_host.py
shows that each changes the output of a named case.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
GAP_BAR = 2.0 ** -20
CAP = F32(1e10)
DMIN = F32(1e-10)
CLIP = F32(100.0)
TINY = 8 * 2.0 ** -149          # room for products that underflow: absolute, not relative

VARIANTS = {
    "ties to the higher index": ("knn", "ties_high"),
    "d2 by the expanded form": ("knn", "expanded"),
    "d2 with fused multiply-add": ("knn", "fma"),
    "d2 summed z-first": ("knn", "zfirst"),
    "selection by float64 d2": ("knn", "select_f64"),
    "fps without the 1e10 cap": ("fps", "nocap"),
    "fps last-maximum": ("fps", "lastmax"),
    "clamp before sqrt": ("upsample", "clamp_first"),
    "weights normalised after the product": ("upsample", "norm_after"),
    "no +-100 clip": ("upsample", "noclip"),
    "interpolate summed right to left": ("interpolate", "rtl"),
}


def _f32(a, what):
    a = np.ascontiguousarray(a, F32)
    assert np.isfinite(a).all(), f"{what}: outside the domain (non-finite value)"
    return a


# ------------------------------------------------------------------------------- distances
def d2_f32(query, ref, variant=None):
    """query [B, S, 3], ref [B, N, 3] -> float32 [B, S, N]"""
    q, r = _f32(query, "query"), _f32(ref, "ref")
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if variant == "expanded":                               # square_distance, utils.py:42-44
            dot = (q[:, :, None, 0] * r[:, None, :, 0] + q[:, :, None, 1] * r[:, None, :, 1]) \
                + q[:, :, None, 2] * r[:, None, :, 2]
            d = F32(-2) * dot
            d = d + ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2])[:, :, None]
            return d + ((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2])[:, None, :]
        dx, dy, dz = (r[:, None, :, c] - q[:, :, None, c] for c in range(3))
        if variant == "fma":                                    # fma(dz, dz, fma(dy, dy, dx*dx))
            t = dx * dx
            t = (dy.astype(np.float64) * dy + t).astype(F32)
            return (dz.astype(np.float64) * dz + t).astype(F32)
        if variant == "zfirst":
            return (dz * dz + dy * dy) + dx * dx
        return (dx * dx + dy * dy) + dz * dz


def d2_f64(query, ref):
    q, r = _f32(query, "query").astype(np.float64), _f32(ref, "ref").astype(np.float64)
    d = r[:, None, :, :] - q[:, :, None, :]
    return (d * d).sum(-1)


def _order(key, higher=False):
    index = np.broadcast_to(np.arange(key.shape[-1]), key.shape)
    return np.lexsort((-index if higher else index, key))


def neighbours(query, ref, kmax, variant=None):
    """(float32 d2, index) of the min(kmax, n) nearest, [B, S, min(kmax, n)]"""
    d2 = d2_f32(query, ref, variant)
    key = d2_f64(query, ref) if variant == "select_f64" else d2
    order = _order(key, variant == "ties_high")[..., :kmax]
    return np.take_along_axis(d2, order, -1), order


# ------------------------------------------------------------------------------- k-NN
def knn(k, query, ref, variant=None, nbr=None):
    """-> (dist float32, idx int32), [B, S, k]"""
    d2k, order = neighbours(query, ref, k, variant) if nbr is None else nbr
    d2k, order = d2k[..., :k], order[..., :k]
    m = order.shape[-1]
    dist = np.zeros(order.shape[:2] + (k,), F32)
    idx = np.zeros(order.shape[:2] + (k,), np.int32)
    with np.errstate(invalid="ignore"):
        dist[..., :m] = np.sqrt(d2k)
    idx[..., :m] = order
    return dist, idx


def knn64(k, query, ref):
    """-> (idx [B, S, k] of the float64 order, gap [B, S, k]); ranks >= n: index 0, gap inf"""
    d2 = d2_f64(query, ref)
    n = d2.shape[-1]
    order = _order(d2)[..., :k + 1]
    e = np.take_along_axis(d2, order, -1)
    m = min(k, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(e[..., 1:] > 0, (e[..., 1:] - e[..., :-1]) / e[..., 1:], 0.0)   # [.., min(k, n-1)]
    up = np.full(d2.shape[:2] + (k,), np.inf)
    up[..., :rel.shape[-1]] = rel
    lo = np.full_like(up, np.inf)
    lo[..., 1:] = up[..., :-1]
    gap = np.minimum(up, lo)
    gap[..., m:] = np.inf
    idx = np.zeros(d2.shape[:2] + (k,), np.int64)
    idx[..., :m] = order[..., :m]
    return idx, gap


def check_decisive(idx32, idx64, gap):
    """-> (number of decisive (query, rank) pairs that disagree, share of non-decisive pairs)"""
    dec = gap > GAP_BAR
    return int(np.count_nonzero(dec & (idx32 != idx64))), float(1.0 - dec.mean()) if dec.size else 0.0


# ------------------------------------------------------------------------------- FPS
def fps(xyz, npoint, start=None, variant=None):
    """xyz [B, N, 3] -> int32 [B, npoint]"""
    x = _f32(xyz, "xyz")
    B, n, _ = x.shape
    out = np.zeros((B, npoint), np.int32)
    for b in range(B):
        distance = np.full(n, np.inf if variant == "nocap" else CAP, F32)
        far = 0 if start is None else int(np.clip(int(start[b]), 0, n - 1))
        for i in range(npoint):
            out[b, i] = far
            d = x[b] - x[b, far]
            dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            distance = np.minimum(distance, dist)
            far = int(n - 1 - np.argmax(distance[::-1])) if variant == "lastmax" else int(np.argmax(distance))
    return out


def fps64(xyz, idx, start=None):
    """Follows the float32 layer's choices in float64: -> (want [B, npoint], gap [B, npoint]),
    the float64 first maximum at every step and the relative gap of its distance to the second
    largest.  Step 0 is the start itself (gap inf)."""
    x = _f32(xyz, "xyz").astype(np.float64)
    B, n, _ = x.shape
    want = np.zeros(idx.shape, np.int64)
    gap = np.full(idx.shape, np.inf)
    for b in range(B):
        distance = np.full(n, float(CAP))
        want[b, 0] = 0 if start is None else int(np.clip(int(start[b]), 0, n - 1))
        for i in range(1, idx.shape[1]):
            d = x[b] - x[b, idx[b, i - 1]]
            distance = np.minimum(distance, (d * d).sum(-1))
            want[b, i] = int(np.argmax(distance))
            if n > 1:
                two = np.partition(distance, n - 2)[n - 2:]
                gap[b, i] = (two[1] - two[0]) / two[1] if two[1] > 0 else 0.0
    return want, gap


# ------------------------------------------------------------------------------- gathers
def gather(feat, idx):
    """feat [B, C, N], idx [B, ...] -> (float32 [B, C, ...], bad)"""
    f = _f32(feat, "features")
    ix = np.asarray(idx, np.int64)
    B, C, n = f.shape
    ok = (ix >= 0) & (ix < n)
    flat = np.where(ok, ix, 0).reshape(B, 1, -1)
    out = np.take_along_axis(f, np.broadcast_to(flat, (B, C, flat.shape[-1])), 2)
    out = np.where(ok.reshape(B, 1, -1), out, F32(0)).astype(F32)
    return out.reshape((B, C) + ix.shape[1:]), bool((~ok).any())


def group_relative(xyz, new_xyz, points, idx):
    """utils.py:228-234: xyz [B, 3, N], new_xyz [B, 3, S], points [B, C, N] or None,
    idx [B, S, K] -> (float32 [B, 3 + C, S, K], bad)"""
    g, bad = gather(xyz, idx)
    out = g - _f32(new_xyz, "new_xyz")[..., None]
    if points is not None:
        out = np.concatenate([out, gather(points, idx)[0]], axis=1)
    return out, bad


def three_interpolate(feat, idx, weight, variant=None):
    """feat [B, C, M], idx / weight [B, N, 3] -> (float32 [B, C, N], bad)"""
    g, bad = gather(feat, idx)                                   # [B, C, N, 3]
    p = g * _f32(weight, "weight")[:, None]
    if variant == "rtl":
        return (p[..., 2] + p[..., 1]) + p[..., 0], bad
    return (p[..., 0] + p[..., 1]) + p[..., 2], bad


def three_interpolate64(feat, idx, weight):
    """-> (float64 value, bound on |float32 - float64|)"""
    g, _ = gather(feat, idx)
    p = g.astype(np.float64) * _f32(weight, "weight").astype(np.float64)[:, None]
    return p.sum(-1), 3 * U / (1 - 3 * U) * np.abs(p).sum(-1) + TINY


# ------------------------------------------------------------------------------- upsample
def upsample_flow(xyz, sparse_xyz, sparse_feat, k, variant=None, nbr=None):
    """xyz [B, 3, N], sparse_xyz [B, 3, S], sparse_feat [B, C, S] -> (float32 [B, C, N],
    neighbour indices [B, N, min(k, s)])"""
    q = np.ascontiguousarray(np.transpose(xyz, (0, 2, 1)))
    r = np.ascontiguousarray(np.transpose(sparse_xyz, (0, 2, 1)))
    f = _f32(sparse_feat, "sparse_feat")
    d2k, idx = neighbours(q, r, k) if nbr is None else nbr
    d2k, idx = d2k[..., :k], idx[..., :k]
    assert np.isfinite(d2k).any(-1).all(), "upsample: outside the domain (every neighbour at d2 = inf)"
    m = idx.shape[-1]
    with np.errstate(over="ignore", under="ignore"):
        d = np.sqrt(np.maximum(d2k, DMIN)) if variant == "clamp_first" else np.maximum(np.sqrt(d2k), DMIN)
        rcp = F32(1) / d
        norm = rcp[..., 0]
        for j in range(1, m):
            norm = norm + rcp[..., j]
        w = rcp if variant == "norm_after" else rcp / norm[..., None]
        g = gather(f, idx)[0]                                    # [B, C, N, m]
        acc = w[:, None, :, 0] * g[..., 0]
        for j in range(1, m):
            acc = acc + w[:, None, :, j] * g[..., j]
        if variant == "norm_after":
            acc = acc / norm[:, None]
    return (acc if variant == "noclip" else np.clip(acc, -CLIP, CLIP)).astype(F32), idx


def upsample_flow64(xyz, sparse_xyz, sparse_feat, idx):
    """The formula in float64 on the given neighbour indices -> (value, bound)"""
    x = _f32(xyz, "xyz").astype(np.float64)                      # [B, 3, N]
    f = _f32(sparse_feat, "sparse_feat")
    k = idx.shape[-1]
    gx = gather(sparse_xyz, idx)[0].astype(np.float64) - x[..., None]    # [B, 3, N, k]
    d = np.maximum(np.sqrt((gx * gx).sum(1)), float(DMIN))
    w = (1.0 / d) / (1.0 / d).sum(-1, keepdims=True)
    p = w[:, None] * gather(f, idx)[0].astype(np.float64)
    c = (2 * k + 9) * U
    return np.clip(p.sum(-1), -100.0, 100.0), c / (1 - c) * np.abs(p).sum(-1) + TINY

"""Seeded, named cases for the TFlow point-set operators at the smallest shapes that reach every
path edge of csrc/pointnet2.hip, with the yardstick's answers (tests/pn2_reference.py) computed
once per case and shared by tests/test_pn2_host.py (oracle) and tests/test_gpu_pn2_yardstick.py
(device).

Path edges: the four FPS kernels change at n = 4096 | 8192 | 16384; the two k-NN launch families
at b * ceil(s / 256) = 512, each with list lengths 4 | 8 | 16 | 32; LDS tiles of 2048 points
split into wave slices of 256 (k <= 16) or 512 points (k > 16); an odd tile or slice ends in a
scalar element after the packed pairs; gathers and the interpolation stage rows of n <= 36864
floats in LDS, ceil(c b / 512) channels per work-group; upsample's two launch families change at
b * ceil(n / 256) = 512.

A seeded case is admitted on the yardstick alone: at most MAX_UNCLEAR of its (query, rank) pairs
may be non-decisive by the 2^-20 rule, and none of its decisive pairs may differ between the
yardstick's two layers (asserted at import for every seeded k-NN and upsample case; the FPS
cases, whose float64 layer follows the float32 choices, in tests/test_pn2_host.py).  The
constructed tie cases (`exact=True`) are held by bit equality only.
"""
import functools
from collections import namedtuple

import numpy as np

import pn2_reference as ref

F32 = np.float32
MAX_UNCLEAR = 0.05
KS = (1, 3, 4, 5, 8, 9, 16, 17, 32)
UP_KS = (1, 3, 4, 5, 8, 9, 16)
STAGE = 36864                                   # floats of an LDS-staged feature row

FpsCase = namedtuple("FpsCase", "name xyz npoint start exact")
KnnCase = namedtuple("KnnCase", "name query ref ks exact")
GatherCase = namedtuple("GatherCase", "name feat idx")
RelCase = namedtuple("RelCase", "name xyz new_xyz points idx")
InterpCase = namedtuple("InterpCase", "name feat idx weight")
UpCase = namedtuple("UpCase", "name xyz sxyz sfeat ks")


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _noise(rng, b, n, scale=20.0):
    return (rng.standard_normal((b, n, 3)) * scale).astype(F32)


# ------------------------------------------------------------------------------- FPS
def lattice_twice(n, shift=0):
    """integer lattice, every point twice (at i and i + ceil(n / 2)): every d2 is exact, ties
    across lanes, waves and register slots"""
    m = (n + 1) // 2
    i = (np.arange(n) % m) + shift
    return np.stack([i % 16, (i // 16) % 16, i // 256], -1).astype(F32)


def two_clusters(rng, n):
    """two clusters 2e5 apart, interleaved by index: every point of the far one is capped at 1e10
    after the first step, so the first of them wins, not the farthest"""
    x = (rng.standard_normal((n, 3)) * 5).astype(F32)
    x[1::2, 0] += F32(2e5)
    return x


FPS_N = (1, 2, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385)


@functools.lru_cache(maxsize=None)
def fps_cases():
    out = []
    for i, n in enumerate(FPS_N):
        rng = _rng(1, n)
        starts = (None, [0, n // 3, n - 1], [-5, -1, -2 ** 31], [n, n + 7, 2 ** 31 - 1])[i % 4]
        st = None if starts is None else np.array(starts, np.int32)
        tie = np.stack([lattice_twice(n), lattice_twice(n, 3), two_clusters(rng, n)])
        out.append(FpsCase(f"fps_ties_n{n}", tie, 64, st, True))
        out.append(FpsCase(f"fps_noise_n{n}", _noise(rng, 3, n), 33, st, False))
    for n in (257, 8193, 16385):
        out.append(FpsCase(f"fps_equal_n{n}", np.full((1, n, 3), F32(1.5)), 5, np.array([n - 2], np.int32), True))
    small = lattice_twice(37)[None]
    for tag, st in (("none", None), ("in", [20]), ("neg", [-3]), ("past", [37])):
        out.append(FpsCase(f"fps_npoint_eq_n_start_{tag}", small, 37, None if st is None else np.array(st, np.int32), True))
    out.append(FpsCase("fps_npoint_gt_n", small, 50, None, True))
    out.append(FpsCase("fps_npoint_gt_n_noise", _noise(_rng(1, 0), 1, 37), 50, None, False))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fps_yard(name):
    cs = next(c for c in fps_cases() if c.name == name)
    return ref.fps(cs.xyz, cs.npoint, cs.start)


# ------------------------------------------------------------------------------- k-NN
KNN_N = (1, 7, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4097)
KNN_S = (1, 63, 64, 65, 300)


def _fma_tail(n):
    """The query is the origin.  The last point W (the scalar tail of an odd tile) wins rank 0 by
    one float32 step over point 0 = (t, 0, 0), whose d2 = fl(t t) is what W's d2 becomes under
    fused multiply-add: there they tie and the lower index wins."""
    rng = _rng(7, n)
    while True:
        w = (rng.uniform(1, 2, (1, 1, 3))).astype(F32)
        o = np.zeros((1, 1, 3), F32)
        a, a2 = ref.d2_f32(o, w)[0, 0, 0], ref.d2_f32(o, w, "fma")[0, 0, 0]
        if a2 != np.nextafter(a, F32(np.inf)):
            continue
        t = np.sqrt(a2)
        if t * t == a2:
            break
    pts = (rng.standard_normal((1, n, 3)) * 3 + 40).astype(F32)
    pts[0, 0] = (t, 0, 0)
    pts[0, n - 1] = w[0, 0]
    return KnnCase(f"knn_fma_tail_n{n}", np.zeros((1, 1, 3), F32), pts, KS, True)


@functools.lru_cache(maxsize=None)
def knn_cases():
    out = []
    # the split family: b small
    for i, n in enumerate(KNN_N):
        s, b = KNN_S[i % len(KNN_S)], (3, 1)[i % 2]
        rng = _rng(2, n)
        q = _noise(rng, b, s)
        r = _noise(rng, b, n)
        out.append(KnnCase(f"knn_split_n{n}_s{s}_b{b}", q, r, KS, False))
    for s in KNN_S:
        rng = _rng(3, s)
        out.append(KnnCase(f"knn_split_n2049_s{s}_b2", _noise(rng, 2, s), _noise(rng, 2, 2049), KS, False))
    # the 256-thread family: b * ceil(s / 256) = 512
    for n in KNN_N:
        s = 3 if n <= 513 else 1
        rng = _rng(4, n)
        out.append(KnnCase(f"knn_wide_n{n}_s{s}_b512", _noise(rng, 512, s), _noise(rng, 512, n), KS, False))
    for wide in (False, True):
        tag, b = ("wide", 512) if wide else ("split", 1)
        rep = lambda a: np.array(np.broadcast_to(a, (b,) + a.shape[1:]))                     # noqa: E731
        # the wide family's elements differ: element e takes the queries rotated by e
        rot = lambda q: np.stack([np.roll(q[0], -e, axis=0) for e in range(b)])              # noqa: E731
        # exact duplicates across the slice and tile edges, queries on and beside them
        rng = _rng(5, b)
        r = _noise(rng, 1, 2050)
        for e in (256, 512, 2048):
            r[0, e] = r[0, e - 1]
        q = np.concatenate([r[:, [255, 511, 2047]], r[:, [256]] + F32(0.25)], 1)
        out.append(KnnCase(f"knn_dups_straddle_{tag}", rot(q[:, :3 if wide else 4]), rep(r), KS, True))
        # queries on reference points: d2 = 0
        r = _noise(rng, 1, 513)
        out.append(KnnCase(f"knn_on_refs_{tag}", rot(r[:, [0, 256, 512]]), rep(r), KS, True))
        # integer lattice: shells of 6, 12, 8, 6, 24 ... equidistant points, cut by every k
        g = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(1, -1, 3).astype(F32)
        out.append(KnnCase(f"knn_lattice_{tag}", rot(g[:, [171, 0, 342]]), rep(g), KS, True))
        # d2 in the float32 denormal range, exact: coordinates m 2^-70, |m| <= 40
        m = rng.integers(-40, 41, (1, 300, 3)).astype(F32) * F32(2.0 ** -70)
        out.append(KnnCase(f"knn_denormal_{tag}", rot(m[:, :3] + F32(2.0 ** -70)), rep(m), KS, True))
        # d2 = +inf: ten candidates near +-1e20 around three real points; they follow every real
        # point in index order (and n = 13 < 16, 17, 32)
        r = np.full((1, 13, 3), 1e20, F32) * np.where(np.arange(13) % 2, -1, 1).astype(F32)[None, :, None]
        r[0, [4, 7, 12]] = [[1, 2, 3], [0, 0, 1], [-2, 0, 0]]
        out.append(KnnCase(f"knn_inf_{tag}", rot(np.array([[[0, 0, 0], [1, 1, 1], [5, 0, 0]]], F32)), rep(r), KS, True))
    out.append(_fma_tail(257))
    out.append(_fma_tail(2049))
    # ~1000 m from the origin at 1 cm spacing: the expanded form's |a|^2 ~ 3e6 has a float32 step
    # of 0.25 m^2, the difference form is accurate
    rng = _rng(6)
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(1, -1, 3)
    r = (1000.0 + 0.01 * (g + 0.3 * rng.uniform(-1, 1, g.shape))).astype(F32)
    q = (1000.0 + 0.01 * rng.uniform(0, 7, (1, 65, 3))).astype(F32)
    out.append(KnnCase("knn_offset_1000m", q, r, KS, False))
    # 200 points within 1e-7 (relative) of one sphere: float32 d2 cannot order them
    v = rng.standard_normal((1, 200, 3))
    v = 10.0 * v / np.linalg.norm(v, axis=-1, keepdims=True) * (1 + 1e-7 * rng.uniform(-1, 1, (1, 200, 1)))
    out.append(KnnCase("knn_near_sphere", np.zeros((1, 1, 3), F32), v.astype(F32), KS, True))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def knn_case(name):
    return next(c for c in knn_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def knn_yard(name):
    """(dist, idx) of the float32 layer at k = 32: knn(k) is its first k columns (a prefix of one
    lexsort order, ranks >= n padded alike)"""
    cs = knn_case(name)
    return ref.knn(max(KS), cs.query, cs.ref)


@functools.lru_cache(maxsize=None)
def knn_yard64(name):
    cs = knn_case(name)
    return ref.knn64(max(KS), cs.query, cs.ref)


def knn_unclear(name):
    """(decisive pairs on which the two layers disagree, share of non-decisive pairs), k = 32"""
    return ref.check_decisive(knn_yard(name)[1], *knn_yard64(name))


# ------------------------------------------------------------------------------- gathers
def _indices(rng, b, n, shape):
    ix = rng.integers(0, n, (b,) + shape).astype(np.int32)
    flat = ix.reshape(b, -1)
    flat[:, 0] = 0
    flat[:, -1] = n - 1
    return ix


@functools.lru_cache(maxsize=None)
def gather_cases():
    """(b, c, n, index shape): g = 1500, 1025 * 3, 2057 are no multiples of the 1024 threads;
    c b > 512 puts 2 or 3 channels into a work-group, which 35 and 130 are no multiples of"""
    out = []
    for b, c, n, shape in ((3, 3, 1, (5,)), (1, 3, STAGE - 1, (1500,)), (3, 1, STAGE, (1025, 3)),
                           (1, 3, STAGE + 1, (2057,)), (3, 35, 700, (77, 5)), (1, 130, 300, (1500,)),
                           (16, 35, 100, (1100,)), (8, 130, 50, (33, 4))):
        rng = _rng(8, b, c, n)
        out.append(GatherCase(f"gather_b{b}_c{c}_n{n}_g{'x'.join(map(str, shape))}",
                              rng.standard_normal((b, c, n)).astype(F32), _indices(rng, b, n, shape)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rel_cases():
    out = []
    for b, c, n, s, k in ((3, 0, 1, 5, 3), (1, 3, STAGE - 1, 300, 4), (1, 1, STAGE, 257, 5), (3, 35, 700, 77, 16),
                          (16, 35, 100, 70, 9)):
        rng = _rng(9, b, c, n)
        out.append(RelCase(f"rel_b{b}_c{c}_n{n}_s{s}_k{k}", _noise(rng, b, n).transpose(0, 2, 1).copy(),
                           _noise(rng, b, s).transpose(0, 2, 1).copy(),
                           rng.standard_normal((b, c, n)).astype(F32) if c else None, _indices(rng, b, n, (s, k))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def interp_cases():
    out = []
    for b, c, m, n in ((3, 3, 1, 5), (1, 3, STAGE - 1, 1500), (3, 1, STAGE, 1025), (1, 3, STAGE + 1, 2057),
                       (3, 35, 700, 65), (16, 35, 100, 1100), (8, 130, 50, 33)):
        rng = _rng(10, b, c, m)
        w = rng.uniform(0, 1, (b, n, 3))
        out.append(InterpCase(f"interp_b{b}_c{c}_m{m}_n{n}", rng.standard_normal((b, c, m)).astype(F32),
                              _indices(rng, b, m, (n, 3)), (w / w.sum(-1, keepdims=True)).astype(F32)))
    return tuple(out)


BAD_INDICES = (-1, "n")                         # "n": the first index past the row


def with_bad(idx, n, which):
    """a copy of idx with one element (not the first, not the last) replaced"""
    bad = idx.copy()
    flat = bad.reshape(bad.shape[0], -1)
    at = (bad.shape[0] - 1, flat.shape[1] // 2)
    flat[at] = n if which == "n" else which
    return bad, at


# ------------------------------------------------------------------------------- upsample
@functools.lru_cache(maxsize=None)
def up_cases():
    """(b, n, s, c).  Coincident dense / sparse points (d = 0: the 1e-10 clamp), flows of +-100
    exactly on them, and flows wide enough (sigma 120) that sums cross +-100."""
    out = []
    for b, n, s, c in ((1, 1, 1, 1), (3, 63, 2, 3), (1, 64, 4095, 3), (3, 65, 4096, 1), (1, 65, 300, 0),
                       (512, 5, 2, 3), (512, 3, 37, 1), (512, 1, 4096, 1)):
        rng = _rng(11, b, n, s)
        xyz = _noise(rng, b, n).transpose(0, 2, 1).copy()
        sxyz = _noise(rng, b, s).transpose(0, 2, 1).copy()
        m = min(2, n, s)
        sxyz[:, :, :m] = xyz[:, :, :m]
        sf = (rng.standard_normal((b, c, s)) * 120).astype(F32)
        sf[:, :, :m] = np.array([100.0, -100.0], F32)[:m]
        out.append(UpCase(f"up_b{b}_n{n}_s{s}_c{c}", xyz, sxyz, sf, UP_KS))
    return tuple(out)


def up_case(name):
    return next(c for c in up_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def up_nbr(name):
    cs = up_case(name)
    return ref.neighbours(np.ascontiguousarray(cs.xyz.transpose(0, 2, 1)),
                          np.ascontiguousarray(cs.sxyz.transpose(0, 2, 1)), max(UP_KS))


@functools.lru_cache(maxsize=None)
def up_yard(name, k):
    """(float32 value, float64 value, bound) at k"""
    cs = up_case(name)
    y, idx = ref.upsample_flow(cs.xyz, cs.sxyz, cs.sfeat, k, nbr=up_nbr(name))
    y64, bound = ref.upsample_flow64(cs.xyz, cs.sxyz, cs.sfeat, idx)
    return y, y64, bound


def up_unclear(name):
    cs = up_case(name)
    i64, gap = ref.knn64(max(UP_KS), np.ascontiguousarray(cs.xyz.transpose(0, 2, 1)),
                         np.ascontiguousarray(cs.sxyz.transpose(0, 2, 1)))
    i32 = ref.knn(max(UP_KS), None, None, nbr=up_nbr(name))[1]
    return ref.check_decisive(i32, i64, gap)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def worst_ratio(got, y64, bound):
    """max of |got - y64| / bound: <= 1 meets the bar"""
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got.astype(np.float64) - y64) / bound))


# ------------------------------------------------------------------------------- admission
def _admit():
    """the yardstick itself meets the cap on every seeded case, and never contradicts its
    float64 layer on a decisive pair"""
    for cs in knn_cases():
        if not cs.exact:
            wrong, unclear = knn_unclear(cs.name)
            assert wrong == 0 and unclear <= MAX_UNCLEAR, (cs.name, wrong, unclear)
    for cs in up_cases():
        wrong, unclear = up_unclear(cs.name)
        assert wrong == 0 and unclear <= MAX_UNCLEAR, (cs.name, wrong, unclear)


_admit()

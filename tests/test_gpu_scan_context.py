"""The Scan Context loop detector on the GPU (scan_context.hip, ssf.scan_context, LoopCloser with
detector="scan_context") against tests/scan_context_reference.py, the numpy
yardstick written from the definitions alone (float64 geometry, float64 distance).

Bars:
  descriptor  bit for bit on clouds whose points all lie at least 1e-3 m from a ring edge and 1e-3
              rad from a sector edge by the yardstick's float64 report (about 1000 x the float32
              error of sqrt / atan2 at these magnitudes, so every point's bin is decided); on clouds
              with points exactly on edges, between the descriptor without them and the one with
              each of them in both bins it borders.
  distance    |dist - yardstick| <= 1e-5: a cosine is a dot product of two unit 20-vectors in
              float32 (about 24 * 2^-24 = 1.4e-6), the mean over at most 60 columns and the
              normalisations keep the total under 6e-6.  shift: any s whose yardstick d(s) is
              within 2e-5 of the minimum; the best candidate: any whose yardstick distance is
              within 2e-5 of the best.
  and bit for bit between runs, between batch shapes and between the database and one call."""
import ctypes as C

import numpy as np
import pytest
import torch

import scan_context_reference as SR

pytestmark = pytest.mark.gpu

DIST_TOL, TIE_TOL = 1e-5, 2e-5


@pytest.fixture(scope="module")
def fe(dev):
    from ssf import Frontend
    return Frontend(64, device=dev.index or 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------ descriptor
def _clean_cloud(rng, n, stride, max_range=SR.MAX_RANGE):
    """n random points (a few more are drawn, the ones near an edge dropped): ranges beyond
    max_range, heights below -lidar_height, every one 1e-3 clear of the bin edges."""
    m = n + n // 8 + 8
    r = rng.uniform(0.01, 1.1 * max_range, m)
    phi = rng.uniform(0, 2 * np.pi, m)
    cols = [r * np.cos(phi), r * np.sin(phi), rng.uniform(-4.0, 10.0, m)]
    if stride == 4:
        cols.append(rng.uniform(0, 64, m))
    pts = np.stack(cols, -1).astype(np.float32)
    _, _, _, rm, sm = SR.bins(pts, max_range)
    pts = pts[(rm >= 1e-3) & (sm >= 1e-3)][:n]
    assert len(pts) == n
    return pts


def _describe_raw(fe, dev, clouds, stride, params):
    """ssf_scan_context_batch into the middle of a sentinel-filled buffer -> desc [F, 20, 60]."""
    import ssf
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    F = len(clouds)
    flat = np.concatenate(clouds) if F else np.zeros((0, stride), np.float32)
    pts = torch.from_numpy(np.ascontiguousarray(flat.reshape(-1, stride))).to(dev)
    off, h_off = ssf.frame_offsets([len(c) for c in clouds], dev)
    buf = torch.full(((F + 2) * 1200,), -7.0, dtype=torch.float32, device=dev)
    rc = _abi.lib().ssf_scan_context_batch(fe._h, _stream(dev), F, _ptr(pts), stride, _ptr(off),
                                           C.c_void_p(h_off.data_ptr()), C.byref(params),
                                           C.c_void_p(buf.data_ptr() + 4 * 1200))
    assert rc == _abi.SSF_OK, _abi.lib().ssf_last_error(fe._h)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:1200] == -7.0).all() and (out[(F + 1) * 1200:] == -7.0).all(), "sentinels overwritten"
    return out[1200:(F + 1) * 1200].reshape(F, 20, 60), pts, off, h_off


@pytest.mark.parametrize("stride", [3, 4])
def test_descriptor_bit_for_bit_on_clean_clouds(fe, dev, stride):
    from ssf import scan_context as sc
    rng = np.random.default_rng(40 + stride)
    clouds = [_clean_cloud(rng, n, stride) for n in (5000, 0, 1, 777, 1025)]
    bad = _clean_cloud(rng, 600, stride)                   # non-finite coordinates, each alone and together
    bad[0:40, 0], bad[40:80, 1], bad[80:120, 2] = np.nan, np.inf, -np.inf
    bad[120:140, :3] = np.nan
    bad[140:160, 2] = 1e30                                 # finite and huge: kept
    clouds.append(bad)
    clouds.append(np.full((50, stride), np.nan, np.float32))   # nothing survives: all zero
    low = _clean_cloud(rng, 300, stride)
    low[:, 2] = -np.abs(low[:, 2]) - 2.0                   # every height at or below 0: all zero
    clouds.append(low)
    params = sc.sc_params()
    got, pts, off, h_off = _describe_raw(fe, dev, clouds, stride, params)
    want = SR.describe_batch(np.concatenate(clouds), [len(c) for c in clouds])
    for k in range(len(clouds)):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, np.abs(got[k] - want[k]).max())
    assert not got[1].any() and not got[6].any() and not got[7].any() and np.count_nonzero(got[2]) <= 1
    assert want[0].any() and (want[5] == np.float32(1e30)).any()
    # the Python entry point is the same call
    assert np.array_equal(_bits(sc.describe(fe, pts, off, h_off).cpu().numpy()), _bits(got))
    assert np.array_equal(_bits(sc.describe_one(fe, pts[:5000]).cpu().numpy()), _bits(got[0]))
    # other parameters: the ring width is max_range / 20, the heights move with lidar_height
    p2 = sc.sc_params(max_range=50.0, lidar_height=1.5)
    c2 = [_clean_cloud(rng, 3000, stride, 50.0), _clean_cloud(rng, 33, stride, 50.0)]
    got2 = _describe_raw(fe, dev, c2, stride, p2)[0]
    want2 = SR.describe_batch(np.concatenate(c2), [len(c) for c in c2], 50.0, 1.5)
    assert np.array_equal(_bits(got2), _bits(want2))


def test_descriptor_200k_points(fe, dev):
    from ssf import scan_context as sc
    rng = np.random.default_rng(7)
    big = _clean_cloud(rng, 200_000, 4)
    got = _describe_raw(fe, dev, [big[:3], big], 4, sc.sc_params())[0]
    assert np.array_equal(_bits(got[1]), _bits(SR.describe(big)))
    assert np.array_equal(_bits(got[0]), _bits(SR.describe(big[:3])))
    assert np.count_nonzero(got[1]) > 1100


def test_descriptor_on_edge_clouds(fe, dev):
    """Points exactly on ring edges, on sector edges (k * 6 degrees, 0 and the wrap included) and
    at r = max_range may fall on either side: lower <= desc <= upper elementwise."""
    from ssf import scan_context as sc
    rng = np.random.default_rng(11)
    base = _clean_cloud(rng, 4000, 3)
    base[:, 2] = rng.uniform(-3.0, 4.0, len(base)).astype(np.float32)
    lower = SR.describe(base)
    upper = lower.copy()
    edge = []

    def put(r, phi, z, bins_):
        x, y = r * np.cos(phi), r * np.sin(phi)
        edge.append([x, y, z])
        for ring, sector in bins_:
            upper[ring, sector] = max(upper[ring, sector], np.float32(np.float32(z) + np.float32(2.0)))

    w, a = SR.MAX_RANGE / SR.RINGS, SR.SECTOR_ANGLE
    for k in range(1, 20):                                 # ring edges, mid-sector
        for s in (0, 17, 42, 59):
            put(k * w, (s + 0.5) * a, 6.0 + 0.01 * k, [(k - 1, s), (k, s)])
    for s in (3, 31):                                      # r = max_range: ring 19 or skipped
        put(SR.MAX_RANGE, (s + 0.5) * a, 7.0, [(19, s)])
    for m in range(60):                                    # sector edges, mid-ring
        for ring in (0, 9, 19):
            put((ring + 0.5) * w, m * a, 6.5 + 0.01 * m, [(ring, (m - 1) % 60), (ring, m)])
    edge = np.array(edge, np.float32)
    edge = np.concatenate([edge, [[10.0, -0.0, 8.0], [10.0, 0.0, 8.0], [-10.0, 0.0, 8.5], [-10.0, -0.0, 8.5],
                                  [0.0, 10.0, 8.5], [0.0, -10.0, 8.5]]]).astype(np.float32)
    for ring, s in ((2, 59), (2, 0), (2, 29), (2, 30), (2, 14), (2, 15), (2, 44), (2, 45)):
        hgt = 10.0 if s in (59, 0) else 10.5
        upper[ring, s] = max(upper[ring, s], np.float32(hgt))
    _, _, _, rm, sm = SR.bins(edge)
    assert (np.minimum(rm, sm) < 1e-4).all()               # they are edge points by the yardstick's report
    cloud = np.concatenate([base, edge])[rng.permutation(len(base) + len(edge))]
    got = _describe_raw(fe, dev, [cloud], 3, sc.sc_params())[0][0]
    assert (lower <= got).all() and (got <= upper).all(), (np.argwhere(got < lower), np.argwhere(got > upper))
    assert (upper > lower).sum() > 200 and (got > lower).sum() > 60        # the edge points do land


# ------------------------------------------------------------------------------ distance
def _random_descs(rng, n):
    """A mix: dense-ish random descriptors with empty columns, single-ring columns, sparse ones."""
    d = (rng.uniform(0.0, 5.0, (n, 20, 60)) * (rng.random((n, 20, 60)) < 0.4)).astype(np.float32)
    for k in range(n):
        d[k][:, rng.random(60) < 0.2] = 0                  # empty columns
        if k % 3 == 1:                                     # single-ring columns
            one = np.zeros((20, 60), np.float32)
            one[rng.integers(0, 20, 60), np.arange(60)] = rng.uniform(0.1, 9.0, 60)
            one[:, rng.random(60) < 0.3] = 0
            d[k] = one
    return d


@pytest.fixture(scope="module")
def scan_descs():
    """Yardstick descriptors of 8 synthetic scans and of their copies rotated by 0, 42 and 93
    degrees (the sensor yawed: the points turn the other way)."""
    from ssf import synth
    sc = synth.Scene(0)
    scans = [synth.scan(0, 3 * k, n_az=300, scene=sc)["pos1"].numpy() for k in range(8)]
    db = np.stack([SR.describe(s) for s in scans])
    yaws = (0.0, 42.0, 93.0)
    q = np.stack([SR.describe(SR.rot_z(s, -y)) for s in scans for y in yaws])
    return db, q, yaws


def _match_full(fe, dev, q, db, n_el):
    from ssf import scan_context as sc
    out = sc.match(fe, torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev), n_el, full=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check_match(got, q, db, n_el):
    idx, bdist, bshift, dist, shift = got
    rd, _, dall = SR.match(q, db)
    Q, N = len(q), len(db)
    n_el = np.broadcast_to(np.asarray(n_el), (Q,))
    assert dist.shape == (Q, N) and shift.shape == (Q, N)
    if N:
        err = np.abs(dist.astype(np.float64) - rd)
        print(f"[scan context] Q {Q} N {N}: max |dist - yardstick| {err.max():.3g}")
        assert err.max() <= DIST_TOL, err.max()
        assert shift.min() >= 0 and shift.max() < 60
        at = np.take_along_axis(dall, shift[:, :, None].astype(np.int64), axis=2)[:, :, 0]
        assert (at <= rd + TIE_TOL).all(), (at - rd).max()
    for a in range(Q):
        n = int(n_el[a])
        if n == 0:
            assert idx[a] == -1 and bdist[a] == 1.0 and bshift[a] == 0
            continue
        assert 0 <= idx[a] < n
        assert rd[a, idx[a]] <= rd[a, :n].min() + TIE_TOL, (a, idx[a], rd[a, idx[a]], rd[a, :n].min())
        # the device's own order: the smallest (dist, index) of its own row
        assert idx[a] == SR.select(dist[a], n)
        assert _bits(bdist[a]) == _bits(dist[a, idx[a]]) and bshift[a] == shift[a, idx[a]]


@pytest.mark.parametrize("N", [1, 3, 4, 5, 63, 64, 65, 257])
def test_distance_against_yardstick(fe, dev, N, scan_descs):
    """Every wave and work-group remainder of the match kernel (4 candidates per pass, 16 per
    work-group); an all-zero query and an all-zero candidate among them, up to 8 synthetic scans
    in the database and their rotated copies among the queries."""
    rng = np.random.default_rng(100 + N)
    db = _random_descs(rng, N)
    ns = min(N // 2, 8)
    db[:ns] = scan_descs[0][:ns]
    if N >= 3:
        db[N // 2] = 0
    q = _random_descs(rng, 4)
    q[2] = 0
    q[3] = db[N - 1]                                       # a stored descriptor asks for itself
    q = np.concatenate([q, scan_descs[1]])
    got = _match_full(fe, dev, q, db, N)
    _check_match(got, q, db, N)
    assert got[0][3] == (N - 1 if np.any(db[N - 1]) else 0) or SR.match(q[3:], db)[0][0, got[0][3]] <= TIE_TOL
    assert (got[3][2] == 1.0).all() and (got[4][2] == 0).all()          # the all-zero query: distance 1 everywhere
    if N >= 3:
        assert (got[3][:, N // 2] == 1.0).all()
    # a single-ring column against itself is exactly 1: a descriptor of such columns is at 0 from itself
    one = _random_descs(rng, 2)[1:2]
    g = _match_full(fe, dev, one, one, 1)
    assert g[1][0] == 0.0 and g[2][0] == 0 and g[0][0] == 0


def test_distance_on_rotated_scans(fe, dev, scan_descs):
    db, q, yaws = scan_descs
    got = _match_full(fe, dev, q, db, len(db))
    _check_match(got, q, db, len(db))
    idx, bdist, bshift = got[:3]
    for k in range(8):
        for j, yaw in enumerate(yaws):
            a = 3 * k + j
            assert idx[a] == k, (k, yaw, idx[a], bdist[a])           # its own frame ranks first
            want = yaw / 6.0
            assert min(abs(bshift[a] - np.floor(want)), abs(bshift[a] - np.ceil(want))) == 0, (yaw, bshift[a])
            if yaw % 6.0 == 0.0:                        # whole sectors: the columns move, nothing else
                assert bshift[a] == int(want) and bdist[a] < 0.01


def test_eligible_counts_and_selection_only(fe, dev):
    from ssf import scan_context as sc
    rng = np.random.default_rng(21)
    db = _random_descs(rng, 37)
    q = _random_descs(rng, 3)
    db[5] = q[0]
    dq, ddb = torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev)
    for n_el in (0, 1, 37, [0, 1, 37], [6, 5, 20]):
        got = _match_full(fe, dev, q, db, n_el)
        _check_match(got, q, db, n_el)
        sel = [t.cpu().numpy() for t in sc.match(fe, dq, ddb, n_el)]   # d_dist and d_shift null
        assert np.array_equal(sel[0], got[0]) and np.array_equal(_bits(sel[1]), _bits(got[1]))
        assert np.array_equal(sel[2], got[2])
    assert _match_full(fe, dev, q, db, [6, 5, 20])[0][0] == 5 and _match_full(fe, dev, q, db, [5, 5, 5])[0][0] != 5
    # ties in (dist, index): equal candidates, the first wins
    db[9] = db[2]
    db[30] = db[2]
    got = _match_full(fe, dev, db[2:3], db, 37)
    assert got[0][0] == 2 and _bits(got[3][0, 2]) == _bits(got[3][0, 9]) == _bits(got[3][0, 30])
    # an empty database: every query gets -1
    got = _match_full(fe, dev, q, db[:0], 0)
    assert (got[0] == -1).all() and got[3].shape == (3, 0)


def test_batch_shape_and_run_to_run_bits(fe, dev):
    """A pair's dist and shift are the same bits whatever else is in the call, and on every run."""
    rng = np.random.default_rng(33)
    db = _random_descs(rng, 70)
    q = _random_descs(rng, 3)
    a = _match_full(fe, dev, q, db, [70, 33, 1])
    b = _match_full(fe, dev, q, db, [70, 33, 1])
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for k, n in enumerate([70, 33, 1]):
        one = _match_full(fe, dev, q[k:k + 1], db, n)
        for x, y in zip(a, one):
            assert np.array_equal(x[k:k + 1].view(np.uint32), y.view(np.uint32)), k
    part = _match_full(fe, dev, q, db[:21], 21)              # a shorter database: the same pairs
    assert np.array_equal(part[3].view(np.uint32), a[3][:, :21].view(np.uint32))
    assert np.array_equal(part[4], a[4][:, :21])


def test_argument_errors(fe, dev):
    """SSF_E_ARG, and nothing written: the outputs keep their sentinels."""
    from ssf import _abi, scan_context as sc
    from ssf.frontend import _ptr, _stream
    L = _abi.lib()
    pts = torch.zeros(8, 3, device=dev)
    h = torch.tensor([0, 3, 8], dtype=torch.int64)
    off = h.to(dev)
    desc = torch.full((2, 20, 60), -7.0, device=dev)
    p = sc.sc_params()
    hp = C.c_void_p(h.data_ptr())
    st = _stream(dev)

    def describe(n=2, pts_=pts, stride=3, off_=off, h_=hp, prm=p, out=desc):
        return L.ssf_scan_context_batch(fe._h, st, n, _ptr(pts_), stride, _ptr(off_), h_,
                                        None if prm is None else C.byref(prm), _ptr(out))
    assert describe() == _abi.SSF_OK
    desc.fill_(-7.0)
    bad_h = torch.tensor([0, 5, 3], dtype=torch.int64)
    neg_h = torch.tensor([-1, 3, 8], dtype=torch.int64)
    zero_range, nan_h = sc.sc_params(), sc.sc_params()
    zero_range.max_range, nan_h.lidar_height = 0.0, float("nan")
    neg_range = sc.sc_params()
    neg_range.max_range = -80.0
    for kw in (dict(n=-1), dict(stride=2), dict(stride=5), dict(pts_=None), dict(off_=None), dict(h_=None),
               dict(prm=None), dict(out=None), dict(h_=C.c_void_p(bad_h.data_ptr())),
               dict(h_=C.c_void_p(neg_h.data_ptr())), dict(prm=zero_range), dict(prm=neg_range), dict(prm=nan_h)):
        assert describe(**kw) == _abi.SSF_E_ARG, kw
    assert describe(n=0, pts_=None, off_=None, h_=None, out=None) == _abi.SSF_OK
    torch.cuda.synchronize()
    assert (desc == -7.0).all()

    q = torch.zeros(2, 20, 60, device=dev)
    db = torch.zeros(5, 20, 60, device=dev)
    h_ne = torch.tensor([5, 2], dtype=torch.int32)
    d_ne = h_ne.to(dev)
    best = torch.full((2, 4), -7, dtype=torch.int32, device=dev)
    dist = torch.full((2, 5), -7.0, device=dev)
    shift = torch.full((2, 5), -7, dtype=torch.int32, device=dev)
    hn = C.c_void_p(h_ne.data_ptr())

    def match(nq=2, q_=q, n=5, db_=db, dn=d_ne, hn_=hn, di=dist, sh=shift, be=best):
        return L.ssf_scan_context_match(fe._h, st, nq, _ptr(q_), n, _ptr(db_), _ptr(dn), hn_, _ptr(di), _ptr(sh),
                                        _ptr(be))
    over = torch.tensor([5, 6], dtype=torch.int32)
    under = torch.tensor([-1, 2], dtype=torch.int32)
    for kw in (dict(nq=-1), dict(n=-1), dict(q_=None), dict(db_=None), dict(dn=None), dict(hn_=None), dict(be=None),
               dict(di=None), dict(sh=None), dict(hn_=C.c_void_p(over.data_ptr())),
               dict(hn_=C.c_void_p(under.data_ptr())), dict(n=4)):
        assert match(**kw) == _abi.SSF_E_ARG, kw
    assert match(nq=0, q_=None, dn=None, hn_=None, be=None) == _abi.SSF_OK
    torch.cuda.synchronize()
    assert (best == -7).all() and (dist == -7.0).all() and (shift == -7).all()
    assert b"scan_context_match" in L.ssf_last_error(fe._h)
    assert match() == _abi.SSF_OK
    torch.cuda.synchronize()
    assert (dist == 1.0).all() and best[:, 0].tolist() == [0, 0]
    with pytest.raises(ValueError):
        sc.match(fe, q, db, [1, 2, 3])
    with pytest.raises(ValueError):
        sc.match(fe, q, db, 6)
    with pytest.raises(_abi.SSFError):
        sc.match(fe, q.cpu(), db, 1)


# ------------------------------------------------------------------------------ database
def test_database_growth_equals_one_match(fe, dev):
    from ssf import scan_context as sc
    rng = np.random.default_rng(55)
    d = torch.from_numpy(_random_descs(rng, 11)).to(dev)
    q = torch.from_numpy(_random_descs(rng, 2)).to(dev)
    db = sc.ScanContextDB(fe, capacity=2)
    assert len(db) == 0 and db.query(q[0]) == (-1, 1.0, 0)
    for k in range(9):                                     # 2 -> 4 -> 8 -> 16
        assert db.append(d[k]) == k
    assert db.append(d[9:11]) == 9
    assert len(db) == 11 and db.capacity == 16 and db.generation == 3
    assert np.array_equal(_bits(db.descriptors().cpu().numpy()), _bits(d.cpu().numpy()))
    for n_el in (11, 6, 1, 0):
        want = [t.cpu().numpy() for t in sc.match(fe, q, d, n_el)]
        got = [t.cpu().numpy() for t in db.query(q, n_el)]
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), n_el
        i, dist, s = db.query(q[1], n_el)
        assert (i, s) == (int(want[0][1]), int(want[2][1])) and _bits(np.float32(dist)) == _bits(want[1][1])
    assert db.query(q[0]) == db.query(q[0], 11)


# ------------------------------------------------------------------------------ end to end
DRIFT = 40.0          # metres, along y: the forward path runs along x (0 .. 29 m, |y| < 1 m)
THRESHOLD = 0.2


@pytest.fixture(scope="module")
def revisit_frames():
    """The scene of test_loop_closer_detects_revisit (30 frames forward, then frames 0..5 again,
    stamped 30 s later), n_az = 600 -> per step (k, revisit, scan, planes, scan turned by 180
    degrees, its planes, T)."""
    from ssf import synth
    from oracle import oracle as O
    sc = synth.Scene(0)
    R0, p0 = synth.ego_pose(0, 0)
    T0 = np.eye(4); T0[:3, :3] = R0.numpy(); T0[:3, 3] = p0.numpy()
    frames = {}
    for k in range(30):
        pos = synth.scan(0, k, n_az=600, scene=sc)["pos1"].numpy()
        R, p = synth.ego_pose(0, k)
        Tk = np.eye(4); Tk[:3, :3] = R.numpy(); Tk[:3, 3] = p.numpy()
        f = dict(scan=pos, planes=O.extract_planes(pos, 64), T=np.linalg.inv(T0) @ Tk)
        if k < 6:
            f["scan_turned"] = SR.rot_z(pos, 180.0)
            f["planes_turned"] = O.extract_planes(f["scan_turned"], 64)
        frames[k] = f
    return frames


def _drive(fe, dev, frames, turned, drift_xy, **kw):
    """-> (closer, constraints, keyframes as (k, revisit), keyframes before the revisit)"""
    from ssf import loop
    lc = loop.LoopCloser(fe, **kw)
    with_scan = kw.get("detector") == "scan_context"
    cons, keys, n_fwd = [], [], None
    for i, k in enumerate(list(range(30)) + list(range(6))):
        f = frames[k]
        revisit = i >= 30
        if revisit and n_fwd is None:
            n_fwd = len(lc.key6d)
        T = f["T"].copy()
        use_turned = revisit and turned
        if use_turned:                                      # the sensor yawed by 180 degrees: so is the odometry
            T = T @ loop.get_transformation(0, 0, 0, 0, 0, np.pi)
        if revisit:
            T[0, 3] += drift_xy[0]
            T[1, 3] += drift_xy[1]
        yaw = np.arctan2(T[1, 0], T[0, 0])
        q = (0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2))
        pl = torch.from_numpy(f["planes_turned" if use_turned else "planes"]).to(dev)
        args = (pl, q, T[:3, 3], 0.1 * i + (30.0 if revisit else 0.0))
        if with_scan:
            scan = torch.from_numpy(f["scan_turned" if use_turned else "scan"]).to(dev)
            _, c, is_key = lc.process(*args, scan=scan)
        else:
            _, c, is_key = lc.process(*args)
        if is_key:
            keys.append((k, revisit))
        if c is not None:
            cons.append(c)
    return lc, cons, keys, n_fwd


def test_revisit_beyond_the_radius_is_closed_by_scan_context(fe, dev, revisit_frames):
    """Why the detector exists: the revisit of test_loop_closer_detects_revisit, now with a 40 m
    odometry drift (beyond the 15 m radius) and the sensor yawed by 180 degrees (the scan is turned
    before the planes are extracted, the odometry yaw with it).  The radius search closes no
    loop; the Scan Context search closes one, at the right place, with the right yaw, and its
    correction removes the drift.

    threshold = 0.2, chosen on the CPU with the yardstick at n_az = 600 over frames 0..29: the
    largest best-candidate distance of the six revisits is 0.122 when only every second forward
    frame is a candidate (0.000 over the keyframes this sequence really keeps: frames 0, 2, 4 and
    5 are keyframes both times, and a scan turned by whole sectors has the same columns), the
    smallest distance from a revisit to any frame more than 5 m from its true position is 0.311.
    The default 0.13 is not asserted here."""
    from ssf import scan_context as sc
    frames = revisit_frames
    _, cons, _, _ = _drive(fe, dev, frames, True, (0.0, DRIFT), detector="radius")
    assert cons == [], "the inputs must defeat the radius search"

    lc, cons, keys, n_fwd = _drive(fe, dev, frames, True, (0.0, DRIFT), detector="scan_context",
                                   sc=sc.sc_params(threshold=THRESHOLD))
    assert len(cons) == 1, [(c.key_cur, c.key_pre, c.dist) for c in cons]
    c = cons[0]
    assert len(lc.sc_db) == len(lc.key6d) == len(keys)
    assert c.key_pre < n_fwd <= c.key_cur and keys[c.key_cur][1] and not keys[c.key_pre][1]
    true_cur, true_pre = frames[keys[c.key_cur][0]]["T"][:3, 3], frames[keys[c.key_pre][0]]["T"][:3, 3]
    print(f"[scan context] loop {c.key_cur} -> {c.key_pre} (frames {keys[c.key_cur][0]} -> {keys[c.key_pre][0]}), "
          f"dist {c.dist:.4f}, shift {c.shift}, noise {c.noise:.4g}, correction t {c.correction[:3, 3]}")
    assert np.linalg.norm(true_cur - true_pre) < 5.0
    assert c.dist < THRESHOLD and abs(c.shift - 30) <= 1
    assert abs(c.correction[1, 3] + DRIFT) < 0.1 and abs(c.correction[0, 3]) < 0.1, c.correction
    assert abs(c.correction[2, 3]) < 0.1 and np.abs(c.correction[:3, :3] - np.eye(3)).max() < 1e-2
    assert c.noise < 0.2

    # optimize=True: the pose graph is solved at the closure and the key poses that follow are
    # corrected; the last one is asserted.  The closing keyframe itself is printed, not asserted: the
    # whole 40 m sit in one odometry edge of variance 1e-4 m^2, which the solve honours (13.6 m left)
    lo, cons_o, keys_o, _ = _drive(fe, dev, frames, True, (0.0, DRIFT), detector="scan_context",
                                   sc=sc.sc_params(threshold=THRESHOLD), optimize=True)
    assert len(cons_o) == 1 and lo.last_optimization is not None and lo.last_optimization["loops"] == 1
    assert keys_o[-1][1] and len(keys_o) - 1 > cons_o[0].key_cur        # a keyframe after the closing one
    truth = frames[keys_o[-1][0]]["T"][:3, 3]
    err = np.linalg.norm(np.array(lo.key6d[-1][:3]) - truth)
    closing = np.linalg.norm(np.array(lo.key6d[cons_o[0].key_cur][:3]) - frames[keys_o[cons_o[0].key_cur][0]]["T"][:3, 3])
    print(f"[scan context] optimize: last key pose {err:.4f} m from the truth, the closing keyframe {closing:.4f} m")
    assert err < 0.2, err


def test_run_sequence_and_cli_with_scan_context(dev, tmp_path, capsys):
    """An out-and-back drive through the onlyPC node graph with map_detector="scan_context":
    mapOptmization takes /velodyne_points, pairs each scan with its plane cloud and closes a loop
    on the way back (the same scans replayed, so at shift 0); python -m ssf.run does the same and
    its JSON line names the detector."""
    import json
    from ssf import nodes, run, synth
    sc = synth.Scene(0)
    order = list(range(30)) + list(range(28, 18, -1))
    scans = {k: synth.scan(0, k, n_az=600, scene=sc) for k in set(order)}
    data = tmp_path / "data"
    data.mkdir()
    for i, k in enumerate(order):
        np.savez(str(data / f"{i:06d}.npz"), pos1=scans[k]["pos1"].numpy(), gt=scans[k]["flow"].numpy())
    with torch.cuda.device(dev):
        res = nodes.run_sequence(str(data), None, launch="onlyPC", map_tum_path=str(tmp_path / "map.txt"),
                                 rate_hz=0.5, map_detector="scan_context", map_sc_threshold=THRESHOLD)
        assert len(res["loops"]) >= 1
        c = res["loops"][0]
        print(f"[scan context] run_sequence: loop {c.key_cur} -> {c.key_pre}, dist {c.dist:.4f}, shift {c.shift}")
        assert c.dist < THRESHOLD and c.shift in (0, 1, 59) and c.noise < 0.2
        assert np.linalg.norm(c.between[:3, 3]) < 5.0        # the two keyframes are neighbours in space
        assert len(open(tmp_path / "map.txt").read().splitlines()) >= len(order) - 1
        capsys.readouterr()
        run.main([str(data), "--launch", "onlyPC", "--map-tum", str(tmp_path / "cli.txt"), "--rate-hz", "0.5",
                  "--map-detector", f"scan-context:{THRESHOLD}", "--device", str(dev.index or 0)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    md = line["map_detector"]
    assert md["detector"] == "scan_context" and md["threshold"] == THRESHOLD
    assert md["loops_closed"] == line["loops"] == len(res["loops"])
    assert (md["matches"][0]["key_cur"], md["matches"][0]["key_pre"], md["matches"][0]["shift"]) == \
        (c.key_cur, c.key_pre, c.shift)


def test_default_detector_is_untouched(fe, dev, revisit_frames):
    """LoopCloser() and LoopCloser(detector="radius", sc=None) with scan=None give identical
    constraints on the revisit sequence of test_loop_closer_detects_revisit (0.5 m drift)."""
    from ssf import loop
    a = _drive(fe, dev, revisit_frames, False, (0.5, 0.0))
    b = _drive(fe, dev, revisit_frames, False, (0.5, 0.0), detector="radius", sc=None)
    assert a[1] and len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert (x.key_cur, x.key_pre, x.noise) == (y.key_cur, y.key_pre, y.noise)
        assert x.between.tobytes() == y.between.tobytes() and x.correction.tobytes() == y.correction.tobytes()
        assert x.shift is None and x.dist is None and y.shift is None
    assert a[0].key6d == b[0].key6d and a[0].sc_db is None and b[0].sc_db is None
    c = a[1][0]
    assert abs(c.correction[0, 3] + 0.5) < 0.1 and abs(c.correction[1, 3]) < 0.1 and c.noise < 0.2
    assert isinstance(a[0], loop.LoopCloser)

"""The top-K Scan Context selection and the batched candidate verification on the GPU
(k_sc_select_topk, ssf_scan_context_match_topk, ssf.scan_context.match_topk / query_topk,
LoopCloser(sc_candidates=...)).

Bars:
  selection   exact.  The yardstick tests/scan_context_topk_reference.py is applied to the dist and
              shift rows the same call returned (the rows are held to the float64 yardstick by
              tests/test_gpu_scan_context.py; against the device's own rows a near-tie is no coin
              toss): index, the bits of dist, shift.  Slot 0 is ``match``'s result bit for bit,
              selection-only mode is full mode bit for bit, and so are two runs and Q = 3 against
              three Q = 1 calls.
  local maps  bit for bit voxel_grid_one of tests/map_reference.py's map_points.
  end to end  the decoy scene of the issue: margins of 0.02 around threshold 0.2 asserted with the
              numpy yardstick first, the device's distances being within 1e-5 of it."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_reference as MR
import scan_context_reference as SR
import scan_context_topk_reference as TR
from test_gpu_scan_context import DRIFT, THRESHOLD, _drive, _random_descs, revisit_frames  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257]
KS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def fe(dev):
    from ssf import Frontend
    return Frontend(64, device=dev.index or 0)


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.int32 else a


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(_u32(x), _u32(y)) for x, y in zip(a, b))


def _topk(fe, dq, ddb, n_el, k, E, full=False):
    from ssf import scan_context as sc
    out = sc.match_topk(fe, dq, ddb, n_el, k, E, full=full)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check_selection(fe, dev, q, db, n_els, windows=(0, 1, 5, None)):
    """(a) full mode against the yardstick on the call's own rows, (b) slot 0 against ``match``,
    (c) selection-only mode against full mode -- for every K, every window (None: N) and the
    per-query eligible counts n_els."""
    from ssf import scan_context as sc
    Q, N = len(q), len(db)
    dq, ddb = torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev)
    one = [t.cpu().numpy() for t in sc.match(fe, dq, ddb, n_els, full=True)]
    for k in KS:
        for E in windows:
            E = N if E is None else E
            idx, dist, shift, drow, srow = _topk(fe, dq, ddb, n_els, k, E, full=True)
            assert idx.shape == dist.shape == shift.shape == (Q, k) and drow.shape == srow.shape == (Q, N)
            assert _same((drow, srow), one[3:]), "the rows are the rows of ssf_scan_context_match"
            for a in range(Q):
                want = TR.select_topk(drow[a], srow[a], n_els[a], k, E)
                assert _same((idx[a], dist[a], shift[a]), want), (N, k, E, a, idx[a], want[0])
            assert _same((idx[:, 0], dist[:, 0], shift[:, 0]), one[:3]), (N, k, E)          # (b)
            assert _same(_topk(fe, dq, ddb, n_els, k, E), (idx, dist, shift)), (N, k, E)    # (c)
    return one


@pytest.mark.parametrize("N", SIZES)
def test_selection_is_exact(fe, dev, N):
    """The wave (64), the 16 candidates of a k_sc_match work-group and the 256 threads of the
    selection, each at, below and above; Q = 3 with n_eligible 0, 1 and N."""
    rng = np.random.default_rng(900 + N)
    db = _random_descs(rng, N)
    q = _random_descs(rng, 3)
    q[1] = db[N // 2]                                      # a stored descriptor asks for itself
    _check_selection(fe, dev, q, db, [N, 1, 0])
    _check_selection(fe, dev, q, db, [0, N, 1], windows=(0, 5))
    if N > 5:                                              # a prefix that ends inside the database
        _check_selection(fe, dev, q, db, [N - 1, N // 2, 5], windows=(1, None))


def test_selection_with_ties_zeros_and_nan(fe, dev):
    rng = np.random.default_rng(77)
    N = 70
    db = _random_descs(rng, N)
    for k in (3, 4, 20, 21, 40, 66, 69):                   # exact duplicates: equal distances, the lower index first
        db[k] = db[2]
    q = _random_descs(rng, 3)
    q[0] = db[2]
    one = _check_selection(fe, dev, q, db, [N, N, N])
    assert one[0][0] == 2 and len(set(_u32(one[3][0, [2, 3, 4, 20, 21, 40, 66, 69]]).tolist())) == 1
    idx = _topk(fe, torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev), N, 8, 0)[0]
    assert idx[0].tolist() == [2, 3, 4, 20, 21, 40, 66, 69]
    idx = _topk(fe, torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev), N, 8, 1)[0]
    assert idx[0].tolist()[:5] == [2, 4, 20, 40, 66]
    # all-zero queries and candidates: every distance is 1, the order is the index order
    z = np.zeros((3, 20, 60), np.float32)
    zdb = np.zeros((37, 20, 60), np.float32)
    one = _check_selection(fe, dev, z, zdb, [37, 1, 0])
    assert (one[3] == 1.0).all()
    idx = _topk(fe, torch.from_numpy(z).to(dev), torch.from_numpy(zdb).to(dev), 37, 3, 5)[0]
    assert idx[0].tolist() == [0, 6, 12]
    # a descriptor that contains NaN, as a candidate and as a query
    db2 = _random_descs(rng, 33)
    db2[7, 3, 11] = np.nan
    q2 = _random_descs(rng, 3)
    q2[2, 0, 0] = np.nan
    _check_selection(fe, dev, q2, db2, [33, 20, 33])


def test_batch_shape_and_run_to_run_bits(fe, dev):
    """(c) Q = 3 equals three Q = 1 calls and two runs are identical, in both modes."""
    rng = np.random.default_rng(34)
    db = _random_descs(rng, 70)
    q = _random_descs(rng, 3)
    dq, ddb = torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev)
    n_els = [70, 33, 1]
    for full in (False, True):
        a = _topk(fe, dq, ddb, n_els, 4, 2, full=full)
        assert _same(a, _topk(fe, dq, ddb, n_els, 4, 2, full=full))
        for j, n in enumerate(n_els):
            one = _topk(fe, dq[j:j + 1], ddb, n, 4, 2, full=full)
            assert _same([x[j:j + 1] for x in a], one), (full, j)


def test_argument_errors_and_sentinels(fe, dev):
    """(d) every SSF_E_ARG path leaves sentinel-filled outputs untouched; a valid call writes
    its [n_query * k] records and nothing around them; unfilled slots are (-1, 1.0, 0)."""
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    L = _abi.lib()
    st = _stream(dev)
    rng = np.random.default_rng(8)
    q = torch.from_numpy(_random_descs(rng, 2)).to(dev)
    db = torch.from_numpy(_random_descs(rng, 5)).to(dev)
    h_ne = torch.tensor([5, 2], dtype=torch.int32)
    d_ne = h_ne.to(dev)
    hn = C.c_void_p(h_ne.data_ptr())
    PAD = 16
    buf = torch.full((2 * 8 + 2 * PAD, 4), -7, dtype=torch.int32, device=dev)
    best = C.c_void_p(buf.data_ptr() + 16 * PAD)
    dist = torch.full((2, 5), -7.0, device=dev)
    shift = torch.full((2, 5), -7, dtype=torch.int32, device=dev)

    def call(nq=2, q_=q, n=5, db_=db, dn=d_ne, hn_=hn, di=dist, sh=shift, be=best, k=3, e=0):
        return L.ssf_scan_context_match_topk(fe._h, st, nq, _ptr(q_), n, _ptr(db_), _ptr(dn), hn_, _ptr(di),
                                             _ptr(sh), be, k, e)
    over = torch.tensor([5, 6], dtype=torch.int32)
    under = torch.tensor([-1, 2], dtype=torch.int32)
    for kw in (dict(k=0), dict(k=-1), dict(k=9), dict(k=2 ** 31 - 1), dict(e=-1), dict(e=-2 ** 31),
               dict(nq=-1), dict(n=-1), dict(q_=None), dict(db_=None), dict(dn=None), dict(hn_=None), dict(be=None),
               dict(di=None), dict(sh=None), dict(hn_=C.c_void_p(over.data_ptr())),
               dict(hn_=C.c_void_p(under.data_ptr())), dict(n=4)):
        assert call(**kw) == _abi.SSF_E_ARG, kw
        assert b"scan_context_match_topk" in L.ssf_last_error(fe._h), kw
    assert call(nq=0, q_=None, dn=None, hn_=None, be=None) == _abi.SSF_OK
    assert call(nq=0, q_=None, dn=None, hn_=None, be=None, k=0) == _abi.SSF_E_ARG     # k is checked first
    torch.cuda.synchronize()
    assert (buf == -7).all() and (dist == -7.0).all() and (shift == -7).all()
    for k, e, sel in ((3, 0, False), (8, 0, True), (8, 2 ** 31 - 1, False), (1, 3, True)):
        buf.fill_(-7)
        assert call(k=k, e=e, **(dict(di=None, sh=None) if sel else {})) == _abi.SSF_OK, L.ssf_last_error(fe._h)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:PAD] == -7).all() and (out[PAD + 2 * k:] == -7).all(), "sentinels overwritten"
        rec = out[PAD:PAD + 2 * k].reshape(2, k, 4)
        assert (rec[:, :, 3] == 0).all()
        for a, n in enumerate((5, 2)):
            filled = min(k, n) if e == 0 else 1
            assert (rec[a, :filled, 0] >= 0).all() and (rec[a, :filled, 0] < n).all()
            assert (rec[a, filled:, 0] == -1).all() and (rec[a, filled:, 2] == 0).all()
            assert (rec[a, filled:, 1].view(np.float32) == 1.0).all()
            want = TR.select_topk(dist[a].cpu().numpy(), shift[a].cpu().numpy(), n, k, e)
            if not sel:
                assert _same((rec[a, :, 0], rec[a, :, 1].view(np.float32), rec[a, :, 2]), want)


def test_query_topk_across_a_capacity_doubling(fe, dev):
    """(e) ScanContextDB.query_topk equals one match_topk on the same descriptors."""
    from ssf import scan_context as sc
    rng = np.random.default_rng(56)
    d = torch.from_numpy(_random_descs(rng, 11)).to(dev)
    q = torch.from_numpy(_random_descs(rng, 2)).to(dev)
    db = sc.ScanContextDB(fe, capacity=4)
    assert db.query_topk(q[0], 3) == []
    for k in range(4):
        db.append(d[k])
    before = db.query_topk(q[0], 3, 1)
    assert [(int(i), float(x), int(s)) for i, x, s in zip(*(t[0] for t in _topk(fe, q[:1], d[:4], 4, 3, 1)))
            if i >= 0] == before
    db.append(d[4:11])                                      # 4 -> 16
    assert db.generation == 1 and len(db) == 11
    for n_el in (None, 11, 6, 1, 0):
        for k, E in ((1, 0), (3, 0), (3, 2), (8, 4)):
            n = 11 if n_el is None else n_el
            want = _topk(fe, q, d, n, k, E)
            got = [t.cpu().numpy() for t in db.query_topk(q, k, E, n_el)]
            assert _same(got, want), (n_el, k, E)
            lst = db.query_topk(q[1], k, E, n_el)
            keep = want[0][1] >= 0
            assert [c[0] for c in lst] == want[0][1][keep].tolist() and [c[2] for c in lst] == want[2][1][keep].tolist()
            assert np.array_equal(_u32(np.array([c[1] for c in lst], np.float32)), _u32(want[1][1][keep]))
            assert all(type(c[0]) is int and type(c[1]) is float and type(c[2]) is int for c in lst)
    assert db.query_topk(q[1], 3, 2)[:1] == [db.query(q[1])]


# ------------------------------------------------------------------------------ the back-end
def _forward(fe, dev, frames, **kw):
    """The 30 forward frames through a LoopCloser -> (closer, the frame of every keyframe)."""
    from ssf import loop
    lc = loop.LoopCloser(fe, **kw)
    keys = []
    for k in range(30):
        T = frames[k]["T"]
        yaw = np.arctan2(T[1, 0], T[0, 0])
        pl = torch.from_numpy(frames[k]["planes"]).to(dev)
        _, c, is_key = lc.process(pl, (0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)), T[:3, 3], 0.1 * k)
        assert c is None
        if is_key:
            keys.append(k)
    return lc, keys


def test_local_maps_bit_for_bit(fe, dev, revisit_frames):  # noqa: F811
    """(f) every map of one local_maps call -- windows cut by both ends of the sequence, a full
    one, single keyframes, the same keyframe twice -- equals voxel_grid_one of the yardstick's
    map_points for the same parts."""
    from ssf import loop
    lc, keys = _forward(fe, dev, revisit_frames)
    n = len(keys)
    assert n >= 13
    items = [(0, 10), (12, 10), (n - 1, 10), (5, 3), (n - 1, 0), (0, 0), (5, 3), (n // 2, n)]
    maps, h_off = lc.local_maps(items)
    torch.cuda.synchronize()
    assert h_off.dtype == torch.int64 and len(h_off) == len(items) + 1 and int(h_off[0]) == 0
    assert int(h_off[-1]) == maps.shape[0] and maps.shape[1] == 4
    got = maps.cpu().numpy()
    for m, (key, w) in enumerate(items):
        ks = [k for k in range(key - w, key + w + 1) if 0 <= k < n]
        pts = MR.map_points([revisit_frames[keys[k]]["planes"] for k in ks], [lc._T6(k) for k in ks])
        want = loop.voxel_grid_one(fe, torch.from_numpy(pts).to(dev), lc.icp_leaf).cpu().numpy()
        mine = got[int(h_off[m]):int(h_off[m + 1])]
        assert len(want) > 0 and MR.same_bits(mine, want), (m, key, w, mine.shape, want.shape)
    assert MR.same_bits(got[int(h_off[3]):int(h_off[4])], got[int(h_off[6]):int(h_off[7])])
    empty, e_off = lc.local_maps([])
    assert empty.shape == (0, 4) and e_off.tolist() == [0]


YAW, DRIFT_X, DECOY_KEY = 183.0, 40.0, 12


@pytest.fixture(scope="module")
def decoy_scene(revisit_frames):  # noqa: F811
    """30 frames forward, then one revisit of frame 0 (stamp + 30 s, odometry 40 m off in x,
    sensor yawed by 183 degrees); keyframe 12 gets the revisit's scan as its own: the right
    appearance stored at the wrong place, 12 keyframes from keyframe 0 and so outside the default
    exclusion window of 10.  is_key_frame makes keyframe 12 from frame 18 (18 m from frame 0), so
    the decoy is placed by keyframe index, not by frame number."""
    from oracle import oracle as O
    scan = SR.rot_z(revisit_frames[0]["scan"], -YAW)
    return dict(scan=scan, planes=O.extract_planes(scan, 64))


def _drive_decoy(fe, dev, frames, scene, **kw):
    from ssf import loop, scan_context as sc
    lc = loop.LoopCloser(fe, detector="scan_context", sc=sc.sc_params(threshold=THRESHOLD), **kw)
    keys, scans, out = [], [], None
    for i in range(31):
        revisit = i == 30
        f = frames[0 if revisit else i]
        T = f["T"].copy()
        if revisit:
            T = T @ loop.get_transformation(0, 0, 0, 0, 0, np.deg2rad(YAW))
            T[0, 3] += DRIFT_X
        yaw = np.arctan2(T[1, 0], T[0, 0])
        scan = scene["scan"] if revisit or len(lc.key6d) == DECOY_KEY else f["scan"]   # read by a keyframe only
        pl = torch.from_numpy(scene["planes"] if revisit else f["planes"]).to(dev)
        _, c, is_key = lc.process(pl, (0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)), T[:3, 3],
                                  0.1 * i + (30.0 if revisit else 0.0), scan=torch.from_numpy(scan).to(dev))
        if is_key:
            keys.append(i)
            scans.append(scan)
        assert c is None or revisit, (i, c.key_cur, c.key_pre)
        out = c
    assert keys[-1] == 30, "the revisit is a keyframe"
    return lc, out, keys, scans


def test_second_candidate_closes_the_loop_the_nearest_cannot(fe, dev, revisit_frames, decoy_scene):  # noqa: F811
    """(g) The nearest descriptor is the decoy (keyframe 12, distance 0), where ICP fails its
    fitness gate: with sc_candidates=1 the revisit closes nothing.  With sc_candidates=2 the true
    keyframe 0 is verified in the same batch and closes the loop at shift 30, and the correction
    puts the keyframe within 0.1 m of the truth.

    Observed on an MI355X: see DESIGN.md §6.12."""
    frames = revisit_frames
    lc1, c1, keys, scans = _drive_decoy(fe, dev, frames, decoy_scene)
    cur = len(keys) - 1
    assert keys[0] == 0 and cur >= 14 and scans[12] is decoy_scene["scan"] and scans[cur] is decoy_scene["scan"]
    assert sum(s is decoy_scene["scan"] for s in scans) == 2
    print(f"[sc topk] keyframes from frames {keys}: the decoy is keyframe 12, frame {keys[12]}")
    # the yardstick first: the margins the scene is built for
    db = np.stack([SR.describe(s) for s in scans[:cur]])
    rd = SR.match(SR.describe(scans[cur])[None], db)[0][0]
    others = np.delete(rd, [0, 12])
    print(f"[sc topk] yardstick: decoy {rd[12]:.4f}, true {rd[0]:.4f}, nearest other {others.min():.4f}")
    assert rd[12] <= rd[0] - 0.02 and rd[0] <= THRESHOLD - 0.02 and others.min() >= THRESHOLD + 0.02
    dev_d = lc1.sc_db.query_topk(lc1.sc_db.descriptors()[cur], 8, 0, cur)
    print("[sc topk] device (idx, dist, shift), plain 8 smallest:", [(i, round(d, 4), s) for i, d, s in dev_d])
    assert [c[0] for c in dev_d[:2]] == [12, 0]
    assert all(abs(d - rd[i]) <= 1e-5 for i, d, _ in dev_d)

    assert c1 is None and lc1.constraints == [], "one candidate: the decoy is the only place tried"
    assert lc1.loop_record_index == cur + 2

    lc2, c2, keys2, _ = _drive_decoy(fe, dev, frames, decoy_scene, sc_candidates=2)
    assert keys2 == keys and c2 is not None and lc2.constraints == [c2]
    print(f"[sc topk] loop {c2.key_cur} -> {c2.key_pre}, dist {c2.dist:.4f}, shift {c2.shift}, noise {c2.noise:.4g}, "
          f"candidates {c2.candidates}")
    assert c2.key_cur == cur and c2.key_pre == 0 and c2.shift == 30
    assert [c[0] for c in c2.candidates] == [12, 0]
    assert c2.candidates[0][3] > 0.2 and c2.candidates[1][3] <= 0.2 and c2.candidates[1][4]
    assert lc2.sc_match == c2.candidates[1][:3] == (c2.key_pre, c2.dist, c2.shift)
    assert c2.noise == float(np.float32(c2.candidates[1][3]))
    assert abs(c2.dist - rd[0]) <= 1e-5 and c2.candidates[0][1] < c2.candidates[1][1]
    assert lc2.loop_index == {cur: 0} and lc2.loop_record_index == cur + 2 + 30
    fixed = c2.correction @ lc2._T6(cur)
    err = np.linalg.norm(fixed[:3, 3] - frames[0]["T"][:3, 3])
    print(f"[sc topk] corrected keyframe {err * 1e3:.3f} mm from the truth")
    assert err < 0.1, err
    assert np.array_equal(lc2.trans_loop_adjust, c2.correction)


def test_defaults_are_untouched(fe, dev, revisit_frames):  # noqa: F811
    """(h) sc_candidates=1 / sc_exclusion=None spelled out give the constraints of the arguments
    left alone, under both detectors, on the existing revisit scene."""
    from ssf import scan_context as sc

    def same(a, b):
        assert a[1] and len(a[1]) == len(b[1])
        for x, y in zip(a[1], b[1]):
            assert (x.key_cur, x.key_pre, x.noise, x.shift, x.dist) == (y.key_cur, y.key_pre, y.noise, y.shift, y.dist)
            assert x.between.tobytes() == y.between.tobytes() and x.correction.tobytes() == y.correction.tobytes()
            assert x.candidates is None and y.candidates is None
        assert a[0].key6d == b[0].key6d and a[0].loop_record_index == b[0].loop_record_index
    kw = dict(detector="scan_context", sc=sc.sc_params(threshold=THRESHOLD))
    same(_drive(fe, dev, revisit_frames, True, (0.0, DRIFT), **kw),
         _drive(fe, dev, revisit_frames, True, (0.0, DRIFT), sc_candidates=1, sc_exclusion=None, **kw))
    same(_drive(fe, dev, revisit_frames, False, (0.5, 0.0)),
         _drive(fe, dev, revisit_frames, False, (0.5, 0.0), detector="radius", sc_candidates=1, sc_exclusion=None))

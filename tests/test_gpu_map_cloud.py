"""The map cloud of the loop-closure back-end on the GPU (mapCloudPtr of src/mapOptmization.cpp:
updateKeyPose :296-312, correctPoses :315-332, publishResult :387-397): the batched rigid
transform ssf_transform_clouds_batch, ssf.MapCloud, LoopCloser(map_cloud=True), the
/sum_map_cloud_res3 topic of MapOptimizationNode and run_sequence(map_cloud=True).

Every comparison is bit for bit.  The transform yardstick is tests/map_reference.py (numpy
float64, the pinned expression, one rounding); the filter yardstick is the CPU oracle's
voxel_grid.  Both are independent of the code under test, so no tolerance is needed."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import map_reference as M
from helpers import frame

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD          # a NaN no transform produces


@pytest.fixture(scope="module")
def fe(dev):
    from ssf import Frontend
    return Frontend(64, device=dev)


def _call(fe, x, d_off, h_off, d_T, out, first=0, n=None):
    """the raw ABI call for clouds first ... first + n - 1 -> its return code"""
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    n = int(h_off.numel()) - 1 - first if n is None else n
    return _abi.lib().ssf_transform_clouds_batch(
        fe._h, _stream(fe.device), n, _ptr(x), C.c_void_p(d_off.data_ptr() + 8 * first),
        C.c_void_p(h_off.data_ptr() + 8 * first), C.c_void_p(d_T.data_ptr() + 96 * first), _ptr(out))


def _sentinel(n, dev):
    return torch.full((n, 4), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _setup(clouds, Ts, dev, base=0, tail=0):
    """clouds packed from point `base` on, `tail` spare points behind them"""
    sizes = [c.shape[0] for c in clouds]
    h_off = torch.tensor(np.concatenate([[base], base + np.cumsum(sizes)]), dtype=torch.int64)
    total = int(h_off[-1]) + tail
    host = np.zeros((total, 4), np.float32)
    host[base:int(h_off[-1])] = np.concatenate(clouds)
    T12 = np.ascontiguousarray(np.asarray(Ts, np.float64)[:, :3, :].reshape(-1, 12))
    return torch.from_numpy(host).to(dev), h_off.to(dev), h_off, torch.from_numpy(T12).to(dev), total


def test_kernel_ragged_clouds_and_untouched_points(fe, dev):
    from ssf import _abi, loop
    sizes = [0, 0, 1, 3, 255, 256, 257, 0, 1023, 1025, 5000, 2, 0]
    rng = np.random.default_rng(11)
    clouds = [M.cloud(rng, n) for n in sizes]
    Ts = [loop.get_transformation(*rng.uniform(-60, 60, 3), *rng.uniform(-0.3, 0.3, 2),
                                  rng.uniform(-math.pi, math.pi)) for _ in sizes]
    # the special poses go to clouds that have points (0 and 1 are empty)
    Ts[2] = np.eye(4)
    Ts[3] = loop.get_transformation(0, 0, 0, 0, 0, math.pi - 1e-3)
    Ts[4] = loop.get_transformation(1.5, -2.5, 0.5, 0.3, -0.3, 0.7)
    Ts[5] = loop.get_transformation(-4.0, 3.0, 1.0, -0.3, 0.3, -2.0)
    Ts[6] = loop.get_transformation(1000.0, -1000.0, 1000.0, 0.01, 0.02, 1.0)
    base, tail = 5, 7
    x, d_off, h_off, d_T, total = _setup(clouds, Ts, dev, base, tail)
    want = [M.transform(c, T) for c, T in zip(clouds, Ts)]
    ho = [int(v) for v in h_off]

    # every cloud
    out = _sentinel(total, dev)
    assert _call(fe, x, d_off, h_off, d_T, out) == _abi.SSF_OK
    torch.cuda.synchronize()
    got = _bits(out)
    for c, w in enumerate(want):
        assert np.array_equal(got[ho[c]:ho[c + 1]], w.view(np.uint32)), c
    assert (got[:base] == SENTINEL).all() and (got[ho[-1]:] == SENTINEL).all()
    # the identity pose returns its input bit for bit; intensities always do
    assert np.array_equal(got[ho[2]:ho[3]], clouds[2].view(np.uint32)) and sizes[2] == 1
    assert np.array_equal(got[base:ho[-1], 3], np.concatenate(clouds).view(np.uint32)[:, 3])

    # clouds 3 ... 9 only, through d_off + 3
    out = _sentinel(total, dev)
    assert _call(fe, x, d_off, h_off, d_T, out, first=3, n=7) == _abi.SSF_OK
    torch.cuda.synchronize()
    got = _bits(out)
    for c in range(3, 10):
        assert np.array_equal(got[ho[c]:ho[c + 1]], want[c].view(np.uint32)), c
    assert (got[:ho[3]] == SENTINEL).all() and (got[ho[10]:] == SENTINEL).all()

    # nothing to do: no clouds, or a range of empty clouds only
    out = _sentinel(total, dev)
    assert _call(fe, x, d_off, h_off, d_T, out, n=0) == _abi.SSF_OK
    assert _call(fe, x, d_off, h_off, d_T, out, first=0, n=2) == _abi.SSF_OK
    assert _call(fe, x, d_off, h_off, d_T, out, first=12, n=1) == _abi.SSF_OK
    # refused on the host, nothing written
    bad = h_off.clone()
    bad[5], bad[6] = h_off[6], h_off[5]
    assert _call(fe, x, d_off, bad, d_T, out) == _abi.SSF_E_ARG
    assert b"monotone" in _abi.lib().ssf_last_error(fe._h)
    assert _call(fe, x, d_off, h_off, d_T, out, n=-1) == _abi.SSF_E_ARG
    assert _call(fe, x, d_off, h_off, d_T, x) == _abi.SSF_E_ARG                  # aliased
    L, st, vp = _abi.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), lambda t: C.c_void_p(t.data_ptr())
    for args in ([None, vp(d_off), vp(h_off), vp(d_T), vp(out)], [vp(x), None, vp(h_off), vp(d_T), vp(out)],
                 [vp(x), vp(d_off), None, vp(d_T), vp(out)], [vp(x), vp(d_off), vp(h_off), None, vp(out)],
                 [vp(x), vp(d_off), vp(h_off), vp(d_T), None]):
        assert L.ssf_transform_clouds_batch(fe._h, st, 13, *args) == _abi.SSF_E_ARG
    torch.cuda.synchronize()
    assert (_bits(out) == SENTINEL).all()


def test_more_clouds_than_a_grid_dimension(fe, dev):
    """70 000 clouds of 0-2 points: no per-cloud grid dimension, and long runs of empty clouds"""
    from ssf import _abi
    rng = np.random.default_rng(12)
    K = 70000
    sizes = rng.integers(0, 3, K)
    sizes[1000:1400] = 0                                    # one run longer than a tile's clouds
    n = int(sizes.sum())
    pts = M.cloud(rng, n)
    yaw = rng.uniform(-math.pi, math.pi, K)
    T = np.zeros((K, 3, 4))
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    T[:, :, 3] = rng.uniform(-500, 500, (K, 3))
    h_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    x, d_off = torch.from_numpy(pts).to(dev), h_off.to(dev)
    d_T = torch.from_numpy(T.reshape(K, 12).copy()).to(dev)
    out = _sentinel(n + 3, dev)
    assert _call(fe, x, d_off, h_off, d_T, out) == _abi.SSF_OK
    torch.cuda.synchronize()
    want = M.transform(pts, T[np.repeat(np.arange(K), sizes)])
    got = _bits(out)
    assert np.array_equal(got[:n], want.view(np.uint32))
    assert (got[n:] == SENTINEL).all()


def test_map_cloud_append_regrow_rebuild(fe, dev, oracle):
    from ssf import MapCloud, loop
    rng = np.random.default_rng(13)
    K = 12
    sizes = [int(v) for v in rng.integers(10, 901, K)]
    clouds = [M.cloud(rng, n, half=1.0) for n in sizes]
    Ts = [loop.get_transformation(*rng.uniform(-50, 50, 3), *rng.uniform(-0.3, 0.3, 2), rng.uniform(-3, 3))
          for _ in range(K)]
    mc = MapCloud(fe, capacity_points=64, capacity_keyframes=4)
    assert (mc.n_keyframes, mc.n_points) == (0, 0)
    assert tuple(mc.points().shape) == (0, 4) and tuple(mc.filtered(0.4).shape) == (0, 4)
    views, grown = [], 0
    for k in range(K):
        gen, ptrs = mc.generation, (mc.raw.data_ptr(), mc.mapped.data_ptr())
        views.append(mc.store(torch.from_numpy(clouds[k]).to(dev)))
        if mc.generation == gen:                            # between growths nothing moves
            assert (mc.raw.data_ptr(), mc.mapped.data_ptr()) == ptrs
        else:
            grown += 1
        mc.transform(k, k + 1, [Ts[k]])
        n = sum(sizes[:k + 1])
        assert (mc.n_keyframes, mc.n_points) == (k + 1, n) and mc.capacity_points >= n
        assert [int(v) for v in mc.h_off[:k + 2]] == [int(v) for v in mc.d_off[:k + 2].cpu()]
        assert M.same_bits(mc.raw[:n].cpu().numpy(), np.concatenate(clouds[:k + 1])), k
        for j, v in enumerate(views):                       # views handed out before a regrowth keep their values
            assert M.same_bits(v.cpu().numpy(), clouds[j]) and M.same_bits(mc.keyframe(j).cpu().numpy(), clouds[j]), (k, j)
        assert M.same_bits(mc.points().cpu().numpy(), M.map_points(clouds[:k + 1], Ts[:k + 1])), k
    assert grown >= 3 and mc.capacity_points < 4 * sum(sizes)

    # every pose rewritten, the map contracts into a smaller box: one launch
    Ts2 = [loop.get_transformation(*rng.uniform(-0.5, 0.5, 3), *rng.uniform(-0.3, 0.3, 2), rng.uniform(-3, 3))
           for _ in range(K)]
    mc.transform(0, K, Ts2)
    want = M.map_points(clouds, Ts2)
    assert M.same_bits(mc.points().cpu().numpy(), want)
    assert np.abs(want[:, :3]).max() < 8.0
    ref = oracle.voxel_grid(want, 0.4)
    assert ref.shape[0] < want.shape[0] // 2                # the filter has something to merge
    got = mc.filtered(0.4).cpu().numpy()
    assert got.shape == ref.shape and M.same_bits(got, ref)
    assert M.same_bits(got, loop.voxel_grid_one(fe, torch.from_numpy(want).to(dev), 0.4).cpu().numpy())
    assert M.same_bits(mc.filtered().cpu().numpy(), ref)    # 0.4 is the default leaf
    # a sub-range leaves the rest alone
    mc.transform(4, 7, Ts[4:7])
    mixed = Ts2[:4] + Ts[4:7] + Ts2[7:]
    assert M.same_bits(mc.points().cpu().numpy(), M.map_points(clouds, mixed))
    with pytest.raises(ValueError):
        mc.transform(0, K + 1, mixed + [np.eye(4)])
    with pytest.raises(ValueError):
        mc.transform(0, K, mixed[:-1])


# ------------------------------------------------------------------------- LoopCloser(map_cloud=True)
def _square(n=20, step=1.5):
    """ground truth on a closed square and a drifting odometry of it"""
    from ssf import loop
    gt, od = [], []
    x = y = 0.0
    per = n // 4
    for k in range(n):
        yaw = (k // per) * math.pi / 2
        gt.append(loop.get_transformation(x, y, 0.0, 0.0, 0.0, yaw))
        x += step * math.cos(yaw)
        y += step * math.sin(yaw)
    od.append(gt[0].copy())
    for k in range(1, n):
        d = np.linalg.inv(gt[k - 1]) @ gt[k]
        d = d @ loop.get_transformation(0.01, 0.0, 0.002, 0.0, 0.0005, 0.004)
        od.append(od[-1] @ d)
    return gt, od


def _key_clouds(n, seed):
    rng = np.random.default_rng(seed)
    return [M.cloud(rng, 20 + 7 * k, half=20.0) for k in range(n)]


def _perfect_constraint(lc, gt):
    from ssf import loop
    cur = len(lc.key6d) - 1
    corr = gt[cur] @ np.linalg.inv(lc._T6(cur))
    return loop.LoopConstraint(cur, 0, loop.between(gt[cur], lc._T6(0)), 0.02, corr)


def _feed(lc, clouds, od, k, dev):
    from ssf import loop
    p = loop.pose7_from_matrix(od[k])
    out = lc.process(torch.from_numpy(clouds[k]).to(dev), p[:4], p[4:], 0.1 * k)
    assert out[2]                                           # every frame is a keyframe
    return out


def _map_is(lc, clouds):
    K = len(lc.key6d)
    assert lc.map.n_keyframes == K == len(lc.key_frames)
    for k in range(K):
        assert M.same_bits(lc.key_frames[k].cpu().numpy(), clouds[k]), k
    want = M.map_points(clouds[:K], [lc._T6(i) for i in range(K)])
    assert M.same_bits(lc.map.points().cpu().numpy(), want)
    return want


def test_loop_closer_keeps_the_map_at_the_key_poses(fe, dev):
    from ssf import MapCloud, loop
    n = 20
    gt, od = _square(n)
    clouds = _key_clouds(n, 14)
    runs = {}
    for on in (True, False):
        # a tiny store, so that it moves under the closer's key_frames views several times
        lc = (loop.LoopCloser(fe, optimize=True, map_cloud=True, map=MapCloud(fe, capacity_points=64)) if on
              else loop.LoopCloser(fe, optimize=True))
        lc.add_loop_factor = lambda: None
        outs = [_feed(lc, clouds, od, k, dev) for k in range(n - 1)]
        if on:
            assert isinstance(lc.map, MapCloud) and lc.map.generation >= 3
            before6d = [list(v) for v in lc.key6d]
            before = _map_is(lc, clouds)                    # every keyframe at its append-time pose
        else:
            assert lc.map is None
        local = lc.local_map(5, 2).cpu().numpy()
        lc.add_loop_factor = lambda: _perfect_constraint(lc, gt)
        outs.append(_feed(lc, clouds, od, n - 1, dev))
        assert outs[-1][1] is not None and lc.last_optimization is not None
        assert lc.last_optimization["status_name"] in ("ok", "converged")
        if on:
            assert [v[:6] for v in lc.key6d[:n - 1]] != [v[:6] for v in before6d]     # rewritten
            after = _map_is(lc, clouds)                     # rebuilt under the rewritten key6d
            assert not M.same_bits(after[:before.shape[0]], before)
        runs[on] = (lc, outs, local)
    (a, oa, la), (b, ob, lb) = runs[True], runs[False]
    assert a.key6d == b.key6d and M.same_bits(la, lb)
    for (Ta, ca, ka), (Tb, cb, kb) in zip(oa, ob):
        assert np.array_equal(Ta, Tb) and ka == kb and (ca is None) == (cb is None)
    assert a.last_optimization["poses"].tobytes() == b.last_optimization["poses"].tobytes()

    # without optimize the key poses never change: a closure leaves the map appended only
    lc = loop.LoopCloser(fe, map_cloud=True)
    lc.add_loop_factor = lambda: None
    for k in range(6):
        _feed(lc, clouds, od, k, dev)
    first = _map_is(lc, clouds)
    lc.add_loop_factor = lambda: _perfect_constraint(lc, gt)
    _, c, _ = _feed(lc, clouds, od, 6, dev)
    assert c is not None and lc.last_optimization is None
    assert M.same_bits(_map_is(lc, clouds)[:first.shape[0]], first)


def test_two_closers_rebuilt_through_one_launch(fe, dev):
    from ssf import loop
    gt, od = _square(20)
    closers, cons, befores, sets = [], [], [], []
    for s in range(2):
        clouds = _key_clouds(20, 15 + s)
        lc = loop.LoopCloser(fe, optimize=True, map_cloud=True)
        lc.add_loop_factor = lambda: None
        for k in range(20 - 3 * s):
            _feed(lc, clouds, od, k, dev)
        befores.append(_map_is(lc, clouds))
        cons.append(_perfect_constraint(lc, gt))
        closers.append(lc)
        sets.append(clouds)
    Ts = loop.optimize_loop_closers(fe, closers, cons)
    for lc, clouds, before, T in zip(closers, sets, befores, Ts):
        assert lc.last_optimization is not None and np.array_equal(T, lc._T6(-1))
        after = _map_is(lc, clouds)
        assert after.shape == before.shape and not M.same_bits(after, before)


# ------------------------------------------------------------------------- node, replay
N_FRAMES = 12


def _stamp(k):
    t_ns = k * 100_000_000
    return t_ns // 1_000_000_000, t_ns % 1_000_000_000


def _bus_run(dev, tum, map_cloud):
    """the run_onlyPC.launch graph plus mapOptmization on a Bus -> (bus, node, per frame
    (numFrame, keyframes) after the frame)"""
    from ssf import nodes

    class OrderBus(nodes.Bus):
        def __init__(self, keep):
            super().__init__(keep)
            self.order = []

        def publish(self, topic, msg):
            self.order.append(topic)
            super().publish(topic, msg)

    bus = OrderBus(keep=64)
    pco = nodes.PointCloudOdometryNode(bus.publish, device=dev, mode="none")
    ff = nodes.FrameFeatureNode(bus.publish, device=dev)
    lo = nodes.LidarOdometryNode(bus.publish, device=dev)
    mo = (nodes.MapOptimizationNode(bus.publish, device=dev, tum_path=tum, map_cloud=True) if map_cloud
          else nodes.MapOptimizationNode(bus.publish, device=dev, tum_path=tum))
    bus.subscribe("/velodyne_points", ff.on_cloud)
    bus.subscribe("/plane_frame_cloud1", lo.on_plane_cloud)
    bus.subscribe("/plane_frame_cloud2", mo.on_plane_cloud)
    bus.subscribe("/frame_odom2", mo.on_odom)
    trace = []
    for k in range(N_FRAMES):
        pco.on_frame(frame(5, k, n_az=600)[0], None, _stamp(k))
        trace.append((mo.num_frame, len(mo.closer.key6d)))
    return bus, mo, trace


def test_node_publishes_the_filtered_map(dev, oracle, tmp_path):
    from ssf import io as sio
    from ssf import nodes
    tum_on, tum_off = str(tmp_path / "on.txt"), str(tmp_path / "off.txt")
    with torch.cuda.device(dev):
        bus, mo, trace = _bus_run(dev, tum_on, True)
        bus0, mo0, trace0 = _bus_run(dev, tum_off, False)
    lc = mo.closer
    keys = [c.cpu().numpy() for c in lc.key_frames]
    poses = [lc._T6(i) for i in range(len(keys))]
    print("(numFrame, keyframes) per frame:", trace)
    assert trace[0] == (0, 0) and trace[-1][0] == N_FRAMES - 1          # the first cloud has no pose yet
    assert len(keys) >= (N_FRAMES - 1) // 2                             # most pairs are keyframes
    # expected messages: keyframes whose pair count is a multiple of 5
    expect = []
    for k in range(1, N_FRAMES):
        num, nk = trace[k]
        if num % 5 == 0 and nk == trace[k - 1][1] + 1:
            expect.append((k, nk))
    msgs = bus.log["/sum_map_cloud_res3"]
    assert len(msgs) == len(expect) == mo.map_published and len(msgs) >= 1, (trace, len(msgs))
    for m, (k, nk) in zip(msgs, expect):
        assert m.header.frame_id == "map" and m.point_step == 32 and sio.stamp_of(m.header) == _stamp(k)
        want = oracle.voxel_grid(M.map_points(keys[:nk], poses[:nk]), 0.4)
        got = sio.cloud_xyzi(m)
        assert got.shape == want.shape and M.same_bits(got, want), (k, nk)
        assert 0 < want.shape[0] < sum(c.shape[0] for c in keys[:nk])
    # without the option: no such topic, everything else byte for byte the same
    assert "/sum_map_cloud_res3" not in bus0.log and mo0.closer.map is None and trace0 == trace
    assert open(tum_on, "rb").read() == open(tum_off, "rb").read()
    assert bus.log["/map_odom_res3"] == bus0.log["/map_odom_res3"] and len(bus.log["/map_odom_res3"]) == N_FRAMES - 1
    assert [m.data for m in bus.log["/map_frame_res3"]] == [m.data for m in bus0.log["/map_frame_res3"]]
    assert [m.header for m in bus.log["/map_frame_res3"]] == [m.header for m in bus0.log["/map_frame_res3"]]
    assert bus.log["/map_laser_path_res3"][-1] == bus0.log["/map_laser_path_res3"][-1]
    # the map goes out after the three other topics of its frame
    at = [i for i, t in enumerate(bus.order) if t == "/sum_map_cloud_res3"]
    assert len(at) == len(msgs)
    for i in at:
        assert bus.order[i - 3:i] == ["/map_odom_res3", "/map_laser_path_res3", "/map_frame_res3"]
    assert [t for t in bus.order if t != "/sum_map_cloud_res3"] == bus0.order

    # the replay: the final map, filtered once at the end
    data = tmp_path / "data"
    data.mkdir()
    for k in range(N_FRAMES):
        f = frame(5, k, n_az=600)
        np.savez(str(data / f"{k:06d}.npz"), pos1=f[0], gt=f[1])
    t2, t3 = str(tmp_path / "odom2.txt"), str(tmp_path / "map.txt")
    u2, u3 = str(tmp_path / "odom2_off.txt"), str(tmp_path / "map_off.txt")
    with torch.cuda.device(dev):
        res = nodes.run_sequence(str(data), t2, launch="onlyPC", map_tum_path=t3, map_cloud=True)
        off = nodes.run_sequence(str(data), u2, launch="onlyPC", map_tum_path=u3)
    final = oracle.voxel_grid(M.map_points(keys, poses), 0.4)
    assert res["map_cloud"].dtype == np.float32 and M.same_bits(res["map_cloud"], final)
    assert res["map_cloud_published"] == len(msgs) and res["map_cloud_keyframes"] == len(keys)
    assert not [k for k in off if k.startswith("map_cloud")]
    assert open(t3, "rb").read() == open(u3, "rb").read()
    assert open(t2, "rb").read() == open(u2, "rb").read()
    assert np.array_equal(res["odom2"], off["odom2"])

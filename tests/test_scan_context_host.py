"""CPU checks of the Scan Context loop detector: the numpy yardstick
(tests/scan_context_reference.py, which the kernels are held to in tests/test_gpu_scan_context.py)
on hand-built cases -- one point per bin, the sign of the shift, no jointly valid columns, ties
of the selection, the eligible prefix --, the host-side pieces of ssf.scan_context, and the
argument errors that come before any device call."""
import ctypes as C

import numpy as np
import pytest

import scan_context_reference as SR


def _bin_centres():
    """One point in the middle of every bin, each with its own height -> (points, heights)."""
    ring, sector = np.meshgrid(np.arange(SR.RINGS), np.arange(SR.SECTORS), indexing="ij")
    r = (ring + 0.5) * (SR.MAX_RANGE / SR.RINGS)
    phi = (sector + 0.5) * SR.SECTOR_ANGLE
    z = -1.5 + 0.01 * (ring * SR.SECTORS + sector)
    pts = np.stack([r * np.cos(phi), r * np.sin(phi), z], -1).reshape(-1, 3).astype(np.float32)
    return pts, (pts[:, 2] + np.float32(2.0)).reshape(SR.RINGS, SR.SECTORS)


def test_yardstick_one_point_per_bin():
    pts, want = _bin_centres()
    keep, ring, sector, rm, sm = SR.bins(pts)
    assert keep.all()
    assert np.array_equal(ring, np.repeat(np.arange(20), 60)) and np.array_equal(sector, np.tile(np.arange(60), 20))
    assert np.allclose(rm, 2.0, atol=1e-4) and np.allclose(sm, SR.SECTOR_ANGLE / 2, atol=1e-6)
    desc = SR.describe(pts)
    assert desc.dtype == np.float32 and np.array_equal(desc, want) and (desc > 0).all()
    # order-free, and a second lower point in a bin changes nothing
    perm = np.random.default_rng(0).permutation(len(pts))
    low = pts.copy()
    low[:, 2] -= 0.25
    assert np.array_equal(SR.describe(np.concatenate([low, pts[perm]])), want)


def test_yardstick_skips_and_clamps():
    pts = np.array([[1, 1, 0.5], [np.nan, 1, 9], [1, np.inf, 9], [1, 1, np.nan], [80, 0, 9], [60, 60, 9],
                    [79.99, 0, 1.0], [0, 0, 0.25], [5, -1e-9, -3.0], [-4.5, 0, -2.0]], np.float32)
    keep = SR.bins(pts)[0]
    assert keep.tolist() == [True, False, False, False, False, False, True, True, True, True]
    d = SR.describe(pts)
    want = np.zeros((20, 60), np.float32)
    want[0, 7] = 2.5                    # 45 degrees: sector 7
    want[19, 0] = 3.0
    want[0, 0] = 2.25                   # the origin: atan2(0, 0) = 0
    # (5, -1e-9): sector 59, height -1 -> max(0, .) leaves the bin empty; (-4.5, 0): sector 30, height 0
    assert np.array_equal(d, want)
    assert np.array_equal(SR.describe(np.zeros((0, 3), np.float32)), np.zeros((20, 60), np.float32))
    assert SR.describe_batch(pts, [0, 1, 9]).shape == (3, 20, 60)
    assert np.array_equal(SR.describe_batch(pts, [0, 1, 9])[0], np.zeros((20, 60), np.float32))


def test_yardstick_margins():
    pts = np.array([[4.0, 0.0, 0], [3.9990, 0.001, 0], [np.cos(np.pi / 30) * 10, np.sin(np.pi / 30) * 10, 0],
                    [79.9995, -1e-5, 0], [0.5, 0.5, 0]], np.float32)
    _, _, _, rm, sm = SR.bins(pts)
    assert rm[0] < 1e-6 and sm[0] == 0.0
    assert 0.9e-3 < rm[1] < 1.1e-3
    assert sm[2] < 1e-6 and abs(rm[2] - 2.0) < 1e-5
    assert rm[3] < 1e-3 and sm[3] < 1e-6            # next to max_range and to the wrap
    assert rm[4] > 0.7 and abs(sm[4] - np.pi / 60) < 1e-6
    assert np.isinf(SR.bins(np.array([[np.nan, 0, 0]], np.float32))[3][0])


def _clean_cloud(rng, n):
    """Random points at least 1e-3 m / 1e-3 rad from every bin edge."""
    r = rng.uniform(0.5, 79.0, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    pts = np.stack([r * np.cos(phi), r * np.sin(phi), rng.uniform(-1.9, 6.0, n)], -1).astype(np.float32)
    _, _, _, rm, sm = SR.bins(pts)
    return pts[(rm > 2e-3) & (sm > 2e-3)]


@pytest.mark.parametrize("k", [0, 1, 16, 30, 59])
def test_yardstick_shift_sign_convention(k):
    """A query whose sensor is yawed by +theta relative to the candidate's sees the points rotated
    by -theta; theta = k * 6 degrees gives distance 0 at shift k."""
    pts = _clean_cloud(np.random.default_rng(5), 4000)
    cand = SR.describe(pts)
    query = SR.describe(SR.rot_z(pts, -6.0 * k))
    assert np.array_equal(query, np.roll(cand, -k, axis=1))           # q[:, j] = c[:, (j + k) % 60]
    dist, shift = SR.distance(query, cand)
    assert abs(dist) < 1e-12 and shift == k
    d = SR.shift_distances(query, cand)
    assert (np.delete(d, k) > 0.05).all()


def test_yardstick_no_jointly_valid_columns_and_single_rings():
    zero = np.zeros((20, 60), np.float32)
    q = zero.copy()
    q[3, 0] = 1.5
    assert SR.distance(q, zero) == (1.0, 0) and SR.distance(zero, q) == (1.0, 0) and SR.distance(zero, zero) == (1.0, 0)
    c = zero.copy()
    c[3, 5] = 0.25                       # one valid column each: jointly valid only at shift 5
    d = SR.shift_distances(q, c)
    assert d[5] == 0.0 and (np.delete(d, 5) == 1.0).all() and SR.distance(q, c) == (0.0, 5)
    c[3, 5], c[4, 5] = 0.0, 0.25         # orthogonal single-ring columns: cosine 0
    assert SR.distance(q, c) == (1.0, 0)
    # the mean runs over the jointly valid columns only
    q2, c2 = zero.copy(), zero.copy()
    q2[1, 0], q2[1, 1], c2[1, 0], c2[2, 1], c2[1, 2] = 1, 1, 2, 2, 2
    d = SR.shift_distances(q2, c2)
    assert d[0] == 0.5 and d[1] == 0.5 and d[59] == 0.0 and d[2] == 0.0


def test_yardstick_selection_ties_and_prefix():
    row = [0.3, 0.1, 0.1, 0.2, 0.05]
    assert SR.select(row, 5) == 4 and SR.select(row, 4) == 1 and SR.select(row, 2) == 1
    assert SR.select(row, 1) == 0 and SR.select(row, 0) == -1
    assert SR.select([1.0, 1.0, 1.0], 3) == 0


def test_yardstick_batched_match_is_the_pairwise_definition():
    rng = np.random.default_rng(9)
    d = (rng.uniform(0, 5, (7, 20, 60)) * (rng.random((7, 20, 60)) < 0.3)).astype(np.float32)
    d[:, :, ::7] = 0
    d[2] = 0
    dist, shift, dall = SR.match(d[:3], d[2:])
    for a in range(3):
        for b in range(5):
            want = SR.shift_distances(d[a], d[2 + b])
            assert np.abs(dall[a, b] - want).max() < 1e-14
            assert abs(dist[a, b] - SR.distance(d[a], d[2 + b])[0]) < 1e-14
    assert dist[2, 0] == 1.0 and shift[2, 0] == 0 and dist.shape == (3, 5)
    assert SR.match(d[:2], d[:0])[0].shape == (2, 0)


def test_eligible_prefix_rule():
    """Leading keyframes more than time_gap older than the current one; the count stops at the
    first that is not, also when a later stamp (a non-monotone sequence) would qualify."""
    from ssf import scan_context as sc
    cases = [([], 30.0, 20.0), ([0.0, 1.0, 2.0], 30.0, 20.0), ([0.0, 10.0, 10.5], 30.0, 20.0),
             ([0.0, 1.0, 25.0, 3.0], 30.0, 20.0), ([15.0, 0.0], 30.0, 20.0), ([9.99, 10.0, 0.0], 30.0, 20.0),
             ([0.0, 1.0], 5.0, 20.0)]
    want = [0, 3, 1, 2, 0, 1, 0]
    for (stamps, cur, gap), w in zip(cases, want):
        assert SR.eligible_prefix(stamps, cur, gap) == w, (stamps, cur, gap)
        assert sc.eligible_prefix(stamps, cur, gap) == w, (stamps, cur, gap)


def test_params_and_detector_parsing():
    from ssf import scan_context as sc
    p = sc.sc_params()
    assert (p.max_range, p.lidar_height) == (80.0, 2.0) and p.threshold == np.float32(0.13)
    assert sc.sc_params(threshold=0.2).threshold == np.float32(0.2)
    for bad in (dict(max_range=0.0), dict(max_range=float("inf")), dict(lidar_height=float("nan")),
                dict(threshold="x")):
        with pytest.raises(ValueError):
            sc.sc_params(**bad)
    assert sc.parse_detector("radius") == ("radius", None)
    assert sc.parse_detector("scan-context") == ("scan_context", None)
    assert sc.parse_detector("scan-context:0.2") == ("scan_context", 0.2)
    for bad in ("kd-tree", "radius:3", "scan-context:", "scan-context:x"):
        with pytest.raises(ValueError):
            sc.parse_detector(bad)


def test_loop_closer_scan_context_needs_scan_before_any_device_call():
    """No context, no tensors: the ValueError comes before anything touches a device."""
    from ssf import loop
    lc = loop.LoopCloser(None, detector="scan_context")
    with pytest.raises(ValueError, match="scan"):
        lc.process(None, (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.0)
    assert lc.key6d == [] and len(lc.sc_db) == 0
    with pytest.raises(ValueError, match="detector"):
        loop.LoopCloser(None, detector="kd_tree")
    with pytest.raises(ValueError, match="scan_context"):
        loop.LoopCloser(None, sc=object())
    assert loop.LoopCloser(None).detector == "radius"


def test_run_map_detector_flag(capsys, tmp_path):
    """python -m ssf.run --map-detector: listed, needs --map-tum, and its value is parsed before a
    device is looked for"""
    from ssf import nodes, run
    with pytest.raises(SystemExit) as e:
        run.main(["--help"])
    assert e.value.code == 0 and "--map-detector" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        run.main([str(tmp_path), "--map-detector", "scan-context"])
    assert e.value.code == 2 and "--map-tum" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run.main([str(tmp_path), "--map-tum", str(tmp_path / "m.txt"), "--map-detector", "kd-tree"])
    assert e.value.code == 2 and "--map-detector" in capsys.readouterr().err
    with pytest.raises(ValueError, match="map_tum_path"):
        nodes.run_sequence(str(tmp_path), None, map_detector="scan_context")
    with pytest.raises(ValueError, match="map_detector"):
        nodes.run_sequence(str(tmp_path), None, map_tum_path="", map_detector="kd_tree")
    with pytest.raises(ValueError, match="map_sc_threshold"):
        nodes.run_sequence(str(tmp_path), None, map_tum_path="", map_sc_threshold=0.2)


@pytest.mark.parametrize("value, extra", [("radius", {}), ("scan-context", dict(map_detector="scan_context", map_sc_threshold=None)),
                                          ("scan-context:0.2", dict(map_detector="scan_context", map_sc_threshold=0.2))])
def test_entry_map_detector_param(monkeypatch, value, extra):
    """mapOptmization in ROS mode: ~MAP_DETECTOR picks the detector; scan-context also subscribes
    the node to /velodyne_points, radius builds and wires it as without the parameter"""
    import types

    import torch
    from ssf import entry, nodes, rosbridge
    log = dict(subscribed=[], built=[])
    params = {"~MAP_DETECTOR": value}

    class Msg:
        pass

    rospy = types.SimpleNamespace(
        init_node=lambda name, **k: None, has_param=lambda k: k in params, get_param=lambda k: params[k],
        Subscriber=lambda topic, klass, cb, queue_size=None: log["subscribed"].append(topic),
        Publisher=lambda topic, klass, queue_size=None: None, loginfo=lambda *a: None, spin=lambda: None, Time=Msg)
    mods = (rospy, types.SimpleNamespace(PointCloud2=Msg, PointField=Msg),
            types.SimpleNamespace(Header=Msg, Float64MultiArray=Msg), types.SimpleNamespace(Odometry=Msg, Path=Msg),
            types.SimpleNamespace(Pose=Msg, PoseStamped=Msg))
    monkeypatch.setattr(rosbridge, "available", lambda: True)
    monkeypatch.setattr(rosbridge, "require", lambda: mods)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)

    class Node:
        def __init__(self, publish, **kw):
            log["built"].append(kw)

        def on_plane_cloud(self, msg):
            pass

        def on_scan(self, msg):
            pass

    monkeypatch.setattr(nodes, "MapOptimizationNode", Node)
    entry.node_main("mapOptmization", ["__name:=mapOptmization"])
    assert log["built"] == [dict(device=0, tum_path=None, **extra)]
    assert log["subscribed"] == (["/velodyne_points"] if extra else []) + ["/plane_frame_cloud2", "/frame_odom2"]


def test_arg_errors_without_gpu():
    """SSF_E_ARG on the null context, before any HIP call."""
    from ssf import _abi
    L = _abi.lib()
    p = _abi.ScParams()
    assert L.ssf_sc_params_default(C.byref(p)) == _abi.SSF_OK
    assert L.ssf_sc_params_default(None) == _abi.SSF_E_ARG
    assert L.ssf_scan_context_batch(None, None, 1, None, 3, None, None, C.byref(p), None) == _abi.SSF_E_ARG
    assert L.ssf_scan_context_match(None, None, 1, None, 1, None, None, None, None, None, None) == _abi.SSF_E_ARG

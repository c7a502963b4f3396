"""Map cloud, CPU side: the argument checks of ssf_transform_clouds_batch that need no device,
the command-line and replay options, the ROS-mode parameter of the mapOptmization executable
(stand-in rospy), and the sanity of the numpy yardstick (tests/map_reference.py) the GPU tests
compare against."""
import ctypes as C
import struct
import types

import numpy as np
import pytest

import map_reference as M


def test_transform_symbol_rejects_bad_arguments_without_a_device():
    """a null context is SSF_E_ARG whatever else is passed, and nothing is dereferenced"""
    from ssf import _abi
    L = _abi.lib()
    assert "ssf_transform_clouds_batch" in _abi.EXPORTS
    assert L.ssf_abi_version() == 2
    f = L.ssf_transform_clouds_batch
    assert f(None, None, 1, None, None, None, None, None) == _abi.SSF_E_ARG          # null everything
    assert f(None, None, -1, None, None, None, None, None) == _abi.SSF_E_ARG         # negative count
    assert f(None, None, 0, None, None, None, None, None) == _abi.SSF_E_ARG          # null context alone
    off = np.array([0, 3], np.int64)
    bad = np.array([3, 0], np.int64)
    buf, out = np.zeros(64, np.float32), np.zeros(64, np.float32)
    T = np.zeros(12)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert f(None, None, 1, vp(buf), vp(off), vp(off), vp(T), vp(out)) == _abi.SSF_E_ARG
    assert f(None, None, 1, vp(buf), vp(off), vp(bad), vp(T), vp(out)) == _abi.SSF_E_ARG
    assert f(None, None, 1, vp(buf), vp(off), vp(off), None, vp(out)) == _abi.SSF_E_ARG
    assert L.ssf_last_error(None) == b"null context"
    assert not out.any()


def test_map_cloud_is_exported_and_pose_rows():
    import ssf
    from ssf import loop, map_cloud
    assert ssf.MapCloud is map_cloud.MapCloud and "MapCloud" in ssf.__all__
    T = loop.get_transformation(1.0, 2.0, 3.0, 0.1, -0.2, 0.3)
    rows = map_cloud.pose_rows([T, np.eye(4)])
    assert rows.shape == (2, 12) and rows.dtype == np.float64
    assert rows[0].tolist() == T[:3].reshape(-1).tolist()
    assert rows[1].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    assert np.array_equal(map_cloud.pose_rows(np.stack([T[:3]])), rows[:1])
    assert np.array_equal(map_cloud.pose_rows(rows), rows)
    assert map_cloud.pose_rows([]).shape == (0, 12)


def test_loop_closer_without_the_option_has_no_map():
    from ssf import loop

    class NoGpu:
        device = None

    lc = loop.LoopCloser(NoGpu())
    assert lc.map is None and lc.map_cloud is False


def test_run_help_lists_map_cloud(capsys):
    """python -m ssf.run --help (its main, in process)"""
    from ssf import run
    with pytest.raises(SystemExit) as e:
        run.main(["--help"])
    assert e.value.code == 0
    assert "--map-cloud" in capsys.readouterr().out


def test_run_map_cloud_needs_map_tum(capsys, tmp_path):
    from ssf import run
    with pytest.raises(SystemExit) as e:
        run.main([str(tmp_path), "--map-cloud", str(tmp_path / "m.npy")])
    assert e.value.code == 2 and "--map-tum" in capsys.readouterr().err


def test_run_sequence_map_cloud_needs_map_tum_path(tmp_path):
    """refused before a device is looked for (this machine has none)"""
    from ssf import nodes
    with pytest.raises(ValueError, match="map_tum_path"):
        nodes.run_sequence(str(tmp_path), None, map_cloud=True)
    with pytest.raises(ValueError, match="map_tum_path"):
        nodes.run_sequence(str(tmp_path), None, launch="onlyPC", map_optimize=True, map_cloud=True)


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def test_yardstick_reproduces_hand_computed_points():
    # a quarter turn about z and a shift: (1, 2, 3) -> (-2 + 1, 1 + 2, 3 + 3)
    T = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], np.float64)
    got = M.transform(np.array([[1, 2, 3, 7.25]], np.float32), T)
    assert got.dtype == np.float32 and got.tolist() == [[-1.0, 3.0, 6.0, 7.25]]
    # the pinned order in plain Python doubles: ((a x + b y) + c z) + d, then one rounding
    from ssf import loop
    T = loop.get_transformation(1000.0, -3.5, 0.25, 0.3, -0.3, np.pi - 1e-3)
    p = np.array([[12.34, -56.78, 9.1, 1234.17]], np.float32)
    x, y, z = (float(v) for v in p[0, :3])
    want = [_f32(((float(T[r, 0]) * x + float(T[r, 1]) * y) + float(T[r, 2]) * z) + float(T[r, 3])) for r in range(3)]
    got = M.transform(p, T)[0]
    assert [float(v) for v in got[:3]] == want and got[3] == p[0, 3]
    # ((0.1 + 0.2) + 0.3) + 0.4 = 1.0000000000000002 in double, 1 in float
    T = np.array([[0.1, 0.2, 0.3, 0.4]] * 3)
    assert M.transform(np.array([[1, 1, 1, 0]], np.float32), T)[0, :3].tolist() == [1.0, 1.0, 1.0]
    # the map: keyframe order, then input order; empty clouds vanish
    a, b = np.array([[1, 0, 0, 5]], np.float32), np.zeros((0, 4), np.float32)
    c = np.array([[0, 1, 0, 6], [0, 0, 1, 7]], np.float32)
    sh = np.eye(4)
    sh[0, 3] = 10
    m = M.map_points([a, b, c], [np.eye(4), sh, sh])
    assert m.tolist() == [[1, 0, 0, 5], [10, 1, 0, 6], [10, 0, 1, 7]]
    assert M.map_points([], []).shape == (0, 4)
    assert M.same_bits(m, m.copy()) and not M.same_bits(m, m[:2]) and not M.same_bits(np.float32([[0.0]]), np.float32([[-0.0]]))


def test_yardstick_cloud_is_seeded_and_in_range():
    a, b = M.cloud(np.random.default_rng(3), 500), M.cloud(np.random.default_rng(3), 500)
    assert M.same_bits(a, b) and a.shape == (500, 4)
    assert np.abs(a[:, :3]).max() <= 80.0
    frac = a[:, 3] - np.floor(a[:, 3])
    assert (a[:, 3] >= 0).all() and (frac < 0.64).all()


def _fake_ros(params, log):
    class Msg:
        pass

    class Publisher:
        def __init__(self, topic, klass, queue_size=None):
            log["advertised"].append((topic, queue_size))

    rospy = types.SimpleNamespace(
        init_node=lambda name, **k: log.__setitem__("node", name),
        has_param=lambda k: k in params, get_param=lambda k: params[k],
        Subscriber=lambda topic, klass, cb, queue_size=None: log["subscribed"].append(topic),
        Publisher=Publisher, loginfo=lambda *a: None, spin=lambda: None, Time=Msg)
    sensor = types.SimpleNamespace(PointCloud2=Msg, PointField=Msg)
    std = types.SimpleNamespace(Header=Msg, Float64MultiArray=Msg)
    nav = types.SimpleNamespace(Odometry=Msg, Path=Msg)
    geo = types.SimpleNamespace(Pose=Msg, PoseStamped=Msg)
    return rospy, sensor, std, nav, geo


@pytest.mark.parametrize("params, want", [({}, False), ({"~MAP_CLOUD": False}, False),
                                          ({"~MAP_CLOUD": True, "~RESULT_PATH": "/tmp/r.txt"}, True)])
def test_entry_map_cloud_param(monkeypatch, params, want):
    """mapOptmization in ROS mode: ~MAP_CLOUD turns the option on and advertises the topic; without
    it the node is built and wired exactly as before"""
    import torch
    from ssf import entry, nodes, rosbridge
    log = dict(advertised=[], subscribed=[], built=[])
    mods = _fake_ros(params, log)
    monkeypatch.setattr(rosbridge, "available", lambda: True)
    monkeypatch.setattr(rosbridge, "require", lambda: mods)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)

    class Node:
        def __init__(self, publish, **kw):
            log["built"].append(kw)

        def on_plane_cloud(self, msg):
            pass

    monkeypatch.setattr(nodes, "MapOptimizationNode", Node)
    entry.node_main("mapOptmization", ["__name:=mapOptmization"])
    assert log["node"] == "mapOptmization"
    base = [("map_odom_res3", 100), ("map_frame_res3", 10), ("map_laser_path_res3", 100)]
    assert log["advertised"] == base + ([("sum_map_cloud_res3", 10)] if want else [])
    kw = dict(device=0, tum_path=params.get("~RESULT_PATH"))
    assert log["built"] == [dict(kw, map_cloud=True) if want else kw]
    assert log["subscribed"] == ["/plane_frame_cloud2", "/frame_odom2"]

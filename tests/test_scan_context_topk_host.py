"""CPU checks of the top-K Scan Context selection and of the batched candidate verification's
wiring: the numpy yardstick tests/scan_context_topk_reference.py (which
k_sc_select_topk is held to in tests/test_gpu_scan_context_topk.py) on hand-built rows -- plain
K smallest, ties, the exclusion window, an exhausted prefix, n_eligible 0 and 1, NaN --, and every
argument error of the new Python and command-line surface that comes before a device call."""
import ctypes as C

import numpy as np
import pytest
import torch

import scan_context_reference as SR
import scan_context_topk_reference as TR


def _sel(dist, n, k, E, shift=None):
    shift = np.arange(100, 100 + len(dist)) if shift is None else shift
    i, d, s = TR.select_topk(np.array(dist, np.float32), shift, n, k, E)
    assert i.dtype == np.int32 and d.dtype == np.float32 and s.dtype == np.int32 and len(i) == len(d) == len(s) == k
    return i.tolist(), d.tolist(), s.tolist()


ROW = [0.50, 0.10, 0.30, 0.20, 0.40, 0.05, 0.60, 0.15]


def test_plain_k_smallest():
    """E = 0: the K smallest in the order (dist, index), dist and shift copied from the rows."""
    i, d, s = _sel(ROW, 8, 3, 0)
    assert i == [5, 1, 7] and s == [105, 101, 107]
    assert d == [float(np.float32(v)) for v in (0.05, 0.10, 0.15)]
    assert _sel(ROW, 8, 8, 0)[0] == [5, 1, 7, 3, 2, 4, 0, 6]
    assert _sel(ROW, 5, 3, 0)[0] == [1, 3, 2]                      # only the prefix is looked at
    i, d, s = _sel(ROW, 2, 4, 0)                                   # fewer candidates than K
    assert i == [1, 0, -1, -1] and d[2:] == [1.0, 1.0] and s[2:] == [0, 0]


def test_ties_go_to_the_lower_index():
    row = [0.3, 0.1, 0.1, 0.3, 0.1, 0.3]
    assert _sel(row, 6, 6, 0)[0] == [1, 2, 4, 0, 3, 5]
    assert _sel(row, 6, 2, 0)[0] == [1, 2]
    assert _sel([0.2] * 5, 5, 3, 0)[0] == [0, 1, 2]
    assert _sel([0.2] * 5, 5, 3, 1)[0] == [0, 2, 4]


def test_window_skips_neighbours_on_both_sides():
    #       0     1     2     3     4     5     6     7     8     9
    row = [0.90, 0.80, 0.11, 0.10, 0.12, 0.70, 0.13, 0.60, 0.50, 0.14]
    assert _sel(row, 10, 4, 0)[0] == [3, 2, 4, 6]
    # E = 1: 2 and 4 are neighbours of 3 (below and above); 6 is free; 9 is free
    assert _sel(row, 10, 4, 1)[0] == [3, 6, 9, 1]
    # E = 3: 0..6 are within 3 of 3; 9 (0.14) is next, then 8 and 7 are within 3 of 9
    assert _sel(row, 10, 4, 3)[0] == [3, 9, -1, -1]
    # the window is about every taken index, not only the first
    assert _sel(row, 10, 3, 2)[0] == [3, 6, 9]
    assert _sel(row, 10, 4, 2)[0] == [3, 6, 9, 0]


def test_window_exhausts_the_prefix_before_k():
    i, d, s = _sel(ROW, 8, 4, 8)                                   # everything is within 8 of the first
    assert i == [5, -1, -1, -1] and d[1:] == [1.0] * 3 and s == [105, 0, 0, 0]
    assert _sel(ROW, 8, 8, 3)[0] == [5, 1, -1, -1, -1, -1, -1, -1]
    assert _sel(ROW, 8, 3, 10 ** 9)[0] == [5, -1, -1]


def test_n_eligible_zero_and_one():
    for E in (0, 1, 3):
        for k in (1, 2, 8):
            i, d, s = _sel(ROW, 0, k, E)
            assert i == [-1] * k and d == [1.0] * k and s == [0] * k
            i, d, s = _sel(ROW, 1, k, E)
            assert i == [0] + [-1] * (k - 1) and d == [0.5] + [1.0] * (k - 1) and s == [100] + [0] * (k - 1)
    assert TR.select_topk(np.zeros(0, np.float32), np.zeros(0, np.int32), 0, 2, 0)[0].tolist() == [-1, -1]


def test_nan_counts_as_infinity_and_is_copied():
    nan = float("nan")
    i, d, s = _sel([nan, 0.4, nan, 0.2], 4, 4, 0)
    assert i == [3, 1, 0, 2] and d[:2] == [float(np.float32(0.2)), float(np.float32(0.4))]
    assert np.isnan(d[2]) and np.isnan(d[3]) and s == [103, 101, 100, 102]
    i, d, _ = _sel([nan, nan, nan], 3, 2, 1)                       # all NaN: index order, window applied
    assert i == [0, 2] and np.isnan(d).all()
    i, d, _ = _sel([nan, float("inf"), nan], 3, 3, 0)              # NaN ties with +inf: by index
    assert i == [0, 1, 2]


def test_k1_is_the_single_selection_for_every_window():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64, 300):
        row = rng.uniform(0, 1, n).astype(np.float32)
        row[rng.integers(0, n, n // 3)] = row[0]                   # ties
        if n > 2:
            row[1] = np.nan
        for n_el in {0, 1, n // 2, n}:
            for E in (0, 1, 3, n):
                i, d, s = TR.select_topk(row, np.arange(n), n_el, 1, E)
                assert i[0] == SR.select(row, n_el), (n, n_el, E)
                for k in (2, 8):                                    # and slot 0 does not depend on K
                    assert TR.select_topk(row, np.arange(n), n_el, k, E)[0][0] == i[0]


# ------------------------------------------------------------------------------ wiring
def test_loop_closer_argument_errors_before_any_device_call():
    """No context, no tensors: every ValueError comes from the constructor."""
    from ssf import loop
    for bad in (0, 9, -1, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="sc_candidates"):
            loop.LoopCloser(None, detector="scan_context", sc_candidates=bad)
    for bad in (-1, 1.5, "3", True):
        with pytest.raises(ValueError, match="sc_exclusion"):
            loop.LoopCloser(None, detector="scan_context", sc_exclusion=bad)
    with pytest.raises(ValueError, match="scan_context"):
        loop.LoopCloser(None, sc_candidates=2)
    with pytest.raises(ValueError, match="scan_context"):
        loop.LoopCloser(None, detector="radius", sc_exclusion=0)
    with pytest.raises(ValueError, match="scan_context"):
        loop.LoopCloser(None, detector="radius", sc_candidates=2, sc_exclusion=3)
    lc = loop.LoopCloser(None)
    assert (lc.detector, lc.sc_candidates, lc.sc_exclusion) == ("radius", 1, None)
    lc = loop.LoopCloser(None, detector="scan_context")
    assert (lc.sc_candidates, lc.sc_exclusion) == (1, None)
    for k in (1, 2, 8):
        for e in (None, 0, 10):
            lc = loop.LoopCloser(None, detector="scan_context", sc_candidates=k, sc_exclusion=e)
            assert (lc.sc_candidates, lc.sc_exclusion) == (k, e)
    assert loop.LoopConstraint(1, 0, np.eye(4), 0.1, np.eye(4)).candidates is None


def test_candidates_parsing_and_flag(capsys, tmp_path):
    """"K[:EXCLUSION]", and python -m ssf.run --map-sc-candidates: listed, refused with a clear
    message unless --map-detector scan-context is given, parsed before a device is looked for."""
    from ssf import nodes, run, scan_context as sc
    assert sc.parse_candidates("1") == (1, None) and sc.parse_candidates("4") == (4, None)
    assert sc.parse_candidates("8:0") == (8, 0) and sc.parse_candidates("2:25") == (2, 25)
    for bad in ("0", "9", "-1", "x", "", "2:", "2:-1", "2:x", "2.5", "2:1:3"):
        with pytest.raises(ValueError, match="candidates"):
            sc.parse_candidates(bad)
    with pytest.raises(SystemExit) as e:
        run.main(["--help"])
    assert e.value.code == 0 and "--map-sc-candidates" in capsys.readouterr().out
    m = ["--map-tum", str(tmp_path / "m.txt")]
    for argv in ([], m, m + ["--map-detector", "radius"]):
        with pytest.raises(SystemExit) as e:
            run.main([str(tmp_path)] + argv + ["--map-sc-candidates", "2"])
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--map-sc-candidates" in err and "scan-context" in err, argv
    for bad in ("0", "9", "2:-1", "two"):
        with pytest.raises(SystemExit) as e:
            run.main([str(tmp_path)] + m + ["--map-detector", "scan-context:0.2", "--map-sc-candidates", bad])
        assert e.value.code == 2 and "--map-sc-candidates" in capsys.readouterr().err
    for kw in (dict(map_sc_candidates=2), dict(map_sc_exclusion=3), dict(map_detector="radius", map_sc_candidates=2)):
        with pytest.raises(ValueError, match="map_sc_candidates"):
            nodes.run_sequence(str(tmp_path), None, map_tum_path="", **kw)


def test_node_argument_errors_before_any_device_call():
    """MapOptimizationNode refuses the two arguments without the scan-context detector and hands
    LoopCloser's refusals on; frontend= keeps it from creating a context."""
    from ssf import nodes
    fe = object()
    for kw in (dict(map_sc_candidates=2), dict(map_sc_exclusion=0), dict(map_detector="radius", map_sc_candidates=3)):
        with pytest.raises(ValueError, match="map_sc_candidates"):
            nodes.MapOptimizationNode(lambda *a: None, frontend=fe, **kw)
    for kw in (dict(map_sc_candidates=0), dict(map_sc_candidates=9)):
        with pytest.raises(ValueError, match="sc_candidates"):
            nodes.MapOptimizationNode(lambda *a: None, frontend=fe, map_detector="scan_context", **kw)
    with pytest.raises(ValueError, match="sc_exclusion"):
        nodes.MapOptimizationNode(lambda *a: None, frontend=fe, map_detector="scan_context", map_sc_exclusion=-2)
    n = nodes.MapOptimizationNode(lambda *a: None, frontend=fe, map_detector="scan_context", map_sc_candidates=4)
    assert (n.closer.sc_candidates, n.closer.sc_exclusion) == (4, None)
    n = nodes.MapOptimizationNode(lambda *a: None, frontend=fe, map_detector="scan_context", map_sc_candidates=2,
                                  map_sc_exclusion=25)
    assert (n.closer.sc_candidates, n.closer.sc_exclusion) == (2, 25)
    n = nodes.MapOptimizationNode(lambda *a: None, frontend=fe, map_detector="scan_context")
    assert (n.closer.sc_candidates, n.closer.sc_exclusion) == (1, None)


@pytest.mark.parametrize("params, extra", [
    ({"~MAP_DETECTOR": "scan-context:0.2", "~MAP_SC_CANDIDATES": "4"},
     dict(map_detector="scan_context", map_sc_threshold=0.2, map_sc_candidates=4, map_sc_exclusion=None)),
    ({"~MAP_DETECTOR": "scan-context", "~MAP_SC_CANDIDATES": "2:25"},
     dict(map_detector="scan_context", map_sc_threshold=None, map_sc_candidates=2, map_sc_exclusion=25)),
    ({"~MAP_SC_CANDIDATES": "2"}, None), ({"~MAP_DETECTOR": "radius", "~MAP_SC_CANDIDATES": "2"}, None),
    ({"~MAP_DETECTOR": "scan-context", "~MAP_SC_CANDIDATES": "9"}, None)])
def test_entry_map_sc_candidates_param(monkeypatch, params, extra):
    """mapOptmization in ROS mode: ~MAP_SC_CANDIDATES reaches the node with the scan-context
    detector and is refused without it or out of range (extra None)."""
    import types

    from ssf import entry, nodes, rosbridge
    built = []

    class Msg:
        pass

    rospy = types.SimpleNamespace(
        init_node=lambda name, **k: None, has_param=lambda k: k in params, get_param=lambda k: params[k],
        Subscriber=lambda topic, klass, cb, queue_size=None: None,
        Publisher=lambda topic, klass, queue_size=None: None, loginfo=lambda *a: None, spin=lambda: None, Time=Msg)
    mods = (rospy, types.SimpleNamespace(PointCloud2=Msg, PointField=Msg),
            types.SimpleNamespace(Header=Msg, Float64MultiArray=Msg), types.SimpleNamespace(Odometry=Msg, Path=Msg),
            types.SimpleNamespace(Pose=Msg, PoseStamped=Msg))
    monkeypatch.setattr(rosbridge, "available", lambda: True)
    monkeypatch.setattr(rosbridge, "require", lambda: mods)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)

    class Node:
        def __init__(self, publish, **kw):
            built.append(kw)

        def on_plane_cloud(self, msg):
            pass

        def on_scan(self, msg):
            pass

    monkeypatch.setattr(nodes, "MapOptimizationNode", Node)
    if extra is None:
        with pytest.raises(ValueError, match="MAP_SC_CANDIDATES|candidates"):
            entry.node_main("mapOptmization", ["__name:=mapOptmization"])
        assert built == []
    else:
        entry.node_main("mapOptmization", ["__name:=mapOptmization"])
        assert built == [dict(device=0, tum_path=None, **extra)]


def test_match_topk_and_query_topk_argument_errors():
    """k and exclusion out of range: ValueError before the tensors are even looked at."""
    from ssf import _abi, scan_context as sc
    assert _abi.SC_MAX_TOPK == 8
    q = torch.zeros(2, 20, 60)                                     # CPU tensors: a device call would refuse them
    for k, e in ((0, 0), (9, 0), (-1, 0), (2, -1), (2.0, 0), (2, 1.5), ("2", 0), (True, 0), (None, 0)):
        with pytest.raises(ValueError):
            sc.match_topk(None, q, q, 2, k, e)
        with pytest.raises(ValueError):
            sc.ScanContextDB(None).query_topk(q[0], k, e)
    with pytest.raises(_abi.SSFError):                              # in range: the tensors are checked next
        sc.match_topk(None, q, q, 2, 2, 0)


def test_arg_errors_without_gpu():
    """SSF_E_ARG on the null context, before any HIP call; the symbol is exported and bound."""
    from ssf import _abi
    L = _abi.lib()
    assert "ssf_scan_context_match_topk" in _abi.EXPORTS
    f = L.ssf_scan_context_match_topk
    assert len(f.argtypes) == 13 and f.restype is C.c_int32
    assert f(None, None, 1, None, 1, None, None, None, None, None, None, 2, 0) == _abi.SSF_E_ARG

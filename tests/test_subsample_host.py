"""CPU checks of the ActiveSceneFlow wiring: the sampler's numpy yardstick (tests/subsample_reference.py,
which the kernel must equal bit for bit, tests/test_gpu_subsample.py) -- its key formula against the
textbook sequential generator and its uniformity --, the SSF_E_ARG paths of ssf_subsample_batch,
load_checkpoint, the two ASF entry scripts and the launch-graph table."""
import os
import subprocess
import sys

import numpy as np
import pytest

import subsample_reference as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(REPO, "ssf-slam_amd", "scripts")


@pytest.mark.parametrize("seed,tag,stream", [(1234, 0, 0), (1234, 7, 1), (0, 0, 0), (2 ** 64 - 1, 2 ** 63 + 5, 1)])
def test_random_access_keys_equal_the_sequential_generator(seed, tag, stream):
    for bits in (32, 4, 1):
        a = SR.keys_sequential(seed, tag, stream, 500, bits)
        b = SR.keys_random_access(seed, tag, stream, 500, bits)
        assert np.array_equal(a, b)
        assert int(a.max()) < (1 << bits)
    # the textbook generator itself: SplitMix64 seeded with 1234567 (the constants' published vector)
    g = SR.SplitMix64(1234567)
    assert [g.next() for _ in range(3)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]


def test_selection_is_the_lexsort_and_ties_break_by_index():
    pts = np.zeros((300, 3), np.float32)
    for bits in (4, 1):
        keys = SR.keys_random_access(9, 3, 0, 300, bits)
        assert len(np.unique(keys)) <= (1 << bits)
        idx, _, n, st = SR.subsample(pts, 64, 9, 3, key_bits=bits)
        assert (n, st) == (300, SR.OK)
        k = keys[idx].astype(np.int64)
        assert np.all((np.diff(k) > 0) | ((np.diff(k) == 0) & (np.diff(idx) > 0)))
        assert len(set(idx.tolist())) == 64


def test_uniformity_of_the_yardstick():
    """n = 64, nb = 16, seed 1234, tags 0..3999: inclusion counts, first-slot counts and the
    with-replacement hit counts stay within 5 standard deviations of their means."""
    n, nb, T = 64, 16, 4000
    pts = np.zeros((n, 3), np.float32)
    incl = np.zeros(n)
    first = np.zeros(n)
    for tag in range(T):
        idx = SR.subsample(pts, nb, 1234, tag)[0]
        incl[idx] += 1
        first[idx[0]] += 1
    sd = np.sqrt(T * 0.25 * 0.75)
    dev_incl = np.abs(incl - 1000).max() / sd
    sd1 = np.sqrt(T * (1 / 64) * (63 / 64))
    dev_first = np.abs(first - 62.5).max() / sd1
    # the with-replacement rule's ranks (key(1, j) n) >> 32 for 16 slots over n = 64: hits per rank
    hits = np.zeros(n)
    for tag in range(T):
        k1 = SR.keys_random_access(1234, tag, 1, nb, 32)
        np.add.at(hits, ((k1 * np.uint64(n)) >> np.uint64(32)).astype(np.int64), 1)    # ranks repeat
    sdr = np.sqrt(T * 16 * (1 / 64) * (63 / 64))
    dev_hits = np.abs(hits - 1000).max() / sdr
    print(f"[subsample host] inclusion {dev_incl:.2f} sd, first slot {dev_first:.2f} sd, replacement {dev_hits:.2f} sd")
    assert dev_incl <= 5 and dev_first <= 5 and dev_hits <= 5


def test_consecutive_tags_are_independent():
    """mean overlap of consecutive tags' samples, n = 1000, nb = 100, 200 tags: 100 * 100 / 1000 = 10"""
    pts = np.zeros((1000, 3), np.float32)
    s = [set(SR.subsample(pts, 100, 1234, tag)[0].tolist()) for tag in range(200)]
    ov = np.mean([len(a & b) for a, b in zip(s[:-1], s[1:])])
    print(f"[subsample host] mean overlap of consecutive tags {ov:.2f}")
    assert 9 <= ov <= 11


def test_with_replacement_and_quota_follow_the_definition():
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((50, 3)).astype(np.float32)
    idx, xyz, n, st = SR.subsample(pts, 50, 5, 2)              # n == nb resamples
    assert st == SR.OK and len(set(idx.tolist())) < 50
    assert np.array_equal(xyz, pts[idx].T)
    cls = np.zeros(50, np.uint8)
    cls[[3, 9, 11]] = 1
    idx, _, _, st = SR.subsample(pts, 20, 5, 2, cls=cls, quota=2)
    assert st == SR.OK and set(idx[:2].tolist()) <= {3, 9, 11} and not (set(idx[2:].tolist()) & {3, 9, 11})
    assert SR.subsample(pts, 49, 5, 2, cls=cls, quota=1)[3] == SR.SHORT     # 47 background < 48
    assert SR.subsample(pts, 48, 5, 2, cls=cls, quota=1)[3] == SR.OK
    assert SR.subsample(pts, 8, 5, 2, z_min=100.0)[2:] == (0, SR.EMPTY)
    nan = pts.copy()
    nan[:, 2] = np.nan
    assert SR.subsample(nan, 8, 5, 2, z_min=100.0)[2:] == (50, SR.OK)       # a NaN z survives


def test_subsample_arg_errors_without_gpu():
    """bad shapes are SSF_E_ARG before any HIP call (no context can exist without a device, so
    every one of them is tried on the null context; tests/test_gpu_subsample.py repeats them on a
    live one)"""
    from ssf import _abi
    L = _abi.lib()
    good = dict(nb=16, stride=3, quota=-1, key_bits=32)
    for kw in (dict(), dict(nb=0), dict(nb=8193), dict(stride=2), dict(quota=5), dict(key_bits=0),
               dict(key_bits=33)):
        a = dict(good, **kw)
        rc = L.ssf_subsample_batch(None, None, 1, None, a["stride"], None, None, None, a["nb"], -3.3, 0,
                                   a["quota"], 1234, None, a["key_bits"], None, None, None, None)
        assert rc == _abi.SSF_E_ARG
    assert (_abi.SAMPLE_MAX_NB, _abi.SAMPLE_MAX_POINTS) == (8192, 1 << 24)
    assert (SR.OK, SR.EMPTY, SR.SHORT) == (_abi.SAMPLE_OK, _abi.SAMPLE_EMPTY, _abi.SAMPLE_SHORT)


@pytest.mark.parametrize("prefix", ["", "module."])
def test_load_checkpoint_round_trip(tmp_path, prefix):
    import torch
    from cv_reference import seed_state
    from ssf import asf
    from ssf.tflow import RefineFlowRegressor
    net = RefineFlowRegressor(4, 8, 0, [8, 8], [8], use_flow=False)
    sd = net.state_dict()
    want = seed_state([(k, v.shape) for k, v in sd.items()], 21)
    path = str(tmp_path / "ckpt.t7")
    torch.save({prefix + k: torch.from_numpy(v) for k, v in want.items()}, path)
    fresh = RefineFlowRegressor(4, 8, 0, [8, 8], [8], use_flow=False)
    assert asf.load_checkpoint(fresh, path) is fresh
    got = fresh.state_dict()
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert np.array_equal(got[k].numpy(), v), k
    bad = dict(want)
    bad.pop(sorted(bad)[0])
    torch.save({prefix + k: torch.from_numpy(v) for k, v in bad.items()}, path)
    with pytest.raises(RuntimeError):                                  # strict=True
        asf.load_checkpoint(fresh, path)


@pytest.mark.parametrize("exe", ["main_sju_occ_ros.py", "main_sju_occ_addSeg_ros.py"])
def test_asf_launch_targets_exist_and_refuse_without_ros(exe):
    path = os.path.join(SCRIPTS, exe)
    assert os.access(path, os.X_OK)
    # roslaunch appends __name:= / __log:= arguments: they must not break the parser
    r = subprocess.run([sys.executable, path, "__name:=x", "__log:=/tmp/x.log"], capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode != 0
    assert "rospy is not importable" in r.stderr


def test_launch_graphs():
    from ssf import nodes
    g = nodes.LAUNCH_GRAPHS
    assert sorted(g) == ["Seg", "Seg_ActiveSceneFlow", "noSeg", "noSeg_ActiveSceneFlow", "onlyPC"]
    assert g["onlyPC"] == ("none", "registration", ("pos1",))
    assert g["noSeg"] == ("gmm", "ingest", ("pos1", "gt"))
    assert g["Seg"] == ("gt", "ingest", ("pos1", "gt", "s_fg_mask"))
    assert g["noSeg_ActiveSceneFlow"][:3] == ("gmm", "ingest", ("pos1", "pos2"))
    assert g["Seg_ActiveSceneFlow"][:3] == ("gt", "ingest", ("pos1", "pos2", "s_fg_mask"))
    assert set(g["noSeg_ActiveSceneFlow"][3]) == {"gt", "s_fg_mask", "t_fg_mask"}
    with pytest.raises(ValueError, match="weights"):
        nodes._asf_net(None, 2048, "cpu")

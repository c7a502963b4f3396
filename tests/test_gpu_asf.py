"""The ActiveSceneFlow chain (ssf.asf) on the GPU: TFlow with seeded weights (tests/cv_reference.seed_state;
no trained weights exist here), n_points = 2048, raw clouds of 3000 points, about 5 % foreground.

The binding check of the wiring is bit-equality with the hand composition -- TFlow forward, then
ssf.mask_and_pose(points, flow, draws=..., kabsch_dtype="float32") on copies.  The pose itself is held
to the yardsticks the ASF block already has: mode 'gt' against tests/rigid_reference.kabsch in float32
with the k_kabsch_f32 rule of tests/test_gpu_rigid_tails.py (device error <= FACTOR x numpy's own
float32 error, over the launch), mode 'gmm' against the CPU oracle's float32 restatement in the form of
test_gpu_mask.test_asf_f32_kabsch_tail.  Seeded weights give a flow with no real structure, so the GMM's
mask agreement with the oracle is printed, not asserted."""
import os

import numpy as np
import pytest
import torch

import rigid_reference as RR
import subsample_reference as SR

pytestmark = pytest.mark.gpu
NP, RAW, SEED = 2048, 3000, 1234
DRAWS = np.array([[0.3, 0.6, 0.9], [0.15, 0.45, 0.8]])


def _raw_pair(k):
    rng = np.random.default_rng(100 + k)
    pos1 = (rng.uniform(-1, 1, (RAW, 3)) * [8.0, 8.0, 2.0]).astype(np.float32)
    a = 0.02 + 0.005 * k
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    pos2 = (pos1 @ Rz.T + [0.3, 0.05, 0.0] + rng.standard_normal((RAW, 3)) * 0.01).astype(np.float32)
    fg1 = (rng.uniform(size=RAW) < 0.05).astype(np.uint8)
    fg2 = (rng.uniform(size=RAW) < 0.05).astype(np.uint8)
    return dict(pos1=pos1, pos2=pos2, gt=(pos2 - pos1).astype(np.float32), s_fg_mask=fg1, t_fg_mask=fg2)


@pytest.fixture(scope="module")
def state():
    import ssf
    from cv_reference import seed_state
    sd = ssf.TFlow().state_dict()
    return {k: torch.from_numpy(v) for k, v in seed_state([(k, v.shape) for k, v in sd.items()], 31).items()}


@pytest.fixture(scope="module")
def net(state, dev):
    import ssf
    n = ssf.TFlow()
    n.load_state_dict(state, strict=True)
    return n.to(dev)


@pytest.fixture(scope="module")
def fe(dev):
    import ssf
    return ssf.Frontend(64, device=dev.index or 0)


@pytest.fixture(scope="module")
def pairs(dev):
    """two network inputs: pc1 / pc2 [2, 3, NP] and fg1 [2, NP], the first NP raw points of each pair"""
    raw = [_raw_pair(k) for k in range(2)]
    pc1 = torch.from_numpy(np.stack([r["pos1"][:NP].T for r in raw])).contiguous().to(dev)
    pc2 = torch.from_numpy(np.stack([r["pos2"][:NP].T for r in raw])).contiguous().to(dev)
    fg1 = torch.from_numpy(np.stack([r["s_fg_mask"][:NP] for r in raw])).to(dev)
    return pc1, pc2, fg1


@pytest.fixture(scope="module")
def chain(net, fe, pairs):
    """flow_mask_pose on the two pairs, both modes, computed once: mode -> (out, bg, flow) numpy"""
    from ssf import asf
    pc1, pc2, fg1 = pairs
    res = {}
    for mode in ("gmm", "gt"):
        out, bg, flow = asf.flow_mask_pose(net, fe, pc1, pc2, mode=mode, fg1=fg1 if mode == "gt" else None,
                                           draws=DRAWS if mode == "gmm" else None)
        torch.cuda.synchronize()
        res[mode] = (out.cpu().numpy(), bg.cpu().numpy(), flow.cpu().numpy())
    return res


@pytest.mark.parametrize("mode", ["gmm", "gt"])
def test_flow_mask_pose_is_the_hand_composition(net, fe, pairs, chain, mode, dev):
    import ssf
    from ssf import asf
    pc1, pc2, fg1 = pairs
    out, bg, flow = chain[mode]
    # the TFlow forward, pair by pair as flow_mask_pose runs it; how far a batched forward is from
    # it is printed (0 in three of four runs, 2e-7 in one), not asserted: that is TFlow's, not the wiring's
    hand = torch.cat([net(pc1[b:b + 1], pc2[b:b + 1])[0][0] for b in range(2)])
    assert np.array_equal(hand.cpu().numpy(), flow)
    batched = net(pc1, pc2)[0][0]
    print(f"[asf] TFlow B = 2 forward against two B = 1 forwards: max |d flow| {float((batched - hand).abs().max()):.3e}")
    pts = pc1.permute(0, 2, 1).reshape(-1, 3).clone()
    fl = hand.permute(0, 2, 1).reshape(-1, 3).clone()
    kw = dict(draws=DRAWS) if mode == "gmm" else dict(mode="gt", gt_mask=fg1.reshape(-1).clone())
    res = ssf.mask_and_pose(pts, fl, frame_sizes=[NP, NP], kabsch_dtype="float32", errors="status",
                            device=dev.index or 0, **kw)
    assert np.array_equal(res["para_t_q"], out[:, 0:7])
    assert np.array_equal(res["R"].reshape(-1, 9), out[:, 7:16])
    assert np.array_equal(res["info"]["status"], out[:, 16].astype(np.int32))
    assert np.array_equal(res["info"]["n_bg"], out[:, 17]) and np.array_equal(res["info"]["em_iter"], out[:, 20])
    assert np.array_equal(res["bg_mask"].cpu().numpy(), bg)
    if mode == "gt":
        assert np.array_equal(bg, (fg1.reshape(-1).cpu().numpy() == 0).astype(np.uint8))
    # B = 2 is two B = 1 calls
    for b in range(2):
        o1, bg1, f1 = asf.flow_mask_pose(net, fe, pc1[b:b + 1], pc2[b:b + 1], mode=mode,
                                         fg1=fg1[b:b + 1] if mode == "gt" else None,
                                         draws=DRAWS[b:b + 1] if mode == "gmm" else None)
        assert np.array_equal(f1.cpu().numpy()[0], flow[b])
        assert np.array_equal(bg1.cpu().numpy(), bg[b * NP:(b + 1) * NP])
        assert np.array_equal(o1.cpu().numpy()[0, :25], out[b, :25])
    with pytest.raises(ValueError):
        asf.flow_mask_pose(net, fe, pc1, pc2, mode="gt")


def test_mode_gt_pose_against_the_float32_kabsch_yardstick(pairs, chain):
    from test_gpu_rigid_tails import _e_ref_check
    pc1, _, fg1 = pairs
    out, bg, flow = chain["gt"]
    p = pc1.cpu().numpy()
    R64, t64, R32, t32, q64, q32, good = [], [], [], [], [], [], []
    for b in range(2):
        d32 = np.ascontiguousarray(p[b].T)
        f32 = np.ascontiguousarray(flow[b].T)
        m = bg[b * NP:(b + 1) * NP]
        assert out[b, 17] == m.sum() and out[b, 16] in (0, -3)
        Rr, tr, det = RR.kabsch((d32 + f32).astype(np.float64), d32.astype(np.float64), mask=m)
        Rf, tf, _ = RR.kabsch(d32 + f32, d32, mask=m, dtype=np.float32)
        assert det > 0
        R64.append(Rr), t64.append(tr), R32.append(Rf.astype(np.float64)), t32.append(tf.astype(np.float64))
        if out[b, 16] == 0:
            good.append(b)
            q64.append(RR.quat_xyzw(Rr)[0])
            q32.append(np.asarray(RR.quat_xyzw(Rf, dtype=np.float32)[0], np.float64))
    _e_ref_check("asf gt R", [out[b, 7:16].reshape(3, 3) for b in range(2)], R64, R32)
    _e_ref_check("asf gt t", [out[b, 0:3] for b in range(2)], t64, t32)
    if good:
        _e_ref_check("asf gt q", [out[b, 3:7] for b in good], q64, q32)
    assert np.array_equal(out[:, 7:16], out[:, 7:16].astype(np.float32))       # float32 values
    assert np.array_equal(out[:, 0:3], out[:, 0:3].astype(np.float32))


def test_mode_gmm_pose_against_the_oracle(oracle, pairs, chain):
    pc1, _, _ = pairs
    out, bg, flow = chain["gmm"]
    p = pc1.cpu().numpy()
    for b in range(2):
        pts, fl = np.ascontiguousarray(p[b].T), np.ascontiguousarray(flow[b].T)
        ref = oracle.mask_and_pose(pts, fl, DRAWS[b], kabsch_dtype="float32")
        m = bg[b * NP:(b + 1) * NP]
        agree = (m == ref["bg_mask"]).mean()
        print(f"[asf] gmm pair {b}: mask agreement with the oracle {agree:.6f}, device status {int(out[b, 16])}, "
              f"oracle rc {ref['rc']}, em_iter {int(out[b, 20])}")
        if np.array_equal(m, ref["bg_mask"]):           # same rows: the same float32 arithmetic
            assert int(out[b, 16]) == ref["rc"]
            assert np.abs(out[b, 7:16].reshape(3, 3) - ref["R"]).max() < 1e-6
            assert np.abs(out[b, 0:3] - ref["t"]).max() < 1e-6
            assert np.abs(out[b, 3:7] - ref["q_xyzw"]).max() < 1e-6
        assert np.array_equal(out[b, 7:16], out[b, 7:16].astype(np.float32))
        assert int(out[b, 20]) >= 1 and out[b, 17] == m.sum()


def test_node_publishes_the_sampled_cloud_and_a_pose(net, fe):
    from ssf import asf, nodes
    from ssf import io as sio
    bus = nodes.Bus(keep=8)
    node = asf.ActiveSceneFlowNode(bus.publish, net, frontend=fe, mode="gmm", n_points=NP, seed=SEED)
    r = _raw_pair(0)
    o, metrics = node.on_pair(r["pos1"], r["pos2"], (3, 4), fg1=r["s_fg_mask"], fg2=r["t_fg_mask"], gt_flow=r["gt"])
    clouds, odoms = bus.log["/velodyne_points"], bus.log["/frame_odom1"]
    assert len(clouds) == 1 and len(odoms) == 1
    msg = clouds[0]
    assert (msg.point_step, msg.width, msg.height, msg.header.frame_id) == (12, NP, 1, "livox_frame")
    assert sio.stamp_of(msg.header) == (3, 4)
    # the yardstick's two stages: the quota of 100 to NP, then the choice on exactly NP survivors
    final = []
    for c, (pos, fg) in enumerate(((r["pos1"], r["s_fg_mask"]), (r["pos2"], r["t_fg_mask"]))):
        i1, _, n1, st1 = SR.subsample(pos, NP, SEED, c, cls=fg, quota=100)
        assert st1 == SR.OK and fg[i1].tolist() == [1] * 100 + [0] * (NP - 100)
        i2, _, n2, st2 = SR.subsample(pos[i1], NP, SEED, c + 2 ** 63)
        assert (n2, st2) == (NP, SR.OK) and len(set(i2.tolist())) < NP      # with replacement: duplicates
        final.append(i1[i2])
    assert np.array_equal(sio.cloud_xyz(msg), r["pos1"][final[0]])
    assert np.array_equal(node.last["idx"].cpu().numpy(), np.stack(final))
    assert np.array_equal(node.last["xyz"][1].cpu().numpy(), r["pos2"][final[1]].T)
    data = odoms[0].data
    assert len(data) == 7 and np.isfinite(data).all() and np.array_equal(data, o[0:7])
    assert set(metrics) == {"epe3d", "acc3d_strict", "acc3d_relax", "outlier"}
    want = asf.flow_metrics(node.last["flow"], torch.from_numpy(r["gt"][final[0]].T[None]).to(fe.device))
    assert metrics == want
    # without masks: the second stage alone, pair 1 -> tags 2 and 3 (+ 2^63), without replacement
    node.on_pair(r["pos1"], r["pos2"], (3, 5))
    i = SR.subsample(r["pos1"], NP, SEED, 2 + 2 ** 63)[0]
    assert len(set(i.tolist())) == NP
    assert np.array_equal(sio.cloud_xyz(bus.log["/velodyne_points"][1]), r["pos1"][i])
    # mode 'gt' needs the mask of cloud 1
    import ssf
    with pytest.raises(ssf.SSFError):
        asf.ActiveSceneFlowNode(bus.publish, net, frontend=fe, mode="gt", n_points=NP).on_pair(r["pos1"], r["pos2"])


def _error_f64(pred, gt, mask=None):
    """error() of the reference's test loop restated in numpy float64: pred / gt [B, 3, N]"""
    p = np.transpose(pred, (0, 2, 1)).astype(np.float64)
    g = np.transpose(gt, (0, 2, 1)).astype(np.float64)
    m = np.ones(p.shape[:2]) if mask is None else np.asarray(mask, np.float64)
    l2 = np.sqrt(((g - p) ** 2).sum(-1)) * m
    sf = np.sqrt((g ** 2).sum(-1)) * m
    msum = m.sum(1)
    epe = (l2.sum(1) / (msum + 1e-10)).mean()
    rel = l2 / (sf + 1e-10)
    out = [epe]
    for a, b in (((l2 < 0.05), (rel < 0.05)), ((l2 < 0.1), (rel < 0.1)), ((l2 >= 0.3), (rel >= 0.1))):
        cnt = np.logical_or(a * m, b * m).sum(1).astype(np.float64)
        out.append((cnt[msum > 0] / msum[msum > 0]).mean())
    return out, l2, rel


def test_flow_metrics(dev):
    from ssf import asf
    rng = np.random.default_rng(77)
    B, N = 2, 4096

    def vec(mag):
        v = rng.standard_normal((B, 3, N))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * mag[:, None, :]

    gt = vec(np.exp(rng.uniform(np.log(0.05), np.log(5.0), (B, N)))).astype(np.float32)
    pred = (gt + vec(np.exp(rng.uniform(np.log(0.005), np.log(1.0), (B, N))))).astype(np.float32)
    # reject points whose error or relative error lies within 1e-4 (relative) of a threshold
    _, l2, rel = _error_f64(pred, gt)
    near = np.zeros((B, N), bool)
    for t in (0.05, 0.1, 0.3):
        near |= (np.abs(l2 - t) <= 1e-4 * t) | (np.abs(rel - t) <= 1e-4 * t)
    pred[np.broadcast_to(near[:, None, :], pred.shape)] = gt[np.broadcast_to(near[:, None, :], gt.shape)]
    mask = (rng.uniform(size=(B, N)) < 0.7).astype(np.float32)
    for m in (None, mask):
        want, _, _ = _error_f64(pred, gt, m)
        got = asf.flow_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev),
                               None if m is None else torch.from_numpy(m).to(dev))
        g = [got[k] for k in ("epe3d", "acc3d_strict", "acc3d_relax", "outlier")]
        assert abs(g[0] - want[0]) <= 1e-12 * want[0]
        assert g[1:] == want[1:]
        assert 0 < want[1] < want[2] < 1 and 0 < want[3] < 1


def test_run_sequence_asf_launch(tmp_path, state, dev, capsys):
    import ssf
    from ssf import nodes
    root = tmp_path / "seq"
    root.mkdir()
    raws = [_raw_pair(k) for k in range(3)]
    for k, r in enumerate(raws):
        np.savez(str(root / f"{k:06d}.npz"), **r)
    ckpt = str(tmp_path / "model.best.t7")
    torch.save({"module." + k: v for k, v in state.items()}, ckpt)
    tum = [str(tmp_path / f"traj{i}.txt") for i in range(2)]
    res = [nodes.run_sequence(str(root), t, launch="noSeg_ActiveSceneFlow", weights=ckpt, n_points=NP, device=dev)
           for t in tum]
    a = res[0]
    assert a["odom1"].shape == (3, 7) and a["odom2"].shape == (2, 7) and np.isfinite(a["odom1"]).all()
    assert len(a["flow_metrics"]) == 3
    lines = open(tum[0]).read().splitlines()
    assert len(lines) == 2
    assert open(tum[0], "rb").read() == open(tum[1], "rb").read()
    assert np.array_equal(a["odom1"], res[1]["odom1"]) and np.array_equal(a["odom2"], res[1]["odom2"])
    with pytest.raises(ValueError, match="weights"):
        nodes.run_sequence(str(root), None, launch="noSeg_ActiveSceneFlow", device=dev)
    # python -m ssf.run: the same trajectory, and the mean of each flow metric in its JSON line
    import json
    from ssf import run
    cli = str(tmp_path / "cli.txt")
    run.main([str(root), "--launch", "noSeg_ActiveSceneFlow", "--weights", ckpt, "--n-points", str(NP), "--tum", cli])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert open(cli, "rb").read() == open(tum[0], "rb").read()
    assert (line["launch"], line["odom1_poses"], line["odom2_poses"]) == ("noSeg_ActiveSceneFlow", 3, 2)
    for k in ("epe3d", "acc3d_strict", "acc3d_relax", "outlier"):
        assert line["flow_metrics"][k] == sum(m[k] for m in a["flow_metrics"]) / 3
    with pytest.raises(SystemExit):
        run.main([str(root), "--launch", "noSeg_ActiveSceneFlow"])
    # the Seg launch needs s_fg_mask
    bare = tmp_path / "bare"
    bare.mkdir()
    np.savez(str(bare / "000000.npz"), pos1=raws[0]["pos1"], pos2=raws[0]["pos2"])
    with pytest.raises(ssf.SSFError, match="s_fg_mask"):
        nodes.run_sequence(str(bare), None, launch="Seg_ActiveSceneFlow", weights=ckpt, n_points=NP, device=dev)
    # the existing launches are untouched: noSeg on the same directory = the node driven by hand
    old = nodes.run_sequence(str(root), None, launch="noSeg", seed=5, device=dev)
    rows = []
    pco = nodes.PointCloudOdometryNode(lambda topic, msg: None, device=dev, seed=5, mode="gmm")
    for r in raws:
        rows.append(pco.on_frame(r["pos1"], r["gt"], (0, 0))[0:7])
    assert np.array_equal(old["odom1"], np.stack(rows)) and old["odom2"].shape == (2, 7)
    assert "flow_metrics" not in old

"""The context's life cycle through the C ABI: its scratch, draw slots, pinned staging and events
are created by ordinary launches, released by ssf_destroy, and the 4-slot draw ring wraps and
grows without changing a result."""
import numpy as np
import pytest
import torch

from helpers import frame

pytestmark = pytest.mark.gpu

DRAWS = np.array([[0.3, 0.6, 0.9], [0.11, 0.52, 0.93], [0.7, 0.2, 0.4]])


def _mask(fe, dev, fr):
    import ssf
    pts = torch.from_numpy(np.concatenate([f[0] for f in fr])).to(dev)
    fl = torch.from_numpy(np.concatenate([f[1] for f in fr])).to(dev)
    off, h_off = ssf.frame_offsets([f[0].shape[0] for f in fr], dev)
    out, bg = fe.mask_pose(pts, fl, off, h_off, mode="gmm", draws=DRAWS[:len(fr)])
    torch.cuda.synchronize()
    return out.cpu().numpy(), bg.cpu().numpy()


def _register(fe, dev):
    import ssf
    clouds = [frame(0, k, n_az=300)[0] for k in range(2)]
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    off, h_off = ssf.frame_offsets([c.shape[0] for c in clouds], dev)
    pb = fe.extract_planes_batch(pts, off, h_off)
    table = fe.plane_table(pb)
    last = ssf.PlaneBatch(pb.xyzi, pb.count[0:1], off[0:2], h_off[0:2], pb.max_points)
    curr = ssf.PlaneBatch(pb.xyzi, pb.count[1:2], off[1:3].contiguous(), h_off[1:3].contiguous(), pb.max_points)
    res = fe.register(last, table, curr, ssf.identity_poses(1, dev))
    torch.cuda.synchronize()
    return res["pose_rel"].cpu().numpy()


def test_context_lifecycle(dev):
    """Three rounds of create / launch / close: a split GMM mask launch (draws, Lloyd records,
    sync words, exchange slots, pinned staging, both events) and extract -> plane table ->
    register (feature and registration scratch) give the same bits every round.  Then five mask
    launches of 1, 2, 1, 3 and 2 frames on one context -- the fifth wraps the ring onto the
    first launch's slot and grows it -- each equal to the same launch on a fresh context."""
    import ssf
    fr = [frame(s, k, n_az=8) for s, k in ((1, 0), (2, 3), (3, 1))]      # 512 points each

    def fresh(n):
        fe = ssf.Frontend(64, device=dev.index)
        fe.mask_split(2)
        out, bg = _mask(fe, dev, fr[:n])
        return fe, out, bg

    rounds = []
    for _ in range(3):
        fe, out, bg = fresh(2)
        pose = _register(fe, dev)
        torch.cuda.synchronize()
        fe.close()
        rounds.append((out, bg, pose))
    assert np.all(rounds[0][0][:, 16] == 0)                              # the fits ran
    for out, bg, pose in rounds[1:]:
        assert np.array_equal(out.view(np.uint64), rounds[0][0].view(np.uint64))
        assert np.array_equal(bg, rounds[0][1])
        assert np.array_equal(pose.view(np.uint64), rounds[0][2].view(np.uint64))

    ref = {}
    for n in (1, 2, 3):
        fe, ref_out, ref_bg = fresh(n)
        fe.close()
        ref[n] = (ref_out, ref_bg)
    fe = ssf.Frontend(64, device=dev.index)
    fe.mask_split(2)
    for n in (1, 2, 1, 3, 2):
        out, bg = _mask(fe, dev, fr[:n])
        assert np.array_equal(out.view(np.uint64), ref[n][0].view(np.uint64)), n
        assert np.array_equal(bg, ref[n][1]), n
    fe.close()

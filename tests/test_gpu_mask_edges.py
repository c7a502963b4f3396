"""k_mask_pose against sklearn on tiny, tied and degenerate frames (tests/golden/gmm_edges.npz, see
tests/golden/make_golden_gmm_edges.py for the families and tests/test_gmm_edges_host.py for the
bars; the CPU oracle is held to the same file without a GPU).

One launch per (storage, split) holds all fixtures as one ragged batch: float32 and float64
storage, ssf_set_mask_split 1, 2, 3, 8 and 0 (automatic).  A part of a frame is a multiple of
128 records (chunk = ((n + G - 1) / G + 127) / 128 * 128), so under a split most of these frames
leave whole parts without a point, and n = 129, 257 leave a part with one lone point.

What a kernel that mishandled a family would fail:
  size_n*      a part, wave or thread without a point that still adds to a sum, or a lone point
               dropped by the pair loop: CENTER0/1 (k-means++ scan over empty waves and parts),
               KM_ITER (Lloyd sums and changed counts), EM_ITER and LOWER_BOUND (EM sums), the mask
               and NBG (final pass, the clamped slot of an empty part); n = 2, 3, 5: also the rank
               rules of the pose on one, two and four background rows
  tie_*        the tie rule of Counter.most_common: BGLABEL and the whole mask (inverted when the
               label of point 0 does not reach a part that does not stream point 0)
  one label    an empty Lloyd cluster or n1 = 0 in the final pass: KM_ITER, the mask, NBG, BGLABEL;
               covariances of reg_covar alone (precisions ~1e6): EM_ITER, CONVERGED, LOWER_BOUND
  far_2000     cancellation in the moments about the mean 5 km out: LOWER_BOUND, t within 1e-5
  long_em      an E-step or M-step error that grows over 21 iterations: EM_ITER, LOWER_BOUND
LOWER_BOUND is held to 1e-9 on every fixture but the seven with a label of coincident rows beside
another label (n = 2, 3, 5 and the point masses): there the kernel's sum cancels terms of
0.5e6 d^2 and the bar is the bound derived in test_gmm_edges_host.device_lower_bound_bar
(measured 1.1e-10 .. 1.4e-8; every other field of those fixtures is held to equality as elsewhere).
Every frame is also launched alone at the same split and must give the same bits as in the batch
(a frame reading its neighbour's points or LDS state, ticket reuse); at the automatic split the
lone launch runs on 32 parts and is held to the fixture instead.
"""
import functools

import numpy as np
import pytest
import torch

from rigid_reference import rot_from_quat
from test_gmm_edges_host import NAMES, check_fit, check_pose, device_lower_bound_bar, edge_fixtures

pytestmark = pytest.mark.gpu

SPLITS = [1, 2, 3, 8, 0]
STORAGE = {"f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}


def _o(name):
    from ssf import _abi
    return _abi.POSE_OUT[name]


@functools.lru_cache(maxsize=None)
def _frontend(G, queue=0):
    import ssf
    fe = ssf.Frontend(64, device=0)
    fe.mask_split(G)
    if queue:
        fe.mask_schedule(None, queue)
    return fe


def _launch(storage, G, frames, queue=0):
    """frames: [(pos1, flow, draws)] as one ragged batch -> (out [F, 32], [mask per frame])"""
    import ssf
    npd, _ = STORAGE[storage]
    dev = torch.device("cuda", 0)
    sizes = [len(f[0]) for f in frames]
    cat = lambda k: np.concatenate([f[k].reshape(-1, 3) for f in frames]).astype(npd)
    if sum(sizes) == 0:
        raise ValueError("an empty batch")
    pts, fl = torch.from_numpy(cat(0)).to(dev), torch.from_numpy(cat(1)).to(dev)
    off, h_off = ssf.frame_offsets(sizes, dev)
    draws = np.stack([np.asarray(f[2], np.float64) for f in frames])
    out, bg = _frontend(G, queue).mask_pose(pts, fl, off, h_off, draws=draws)
    torch.cuda.synchronize()
    out, bg = out.cpu().numpy(), bg.cpu().numpy()
    e = np.cumsum([0] + sizes)
    return out, [bg[e[k]:e[k + 1]] for k in range(len(sizes))]


def _frame(name):
    fx = edge_fixtures()[0][name]
    return fx["pos1"], fx["flow"], fx["draws"]


@functools.lru_cache(maxsize=None)
def _batch(storage, G, queue=0):
    return _launch(storage, G, [_frame(k) for k in NAMES], queue)


@functools.lru_cache(maxsize=None)
def _alone(storage, G, name):
    out, bg = _launch(storage, G, [_frame(name)])
    return out[0], bg[0]


def _check(tag, name, o, bg):
    """every bar of the issue on one frame's record and mask"""
    fx = edge_fixtures()[0][name]
    assert o[_o("STATUS")] == 0, (tag, name, o[_o("STATUS")])
    R, t, q = o[7:16].reshape(3, 3), o[0:3], o[3:7]
    lb = o[_o("LOWER_BOUND")]
    print(f"{tag} {name}: n={len(bg)} km {int(o[_o('KM_ITER')])}/{int(fx['kmeans_n_iter'])} "
          f"em {int(o[_o('EM_ITER')])}/{int(fx['gmm_n_iter'])} lb {lb:.17g} gap "
          f"{abs(lb - float(fx['gmm_lower_bound'])):.3e} mask diff {int((bg != fx['bg_mask']).sum())} "
          f"nbg {int(o[_o('NBG')])}/{int(fx['bg_mask'].sum())} bglabel {int(o[_o('BGLABEL')])}/{int(fx['bg_label'])} "
          f"dR {np.abs(R - fx['R']).max():.3e} dt {np.abs(t - fx['t']).max():.3e}")
    check_fit(fx, o[_o("CENTER0")], o[_o("CENTER1")], o[_o("KM_ITER")], o[_o("EM_ITER")],
              o[_o("CONVERGED")], lb, bg, o[_o("BGLABEL")], o[_o("NBG")], lb_bar=device_lower_bound_bar(fx))
    assert o[_o("NBG")] == bg.sum()
    check_pose(fx, R, t)
    assert np.abs(rot_from_quat(q) - R).max() < 1e-9


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("G", SPLITS, ids=[f"split{G}" for G in SPLITS])
@pytest.mark.parametrize("storage", sorted(STORAGE))
def test_edge_frame_in_batch_vs_sklearn(dev, storage, G, name):
    out, bg = _batch(storage, G)
    k = NAMES.index(name)
    _check(f"{storage} split {G}", name, out[k], bg[k])


@pytest.mark.parametrize("G", SPLITS, ids=[f"split{G}" for G in SPLITS])
@pytest.mark.parametrize("storage", sorted(STORAGE))
def test_edge_frame_alone(dev, storage, G):
    """a fixed split: the frame alone gives the bits it gave in the batch.  The automatic split:
    alone it runs on 32 parts (the resident work-group slots over one frame, capped at the maximum
    split), the path of a default ssf.mask_and_pose call on one small frame, held to the fixture."""
    out, bg = _batch(storage, G)
    bad = []
    for k, name in enumerate(NAMES):
        o1, bg1 = _alone(storage, G, name)
        if G == 0:
            try:
                _check(f"{storage} alone, automatic split", name, o1, bg1)
            except AssertionError as e:
                bad.append((name, str(e).splitlines()[0] if str(e) else "assert"))
        elif not (np.array_equal(o1.view(np.uint64), out[k].view(np.uint64)) and np.array_equal(bg1, bg[k])):
            bad.append(name)
    assert not bad, bad


@pytest.mark.parametrize("storage", sorted(STORAGE))
def test_edge_frames_through_the_frame_queue(dev, storage):
    """3 work-groups taking frame tickets for the 25 frames (split 1): the bits of the plain launch"""
    out, bg = _batch(storage, 1)
    qout, qbg = _batch(storage, 1, 3)
    assert np.array_equal(qout.view(np.uint64), out.view(np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(qbg, bg))


@pytest.mark.parametrize("G", SPLITS, ids=[f"split{G}" for G in SPLITS])
@pytest.mark.parametrize("storage", sorted(STORAGE))
def test_frames_of_one_and_no_point_between_ordinary_frames(dev, storage, G):
    """n = 1 and n = 0 (sklearn: ValueError) report SSF_POSE_GMM_FAILED and nothing else in their
    records; the frames either side keep the results they have without them."""
    from ssf import _abi
    a, b = "size_n129", "tie_b0_s3"
    one = (np.array([[1.0, 2.0, 3.0]], np.float32), np.array([[0.5, 0.0, 0.0]], np.float32), np.array([0.3, 0.6, 0.9]))
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.array([0.3, 0.6, 0.9]))
    out, bg = _launch(storage, G, [_frame(a), one, none, _frame(b)])
    for k in (1, 2):
        assert out[k, _o("STATUS")] == _abi.POSE_GMM_FAILED, (k, out[k, _o("STATUS")])
        assert not np.delete(out[k], _o("STATUS")).any()
    ref, rbg = _launch(storage, G, [_frame(a), _frame(b)])
    for k, r, name in ((0, 0, a), (3, 1, b)):
        _check(f"{storage} split {G} beside n = 1, 0", name, out[k], bg[k])
        if G:                                        # the automatic split depends on the frame count
            assert np.array_equal(out[k].view(np.uint64), ref[r].view(np.uint64)) and np.array_equal(bg[k], rbg[r])


def test_mask_and_pose_surfaces_gmm_failed(dev):
    import ssf
    from ssf import _abi
    fx = edge_fixtures()[0]
    a, b = fx["size_n129"], fx["tie_b0_s3"]
    pts = np.concatenate([a["pos1"], [[1.0, 2.0, 3.0]], b["pos1"]]).astype(np.float32)
    fl = np.concatenate([a["flow"], [[0.5, 0.0, 0.0]], b["flow"]]).astype(np.float32)
    sizes = [len(a["pos1"]), 1, 0, len(b["pos1"])]
    draws = np.stack([a["draws"], [0.3, 0.6, 0.9], [0.3, 0.6, 0.9], b["draws"]])
    r = ssf.mask_and_pose(pts, fl, draws=draws, frame_sizes=sizes, device=dev.index, errors="status")
    assert list(r["info"]["status"]) == [0, _abi.POSE_GMM_FAILED, _abi.POSE_GMM_FAILED, 0]
    bg = r["bg_mask"].cpu().numpy()
    assert np.array_equal(bg[:sizes[0]], a["bg_mask"]) and np.array_equal(bg[sizes[0] + 1:], b["bg_mask"])
    check_pose(a, r["R"][0], r["t"][0])
    check_pose(b, r["R"][3], r["t"][3])
    with pytest.raises(ValueError):
        ssf.mask_and_pose(pts, fl, draws=draws, frame_sizes=sizes, device=dev.index)
    with pytest.raises(ValueError):                  # one frame of one point, the default call
        ssf.mask_and_pose(pts[:1], fl[:1], draws=draws[:1], device=dev.index)

"""k_mask_pose reads its whole-part point streams with the non-temporal policy (global_load ... nt,
DESIGN 6.2.1).  A cache policy changes no value; what a load that bypasses the L1 can newly get
wrong is reading bytes that something else has just written.  So every test here makes the
kernel read freshly overwritten memory and holds the result, bit for bit, to the same launch on
memory nothing has touched:

  reused input buffer    batch A from buffers X, batch B copied over X on the same stream (no
                         synchronisation), launched again: equals B from freshly allocated buffers;
                         one work-group per frame, 2 parts per frame, and the frame queue (2
                         work-groups take the 8 frames back to back)
  reused record buffer   one context, and so one lloyd_rec buffer, runs A then B: B equals B from a
                         new context
  fresh inputs           pos / flow written by BatchScanner.frame right before the mask on the
                         same stream: equals the launch after a device synchronise

each for float32 and float64 storage.  Frames are ssf.synth.scan frames cut to n points:
2, 3 (fewer points than lanes), 767 / 768 / 769 (the 768-thread stride: a clamped last trip, a
thread's lone last EM point), 1537 (2 x 768 + 1, and a part boundary at a multiple of 128 when
split), 4099, and 20011, which is large enough for the Lloyd skip passes and the relabel queue
(KM_ITER > kLloydFullPasses is asserted).  The float32 references are also held to the CPU oracle
with the bars of tests/test_gpu_mask.py (test_full_size_batch_vs_oracle and
test_frame_split_full_size_vs_oracle: status, k-means++ centres, iteration counts, mask agreement
>= 99.9 %, t within 1e-5 m, R within 1e-6; that file holds them as literals inside its tests, so
they are repeated in test_references_vs_oracle).  The n = 2 and n = 3 frames have one and two
background rows: their pose is not unique, and they are held to the rank rule instead.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from helpers import frame

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 767, 768, 769, 1537, 4099, 20011)
# (sequence, frame) of the scan each size is cut from, per batch.  Both batches reach the Lloyd
# skip passes (checked on the CPU with the oracle: KM_ITER 26 at n = 20011 of batch 0; 11 at
# n = 4099 and 5 at n = 20011 of batch 1)
SCANS = {0: [(11, 0), (12, 1), (13, 2), (14, 3), (15, 0), (16, 1), (17, 2), (18, 3)],
         1: [(21, 3), (22, 2), (23, 1), (24, 0), (25, 3), (26, 2), (27, 1), (28, 0)]}
CONFIGS = {"g1": (1, 0), "g2": (2, 0), "queue2": (1, 2)}     # (parts per frame, frame queue)
STORAGE = {"f32": torch.float32, "f64": torch.float64}


def _lloyd_full_passes():
    src = os.path.join(os.path.dirname(__file__), "..", "ssf-slam_amd", "csrc", "mask_common.hpp")
    return int(re.search(r"#define SSF_LLOYD_FULL_PASSES (\d+)", open(src).read()).group(1))


@functools.lru_cache(maxsize=None)
def batch(b):
    """[(pos1 [n, 3], flow [n, 3])] for SIZES and the draws [8, 3] (float32 / float64 numpy)"""
    fr = [frame(s, k)[:2] for s, k in SCANS[b]]
    draws = np.random.default_rng(100 + b).random((len(SIZES), 3))
    return [(p[:n].copy(), f[:n].copy()) for (p, f), n in zip(fr, SIZES)], draws


def _context(cfg):
    import ssf
    G, queue = CONFIGS[cfg]
    fe = ssf.Frontend(64, device=0)
    fe.mask_split(G)
    if queue:
        fe.mask_schedule(None, queue)
    return fe


def _device_batch(b, storage, dev):
    fr, draws = batch(b)
    pts = torch.from_numpy(np.concatenate([f[0] for f in fr])).to(dev).to(STORAGE[storage]).contiguous()
    fl = torch.from_numpy(np.concatenate([f[1] for f in fr])).to(dev).to(STORAGE[storage]).contiguous()
    return pts, fl, draws


def _offsets(dev):
    import ssf
    return ssf.frame_offsets(list(SIZES), dev)


def _bits(out, bg):
    return out.cpu().numpy().view(np.uint64).copy(), bg.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def reference(b, storage, cfg):
    """batch b from freshly allocated buffers on a new context -> (out bits [8, 32] u64, mask)"""
    dev = torch.device("cuda", 0)
    pts, fl, draws = _device_batch(b, storage, dev)
    off, h_off = _offsets(dev)
    torch.cuda.synchronize()
    out, bg = _context(cfg).mask_pose(pts, fl, off, h_off, draws=draws)
    torch.cuda.synchronize()
    return _bits(out, bg)


def _pose_determined(p, f, bg_mask):
    """Kabsch's R is unique when the background's cross-covariance has rank >= 2; at rank 1 or 0
    (second singular value <= 1e-12 of the first, the kernel's own rule) the rotation
    about the line is free and two correct solvers differ"""
    m = bg_mask != 0
    dst = p[m].astype(np.float64)
    src = dst + f[m].astype(np.float64)
    sv = np.linalg.svd((src - src.mean(axis=0)).T @ (dst - dst.mean(axis=0)), compute_uv=False)
    return sv[0] > 0.0 and sv[1] > 1e-12 * sv[0]


def _same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), (what, np.argwhere(got[0] != ref[0])[:8])
    assert np.array_equal(got[1], ref[1]), (what, int((got[1] != ref[1]).sum()))


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("storage", sorted(STORAGE))
def test_reused_input_buffer(dev, storage, cfg):
    fe = _context(cfg)
    off, h_off = _offsets(dev)
    x_pts, x_fl, draws_a = _device_batch(0, storage, dev)
    b_pts, b_fl, draws_b = _device_batch(1, storage, dev)
    torch.cuda.synchronize()
    out_a, bg_a = fe.mask_pose(x_pts, x_fl, off, h_off, draws=draws_a)
    x_pts.copy_(b_pts)                       # device copies on the launches' stream, no synchronise
    x_fl.copy_(b_fl)
    out_b, bg_b = fe.mask_pose(x_pts, x_fl, off, h_off, draws=draws_b)
    torch.cuda.synchronize()
    _same(_bits(out_a, bg_a), reference(0, storage, cfg), "first batch")
    _same(_bits(out_b, bg_b), reference(1, storage, cfg), "second batch from the overwritten buffers")


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("storage", sorted(STORAGE))
def test_reused_record_buffer(dev, storage, cfg):
    fe = _context(cfg)
    fe.reserve(len(SIZES), max(SIZES))       # one record / queue buffer for both launches
    off, h_off = _offsets(dev)
    a_pts, a_fl, draws_a = _device_batch(0, storage, dev)
    b_pts, b_fl, draws_b = _device_batch(1, storage, dev)
    torch.cuda.synchronize()
    fe.mask_pose(a_pts, a_fl, off, h_off, draws=draws_a)
    out_b, bg_b = fe.mask_pose(b_pts, b_fl, off, h_off, draws=draws_b)
    torch.cuda.synchronize()
    _same(_bits(out_b, bg_b), reference(1, storage, cfg), "second batch on the first one's records")


@pytest.mark.parametrize("storage", sorted(STORAGE))
def test_freshly_produced_inputs(dev, storage):
    from ssf import synth
    S, n_az = 3, 313                         # 20032-point frames: the skip passes run
    N = 64 * n_az
    import ssf
    off, h_off = ssf.frame_offsets([N] * S, dev)
    draws = np.random.default_rng(7).random((S, 3))
    sc = synth.BatchScanner([31, 32, 33], 2, n_az=n_az, device=dev)
    pos = torch.zeros((S * N, 3), dtype=torch.float32, device=dev)
    flow = torch.zeros_like(pos)
    fe = _context("g1")
    fe.reserve(S, N)
    torch.cuda.synchronize()
    sc.frame(1, pos, flow)                   # written on the current stream ...
    if storage == "f64":
        p, f = pos.double(), flow.double()   # ... and converted there
    else:
        p, f = pos, flow
    out, bg = fe.mask_pose(p, f, off, h_off, draws=draws)     # ... and read right behind it
    got = (out.clone(), bg.clone())
    torch.cuda.synchronize()
    out2, bg2 = _context("g1").mask_pose(p, f, off, h_off, draws=draws)
    torch.cuda.synchronize()
    assert np.all(out2.cpu().numpy()[:, 16] == 0)
    assert out2.cpu().numpy()[:, 19].max() > _lloyd_full_passes()
    _same(_bits(*got), _bits(out2, bg2), "launch right behind the producer")


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("b", [0, 1])
def test_references_vs_oracle(oracle, dev, b, cfg):
    """the bars of tests/test_gpu_mask.py against the CPU oracle, on the float32 references"""
    out, bg = reference(b, "f32", cfg)
    out = out.view(np.float64)
    fr, draws = batch(b)
    e = np.cumsum((0,) + SIZES)
    km = []
    for k, (p, f) in enumerate(fr):
        ref = oracle.mask_and_pose(p, f, draws[k])
        o = out[k]
        print(f"batch {b} {cfg} n={SIZES[k]}: status {o[16]}/{ref['rc']} km {int(o[19])}/{ref['info']['kmeans_iter']} "
              f"em {int(o[20])}/{ref['info']['em_iter']} mask agree {(bg[e[k]:e[k + 1]] == ref['bg_mask']).mean():.6f} "
              f"dt {np.abs(o[0:3] - ref['t']).max():.3e} dR {np.abs(o[7:16].reshape(3, 3) - ref['R']).max():.3e}")
        assert o[16] == ref["rc"] == 0
        assert int(o[22]) == int(ref["info"]["center0"]) and int(o[23]) == int(ref["info"]["center1"])
        assert int(o[19]) == int(ref["info"]["kmeans_iter"]) and int(o[20]) == int(ref["info"]["em_iter"])
        assert (bg[e[k]:e[k + 1]] == ref["bg_mask"]).mean() >= 0.999
        R, t = o[7:16].reshape(3, 3), o[0:3]
        if _pose_determined(p, f, ref["bg_mask"]):
            assert np.abs(t - ref["t"]).max() < 1e-5
            assert np.abs(R - ref["R"]).max() < 1e-6
        else:
            # one or two background rows (n = 2, 3): the rotation about their line is free, two
            # correct solvers differ (DESIGN 6.2, rank rules).  Held instead to what every
            # solution shares: a proper rotation that carries the source centroid onto the
            # target centroid; the pose bits of these frames are held by the bitwise tests.
            m = ref["bg_mask"] != 0
            md = p[m].astype(np.float64).mean(axis=0)
            ms = (p[m].astype(np.float64) + f[m].astype(np.float64)).mean(axis=0)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0
            assert np.abs(R @ ms + t - md).max() < 1e-5
        km.append(int(o[19]))
    assert max(km) > _lloyd_full_passes(), km    # a skip pass (records, relabel queue) really ran

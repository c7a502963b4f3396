"""The device feature stage (ring binning, curvature, planar selection: feat_*.hip) against the
numpy yardstick of src/frameFeature.cpp:45-123 (tests/feature_reference.py) -- not against the
CPU oracle -- on the cases of tests/feature_cases.py: rows of every length around the stencil's
10/11-point edge, the span and a candidate word; curvature exactly at planeMin and one float to
either side; rows where two thirds of the points are candidates; infinite and NaN curvature; for
both profiles, in every input order launch_extract_planes routes differently.

One ragged launch per layout and profile holds every case as a frame (and an empty frame); the
debug instantiations give row offsets, the ring-ordered cloud and every curvature value, a second
launch without them runs the product instantiations.  Bar: bit equality (curvature: uint32
where the yardstick is not NaN, NaN where it is; the GPU's NaN bit pattern is its own).
"""
import functools

import numpy as np
import pytest
import torch

import feature_cases as fc
import feature_reference as ref
from test_feature_host import bits_equal, curvature_equal, seen_cloud

pytestmark = pytest.mark.gpu
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _frames(n_rows, layout):
    """[(name, pts [n, stride], keep or None, yardstick result)] -- computed once, never changed"""
    out = []
    for cs in fc.cases(n_rows):
        pts, keep = fc.layout(cs, layout)
        out.append((cs.name, pts, keep, ref.extract_planes(seen_cloud(pts, keep), n_rows)))
    stride = out[0][1].shape[1]
    empty = np.zeros((0, stride), F32)
    out.insert(2, ("empty", empty, None if out[0][2] is None else np.zeros(0, np.uint8),
                   ref.extract_planes(empty[:, :3], n_rows)))
    return out


def _launch(fe, frames, dev, debug):
    import ssf
    pts = np.concatenate([f[1] for f in frames])
    t = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    off, h_off = ssf.frame_offsets([len(f[1]) for f in frames], dev)
    kw = {}
    if frames[0][2] is not None:
        kw["keep"] = torch.from_numpy(np.concatenate([f[2] for f in frames])).to(dev)
    if pts.shape[1] != 3:
        kw["point_stride"] = pts.shape[1]
    out = fe.extract_planes_batch(t, off, h_off, debug=debug, **kw)
    torch.cuda.synchronize()
    return out, h_off


def _check(fe, frames, dev, n_rows):
    (pb, ring, roff, curv), h_off = _launch(fe, frames, dev, True)
    count = pb.count.cpu().numpy()
    ring, roff, curv = ring.cpu().numpy(), roff.cpu().numpy(), curv.cpu().numpy()
    for f, (name, _, _, y) in enumerate(frames):
        o, kept = int(h_off[f]), int(y["off"][-1])
        assert np.array_equal(roff[f].astype(np.int64), y["off"]), (name, "row offsets")
        assert bits_equal(ring[o:o + kept], y["rx"]), (name, "ring-ordered cloud")
        assert curvature_equal(curv[o:o + kept], y["cv"]), (name, "curvature")
        assert int(count[f]) == len(y["planes"]), (name, "count", int(count[f]), len(y["planes"]))
        assert bits_equal(pb.frame(f).cpu().numpy(), y["planes"]), (name, "plane list")
    pb, h_off = _launch(fe, frames, dev, False)                 # the product instantiations
    count = pb.count.cpu().numpy()
    for f, (name, _, _, y) in enumerate(frames):
        assert int(count[f]) == len(y["planes"]), (name, "count, product path")
        assert bits_equal(pb.frame(f).cpu().numpy(), y["planes"]), (name, "plane list, product path")


@pytest.mark.parametrize("layout", fc.LAYOUTS)
@pytest.mark.parametrize("n_rows", [16, 64])
def test_feature_stage_equals_yardstick(dev, n_rows, layout):
    import ssf
    fe = ssf.Frontend(n_rows, device=dev.index or 0)
    _check(fe, _frames(n_rows, layout), dev, n_rows)


@pytest.mark.parametrize("n_rows", [16, 64])
def test_feature_stage_double_ring_chain(dev, n_rows):
    """every finite point is clear of the bin edges and the others have an exact angle, so the
    all-double evaluation of frameFeature.cpp:57 bins them as the float one does (the run above)"""
    import ssf
    fe = ssf.Frontend(n_rows, device=dev.index or 0, ring_chain="double")
    _check(fe, _frames(n_rows, "interleaved"), dev, n_rows)


@pytest.mark.parametrize("n_rows", [16, 64])
def test_binned_stage_equals_yardstick(dev, n_rows):
    """One frame padded with NaN points past 262144 points: the launch takes the binned stage
    (k_bin_count / k_bin_scan / k_bin_curv / k_select) for every frame of the batch, the short
    ones included.  The padded frame's real points lie in eight runs 37k inputs apart."""
    import ssf
    frames = list(_frames(n_rows, "rowmajor"))
    dense = next(c for c in fc.cases(n_rows) if c.name == "dense")
    big = fc.binned(dense)
    assert len(big) > fc.BINNED_POINTS
    frames.insert(1, ("dense, padded", big, None, ref.extract_planes(big, n_rows)))
    fe = ssf.Frontend(n_rows, device=dev.index or 0)
    _check(fe, frames, dev, n_rows)

"""EM pair loop of k_mask_pose: full pairs, a lone first point, a lone last point and threads with
no point at all, against the CPU oracle.

The EM pass hands every thread the points (i, i + T), (i + 2T, i + 3T), ... of its part (T = 768
threads) as pairs and a thread's last point alone when its partner does not exist.  The sizes
below put the part's end on each side of T, 2T and 4T: below T some threads have no point and
every other thread a lone one; at T + 1 one thread has a full pair; at 2T - 1 one thread a lone
point beside full pairs; above 2T the lone point follows a full pair.  A split of 2 halves each
frame into parts of odd and even length (383 / 384 ... 1536 / 1537) that sum across work-groups.

Frames: 16 rows x 500 azimuth steps of the synthetic scene, thinned evenly to n points (the
first n points of a scan are one sector of the scene and converge degenerately).  Bars as in
test_gpu_mask.py: status 0, k-means++ indices and KMeans / EM iteration counts equal, background
agreement >= 0.999, t within 1e-5, R within 1e-6.

Seed policy: the oracle's EM count can differ from the device's only where |lb - prev| at an
iteration lies within rounding (1e-9) of the 1e-3 threshold.  On these seven frames the oracle's
closest approach to the threshold over all iterations is 4.0e-5 (n = 1535; 3.0e-4 or more on the
others), so none is knife-edge and none was swapped.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import frame

pytestmark = pytest.mark.gpu

SIZES = [767, 768, 769, 1535, 1536, 1537, 3073]
DRAWS = np.random.default_rng(11).random((len(SIZES), 3))


@functools.lru_cache(maxsize=None)
def _cut(j):
    """frame (sequence j + 1, scan j) thinned evenly to SIZES[j] points"""
    p, f, _ = frame(j + 1, j, n_rows=16, n_az=500)
    idx = (np.arange(SIZES[j]) * p.shape[0]) // SIZES[j]
    return np.ascontiguousarray(p[idx]), np.ascontiguousarray(f[idx])


@functools.lru_cache(maxsize=None)
def _reference(j):
    from oracle import oracle as O
    p, f = _cut(j)
    return O.mask_and_pose(p, f, DRAWS[j])


@functools.lru_cache(maxsize=None)
def _device(G):
    """all seven cuts in one launch with the split fixed at G parts per frame"""
    import ssf
    dev = torch.device("cuda", 0)
    cuts = [_cut(j) for j in range(len(SIZES))]
    pts = torch.from_numpy(np.concatenate([c[0] for c in cuts]).astype(np.float32)).to(dev)
    fl = torch.from_numpy(np.concatenate([c[1] for c in cuts]).astype(np.float32)).to(dev)
    off, h_off = ssf.frame_offsets(list(SIZES), dev)
    fe = ssf.Frontend(64, device=0)
    fe.mask_split(G)
    out, bg = fe.mask_pose(pts, fl, off, h_off, draws=DRAWS)
    torch.cuda.synchronize()
    return out.cpu().numpy(), bg.cpu().numpy(), [int(v) for v in h_off]


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("j", range(len(SIZES)), ids=[f"n{n}" for n in SIZES])
def test_em_pair_and_tail_shapes_vs_oracle(oracle, dev, j, G):
    ref = _reference(j)
    out, bg, h_off = _device(G)
    o = out[j]
    print(f"n={SIZES[j]} G={G}: km {int(o[19])}/{ref['info']['kmeans_iter']:.0f} em {int(o[20])}/"
          f"{ref['info']['em_iter']:.0f} lb {o[24]:.17g}/{ref['info']['lower_bound']:.17g} "
          f"dt {np.abs(o[0:3] - ref['t']).max():.3e} dR {np.abs(o[7:16].reshape(3, 3) - ref['R']).max():.3e}")
    assert o[16] == ref["rc"] == 0
    assert int(o[22]) == int(ref["info"]["center0"]) and int(o[23]) == int(ref["info"]["center1"])
    assert int(o[19]) == int(ref["info"]["kmeans_iter"]) and int(o[20]) == int(ref["info"]["em_iter"])
    a, b = h_off[j], h_off[j + 1]
    assert b - a == SIZES[j]
    agree = (bg[a:b] == ref["bg_mask"]).mean()
    assert agree >= 0.999, agree
    assert np.abs(o[0:3] - ref["t"]).max() < 1e-5
    assert np.abs(o[7:16].reshape(3, 3) - ref["R"]).max() < 1e-6

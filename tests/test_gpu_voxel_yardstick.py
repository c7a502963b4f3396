"""The device voxel grid (loop.hip: k_vg_bounds, k_vg_keys, the radix sort, k_vg_heads,
k_vg_reduce) against the numpy yardstick of PCL 1.10's VoxelGrid (tests/feature_reference.py) --
not against the CPU oracle -- on the clouds of tests/feature_cases.py: a lattice on voxel
boundaries on both sides of zero, one point, 700 points in one voxel (a run across three
256-thread blocks), duplicates, an empty cloud, neighbouring clouds that end and start in the
same voxel index, in batches of 1, 2, 3, 4, 5, 8 and 9 clouds (the sort's end_bit grows with the
cloud count: 32, 33, 34, 34, 35, 35, 36), at leaf 0.1 and 0.4.  Bar: bit equality and equal
counts.
"""
import numpy as np
import pytest
import torch

import feature_cases as fc
import feature_reference as ref
from test_feature_host import bits_equal

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.mark.parametrize("leaf", fc.VOXEL_LEAVES)
@pytest.mark.parametrize("n_clouds", fc.VOXEL_BATCH_SIZES)
def test_voxel_grid_equals_yardstick(dev, n_clouds, leaf):
    import ssf
    from ssf import loop
    names = fc.VOXEL_BATCHES[n_clouds]
    clouds = [fc.voxel_clouds()[n] for n in names]
    fe = ssf.Frontend(64, device=dev.index or 0)
    x = torch.from_numpy(np.concatenate(clouds)).to(dev)
    off, h_off = ssf.frame_offsets([len(c) for c in clouds], dev)
    out, cnt = loop.voxel_grid(fe, x, off, h_off, leaf)
    torch.cuda.synchronize()
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    for c, (name, cl) in enumerate(zip(names, clouds)):
        want = ref.voxel_grid(cl, leaf)
        assert int(cnt[c]) == len(want), (name, c, int(cnt[c]), len(want))
        o = int(h_off[c])
        assert bits_equal(out[o:o + len(want)], want), (name, c)


@pytest.mark.parametrize("leaf", fc.VOXEL_LEAVES)
def test_voxel_grid_passthrough_equals_yardstick(dev, leaf):
    """PCL's overflow guard: the cloud comes back unchanged, in input order"""
    import ssf
    from ssf import loop
    assert ref.voxel_passthrough(fc.PASSTHROUGH, leaf)
    fe = ssf.Frontend(64, device=dev.index or 0)
    got = loop.voxel_grid_one(fe, torch.from_numpy(fc.PASSTHROUGH).to(dev), leaf).cpu().numpy()
    assert bits_equal(got, ref.voxel_grid(fc.PASSTHROUGH, leaf)) and bits_equal(got, fc.PASSTHROUGH)

"""Golden vectors for the two layer types of the TFlow encoder / decoder, produced by the
REFERENCE's own module code: PointNetSetAbstraction (utils/utils.py:185-248) and
PointNetSetUpConv (utils/utils.py:250-315).

Run in the build container only (it reads /root/reference, absent on the GPU box); the .npz it
writes is committed and is what tests/test_sa_host.py and tests/test_gpu_sa.py read.

What is imported / called:
  * /root/reference/scripts/ActiveSceneFlow/utils/utils.py through import_reference() of
    make_golden_pn2.py (`lib` / `lib.pointnet2_utils` replaced by empty stubs).  The stub's
    furthest_point_sample, gather_operation, knn and grouping_operation are then set to the
    reference's own torch forms: farthest_point_sample (:68-89), index_points (:48-65) and
    knn_point (:92-108).
  * farthest_point_sample draws its first centroid with torch.randint; the un-vendored
    extension starts at index 0, and so does ssf_pn2_furthest_point_sample by default.  The draw
    is therefore replaced by zeros for the duration of that call (nothing else is patched).
  * Indices (FPS, k-NN) are always computed on the float32 coordinates, also in the `.double()`
    run: the float64 outputs are the same arithmetic on the same neighbours, not another
    neighbourhood.

Both modules are in .eval() with seeded weights and seeded, non-trivial running statistics.
Inputs: two seeded synthetic 64-beam scans (ssf.synth), subsampled to 512 points.
"""
from __future__ import annotations

import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_pn2 import import_reference  # noqa: E402

SA_ARGS = dict(npoint=37, radius=0.5, nsample=16, in_channel=6, mlp=[16, 24, 40])
SU_ARGS = dict(nsample=5, radius=2.4, f1_channel=7, f2_channel=40, mlp=[24, 20], mlp2=[12])


def install_pointutils(U, torch):
    pu = U.pointutils

    def fps(xyz_t, npoint):
        zeros = lambda lo, hi, size, dtype=torch.long: torch.zeros(size, dtype=dtype)  # noqa: E731
        with mock.patch.object(torch, "randint", zeros):
            return U.farthest_point_sample(xyz_t.float(), npoint)

    def gather(features, idx):                       # [B, C, N] x [B, S] -> [B, C, S]
        return U.index_points(features.permute(0, 2, 1), idx.long()).permute(0, 2, 1).contiguous()

    def group(features, idx):                        # [B, C, N] x [B, S, K] -> [B, C, S, K]
        return U.index_points(features.permute(0, 2, 1), idx.long()).permute(0, 3, 1, 2).contiguous()

    def knn(k, query, ref):                          # pointutils.knn(k, query, ref) -> (dist, idx)
        return U.knn_point(k, ref.float(), query.float())

    pu.furthest_point_sample, pu.gather_operation, pu.grouping_operation, pu.knn = fps, gather, group, knn
    return pu


def seed_module(mod, torch, gen):
    """Seeded weights and non-trivial BatchNorm statistics."""
    for m in mod.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv1d)):
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) / np.sqrt(m.in_channels))
        elif isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
            c = m.num_features
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(c, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(c, generator=gen) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(c, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(c, generator=gen) * 0.2)


def main():
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "ssf-slam_amd"))
    from ssf import synth

    U = import_reference()
    pu = install_pointutils(U, torch)
    rng = np.random.default_rng(20240611)
    gen = torch.Generator().manual_seed(20240611)
    B, N = 2, 512
    clouds = []
    for b in range(B):
        p = synth.scan(11, b, n_az=300)["pos1"].numpy().astype(np.float32)
        clouds.append(p[np.sort(rng.choice(p.shape[0], N, replace=False))])
    xyz = torch.from_numpy(np.stack(clouds)).permute(0, 2, 1).contiguous()          # [B, 3, N]
    points = torch.from_numpy(rng.standard_normal((B, SA_ARGS["in_channel"], N)).astype(np.float32))
    feat1 = torch.from_numpy(rng.standard_normal((B, SU_ARGS["f1_channel"], N)).astype(np.float32))

    sa = U.PointNetSetAbstraction(group_all=False, **SA_ARGS).eval()
    su = U.PointNetSetUpConv(**SU_ARGS).eval()
    seed_module(sa, torch, gen)
    seed_module(su, torch, gen)
    sa_state = {k: v.numpy().copy() for k, v in sa.state_dict().items()}
    su_state = {k: v.numpy().copy() for k, v in su.state_dict().items()}

    with torch.no_grad():
        new_xyz, new_points, fps_idx = sa(xyz, points)
        # the decoder direction: from the 37 centroids (pos2, feature2) back to the 512 points
        up = su(xyz, new_xyz, feat1, new_points)
        _, sa_knn = pu.knn(SA_ARGS["nsample"], new_xyz.permute(0, 2, 1).contiguous(), xyz.permute(0, 2, 1).contiguous())
        _, su_knn = pu.knn(SU_ARGS["nsample"], xyz.permute(0, 2, 1).contiguous(), new_xyz.permute(0, 2, 1).contiguous())
        sa64, su64 = sa.double(), su.double()
        new_xyz64, new_points64, fps64 = sa64(xyz.double(), points.double(), fps_idx)
        # same float32 inputs as the float32 run, feature2 included
        up64 = su64(xyz.double(), new_xyz.double(), feat1.double(), new_points.double())
    assert torch.equal(fps64, fps_idx) and torch.equal(new_xyz64.float(), new_xyz)

    out = os.path.join(HERE, "sa_ref.npz")
    arrays = dict(
        xyz=xyz.numpy(), points=points.numpy(), feat1=feat1.numpy(),
        fps_idx=fps_idx.numpy().astype(np.int32), sa_knn_idx=sa_knn.numpy().astype(np.int32),
        su_knn_idx=su_knn.numpy().astype(np.int32),
        sa_new_xyz=new_xyz.numpy(), sa_out=new_points.numpy(), sa_out_f64=new_points64.numpy(),
        su_out=up.numpy(), su_out_f64=up64.numpy())
    arrays.update({"sa_state/" + k: v for k, v in sa_state.items()})
    arrays.update({"su_state/" + k: v for k, v in su_state.items()})
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

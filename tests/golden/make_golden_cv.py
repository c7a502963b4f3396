"""Golden vectors for the TFlow cost volume, warping and the whole network, produced by the
REFERENCE's own module code: PointConvTransFlowV2 (utils/soflow.py:281-525), PointWarping
(:1222-1257) and TFlow (TFlowV3_Occlussion_addSeg.py:65-199).

Run in the build container only (it reads /root/reference, absent on the GPU box); the two .npz it
writes (cv_ref.npz, tflow_ref.npz) are committed and are what tests/test_cv_host.py and
tests/test_gpu_cv.py read.

What is imported / called:
  * the reference's `utils` package and TFlowV3_Occlussion_addSeg.py, with these stubs:
    `lib.pointnet2_utils` (install_pointutils of make_golden_sa.py: the reference's own torch
    forms of furthest_point_sample, gather_operation, grouping_operation and knn; three_nn =
    knn(3, ...) is added here), `utils.datasets` / `utils.datasets.carla`
    (add_Seg_after_FLow = False, its value at carla.py:9) and `torch_scatter` (absent here:
    scatter_softmax and scatter_sum written with scatter_reduce_ / scatter_add_, the package's own
    algorithm: subtract the segment maximum, exp, divide by the segment sum).
  * Weights come from cv_reference.seed_state(keys and shapes, seed); the tests rebuild them.
  * Indices (FPS, k-NN) are always those of the float32 run: the float64 run replays them, so its
    outputs are the same arithmetic on the same neighbours.  During the float64 run
    Tensor.float() is the identity, because UpsampleFlow.forward casts the sparse flow with it
    (:1470) and would round the float64 run to float32 there.

The generator asserts, and moves on to the next seed when an assertion fails:
  * max(knn_idxw) + 1 == N2 in cases A and B (scatter_sum gets no dim_size, so the reference's
    cost_bwd is max(knn_idxw) + 1 long and its own gather by knn_idx would be out of range);
  * for every k-NN call of cases A and B and every k-NN call of the TFlow run before flow2_r, the
    repository's direct-difference k-NN (the CPU oracle's pn2_knn, which the device kernel matches
    bit for bit) returns the same neighbour SETS as the reference's knn_point (order within a set
    cannot matter: every consumer is a sum, a max or a softmax over the set);
  * every e_ref = max|f32 - f64| is positive.
"""
from __future__ import annotations

import os
import sys
import types
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_ASF = "/root/reference/scripts/ActiveSceneFlow"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "ssf-slam_amd"))
sys.path.insert(0, REPO)
from make_golden_sa import install_pointutils  # noqa: E402
import cv_reference as R  # noqa: E402

CASES = {
    "A": dict(nsample=8, in_channel=12, sf_channel=10, mlp=[16, 16], flow_mlp=[16, 16], use_flow=True),
    "B": dict(nsample=5, in_channel=12, sf_channel=0, mlp=[16, 16], flow_mlp=[16, 16], use_flow=False),
}
B, N1, N2, CROP = 2, 128, 160, 9.0
TFLOW_N = 2048


def import_reference(torch):
    """-> (utils.utils, utils.soflow, TFlowV3_Occlussion_addSeg) under the stubs"""
    lib = types.ModuleType("lib")
    lib.pointnet2_utils = types.ModuleType("lib.pointnet2_utils")
    sys.modules.setdefault("lib", lib)
    sys.modules.setdefault("lib.pointnet2_utils", lib.pointnet2_utils)

    def scatter_softmax(src, index, dim=1):                 # src [B, M, C], index [B, M]
        assert dim == 1
        ix = index.unsqueeze(-1).expand_as(src)
        size = int(index.max()) + 1
        mx = src.new_full((src.shape[0], size, src.shape[2]), float("-inf"))
        mx.scatter_reduce_(1, ix, src, "amax", include_self=True)
        e = (src - mx.gather(1, ix)).exp()
        su = src.new_zeros(mx.shape).scatter_add_(1, ix, e)
        return e / su.gather(1, ix)

    def scatter_sum(src, index, dim=1):
        assert dim == 1
        ix = index.unsqueeze(-1).expand_as(src)
        return src.new_zeros((src.shape[0], int(index.max()) + 1, src.shape[2])).scatter_add_(1, ix, src)

    ts = types.ModuleType("torch_scatter")
    ts.scatter_softmax, ts.scatter_sum = scatter_softmax, scatter_sum
    sys.modules["torch_scatter"] = ts
    ds = types.ModuleType("utils.datasets")
    carla = types.ModuleType("utils.datasets.carla")
    carla.add_Seg_after_FLow = False
    ds.carla = carla
    sys.modules["utils.datasets"] = ds
    sys.modules["utils.datasets.carla"] = carla
    sys.path.insert(0, REF_ASF)
    import utils.utils as U
    import utils.soflow as S
    import TFlowV3_Occlussion_addSeg as T
    return U, S, T


class Tape:
    """records the index-producing calls of a float32 run and replays them in the float64 run"""

    def __init__(self, fn, keep_inputs):
        self.fn, self.keep_inputs, self.calls, self.queue = fn, keep_inputs, [], None

    def __call__(self, *args):
        if self.queue is not None:
            return self.queue.pop(0)
        out = self.fn(*args)
        self.calls.append((tuple(a.detach().float().numpy().copy() if hasattr(a, "detach") else a
                                 for a in args) if self.keep_inputs else None, out))
        return out

    def replay(self):
        self.queue = [out for _, out in self.calls]


def taped(pu):
    pu.knn = Tape(pu.knn, True)
    pu.three_nn = lambda unknown, known: pu.knn(3, unknown, known)
    pu.furthest_point_sample = Tape(pu.furthest_point_sample, False)
    return pu


def same_sets(O, calls):
    """the repository's k-NN against the reference's knn_point, as neighbour sets"""
    for (k, query, ref), (_, idx) in calls:
        ours = O.pn2_knn(int(k), query, ref)[1]
        if not np.array_equal(np.sort(ours, -1), np.sort(idx.numpy().astype(np.int32), -1)):
            return False
    return True


def load_seeded(mod, torch, seed):
    shapes = [(k, tuple(v.shape)) for k, v in mod.state_dict().items()]
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in R.seed_state(shapes, seed).items()}, strict=True)
    return shapes


def run_both(torch, pu, f32_run, f64_run):
    """f32_run() with recording tapes, then f64_run() replaying them with Tensor.float() = identity"""
    pu.knn.calls, pu.furthest_point_sample.calls = [], []
    pu.knn.queue = pu.furthest_point_sample.queue = None
    with torch.no_grad():
        o32 = f32_run()
        pu.knn.replay()
        pu.furthest_point_sample.replay()
        with mock.patch.object(torch.Tensor, "float", lambda self: self):
            o64 = f64_run()
    assert not pu.knn.queue and not pu.furthest_point_sample.queue
    pu.knn.queue = pu.furthest_point_sample.queue = None
    return o32, o64


def clouds(synth, rng, seed, frames, n):
    out = []
    for f in frames:
        p = synth.scan(seed, f, n_az=300)["pos1"].numpy().astype(np.float32)
        p = p[np.abs(p).max(axis=1) < CROP]
        out.append(p[np.sort(rng.choice(p.shape[0], n, replace=False))])
    return np.stack(out)


def positive(pairs):
    return all(np.abs(a.numpy().astype(np.float64) - b.numpy()).max() > 0 for a, b in pairs)


def make_case(torch, S, pu, O, synth, name, cfg, seed):
    rng = np.random.default_rng(seed)
    t = torch.from_numpy
    xyz1 = t(clouds(synth, rng, 11, (0, 2), N1)).permute(0, 2, 1).contiguous()       # [B, 3, N1]
    xyz2 = t(clouds(synth, rng, 11, (1, 3), N2)).permute(0, 2, 1).contiguous()       # [B, 3, N2]
    c = cfg["in_channel"]
    points1 = t(rng.standard_normal((B, c, N1)).astype(np.float32))
    points2 = t(rng.standard_normal((B, c, N2)).astype(np.float32))
    flow = t((rng.standard_normal((B, 3, N1)) * 0.3).astype(np.float32))
    sf_feat = t(rng.standard_normal((B, cfg["sf_channel"], N1)).astype(np.float32)) if cfg["sf_channel"] else None
    mod = S.PointConvTransFlowV2(**cfg).eval()
    shapes = load_seeded(mod, torch, seed)
    warp = S.PointWarping()
    wn = 5 if name == "A" else None                       # knn(5) and the three_nn path
    with_sf = cfg["use_flow"]

    def run(dt):
        def go():
            m = mod.to(dt)
            c = lambda a: None if a is None else a.to(dt)  # noqa: E731
            w = warp(c(xyz1), c(xyz2), c(flow), wn)
            if with_sf:
                outs = m(c(xyz1), c(xyz2), w, c(points1), c(points2), c(flow), c(sf_feat))
            else:
                outs = m(c(xyz1), c(xyz2), None, c(points1), c(points2))
            return (w,) + tuple(outs)
        return go

    o32, o64 = run_both(torch, pu, run(torch.float32), run(torch.float64))
    calls = pu.knn.calls
    assert len(calls) == 3                                # warping, knn_idx, knn_idxw
    warp_idx, knn_idx, knn_idxw = (c[1][1].numpy().astype(np.int32) for c in calls)
    if int(knn_idxw.max()) + 1 != N2 or not same_sets(O, calls) or not positive(zip(o32, o64)):
        return None
    arrays = dict(seed=np.int64(seed), keys=np.array([k for k, _ in shapes]),
                  shapes=np.array([",".join(map(str, s)) for _, s in shapes]),
                  xyz1=xyz1.numpy(), xyz2=xyz2.numpy(), points1=points1.numpy(), points2=points2.numpy(),
                  flow=flow.numpy(), warp_idx=warp_idx, knn_idx=knn_idx, knn_idxw=knn_idxw)
    if sf_feat is not None:
        arrays["sf_feat"] = sf_feat.numpy()
    for n, a, b in zip(("pc2_warp", "cost_fwd", "cost_bwd", "cost", "flow_out"), o32, o64):
        arrays[n], arrays[n + "_f64"] = a.numpy(), b.numpy()
    return {f"{name}/{k}": v for k, v in arrays.items()}


def make_tflow(torch, T, pu, O, synth, seed):
    rng = np.random.default_rng(seed)
    t = torch.from_numpy
    pc1 = t(clouds(synth, rng, 13, (0,), TFLOW_N)).permute(0, 2, 1).contiguous()
    pc2 = t(clouds(synth, rng, 13, (1,), TFLOW_N)).permute(0, 2, 1).contiguous()
    net = T.TFlow().eval()
    shapes = load_seeded(net, torch, seed)
    mark = []
    hook = net.flow2_r.register_forward_pre_hook(lambda m, a: mark.append(len(pu.knn.calls)) if pu.knn.queue is None else None)
    try:
        (f32, fps32), (f64, fps64) = run_both(torch, pu, lambda: net.float()(pc1, pc2),
                                              lambda: net.double()(pc1.double(), pc2.double()))
    except (IndexError, RuntimeError) as e:               # the reference's own gather out of range
        print("  tflow seed", seed, "failed in the reference:", type(e).__name__, str(e)[:80])
        return None
    finally:
        hook.remove()
    if not same_sets(O, pu.knn.calls[:mark[0]]) or not positive(zip(f32, f64)):
        return None
    arrays = dict(seed=np.int64(seed), keys=np.array([k for k, _ in shapes]),
                  shapes=np.array([",".join(map(str, s)) for _, s in shapes]), pc1=pc1.numpy(), pc2=pc2.numpy(),
                  knn_calls_before_flow2_r=np.int64(mark[0]), knn_calls=np.int64(len(pu.knn.calls)))
    for i, f in enumerate(fps32):
        arrays[f"fps_inds{i}"] = f.numpy().astype(np.int32)
    for i, (a, b) in enumerate(zip(f32, f64)):
        arrays[f"flow{i}"], arrays[f"flow{i}_f64"] = a.numpy(), b.numpy()
    return arrays


def first_seed(make, start):
    for seed in range(start, start + 50):
        arrays = make(seed)
        if arrays is not None:
            return arrays
        print("  seed", seed, "rejected")
    raise SystemExit("no seed passed the generator's assertions")


def main():
    import torch
    from ssf import synth
    from oracle import oracle as O

    U, S, T = import_reference(torch)
    pu = taped(install_pointutils(U, torch))
    cv = {}
    for name, cfg in CASES.items():
        cv.update(first_seed(lambda seed: make_case(torch, S, pu, O, synth, name, cfg, seed), 20241001))
        print("case", name, "seed", int(cv[f"{name}/seed"]))
    out = os.path.join(HERE, "cv_ref.npz")
    np.savez_compressed(out, **cv)
    print("wrote", out, os.path.getsize(out), "bytes")
    tf = first_seed(lambda seed: make_tflow(torch, T, pu, O, synth, seed), 20241101)
    out = os.path.join(HERE, "tflow_ref.npz")
    np.savez_compressed(out, **tf)
    print("wrote", out, os.path.getsize(out), "bytes; seed", int(tf["seed"]),
          "k-NN calls", int(tf["knn_calls"]), "before flow2_r", int(tf["knn_calls_before_flow2_r"]))


if __name__ == "__main__":
    main()

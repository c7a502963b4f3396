#!/usr/bin/env python3
"""Time ssf.tflow.CostVolume (three HIP kernels, csrc/cost_volume.hip) against the same
arithmetic as device torch ops -- the op sequence of PointConvTransFlowV2.forward
(utils/soflow.py:354-525) with this project's knn / grouping_operation, conv2d per layer,
matmul / softmax for the attention and scatter_reduce_ / scatter_add_ for torch_scatter -- on the
four RefineFlowRegressor levels of TFlow (TFlowV3_Occlussion_addSeg.py:81-95) at B = 2 and
N = 8192 input points, and one whole TFlow forward at that size.

The parent has no cost volume, so the unfused device composition is the yardstick; nothing is
asserted.  Inputs: uniform random clouds (cloud 2 = cloud 1 moved by a small random flow, then
shuffled), seeded weights.  HIP events around each call on the current stream, one synchronise
per sample; the two variants alternate in one process; warm-up first, median of --runs samples
(>= 20).  Writes profiles/cv_bench.json."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ssf-slam_amd"))

B = 2
LEVELS = [dict(name="flow3_r", N=256, nsample=16, in_channel=256, sf_channel=0, mlp=[256, 256], flow_mlp=[128, 128], use_flow=False),
          dict(name="flow2_r", N=512, nsample=16, in_channel=192, sf_channel=128, mlp=[128, 128], flow_mlp=[128, 128], use_flow=True),
          dict(name="flow1_r", N=2048, nsample=16, in_channel=96, sf_channel=128, mlp=[64, 64], flow_mlp=[64, 64], use_flow=True),
          dict(name="flow0_r", N=8192, nsample=16, in_channel=96, sf_channel=64, mlp=[64, 64], flow_mlp=[64, 64], use_flow=True)]


def unfused(torch, P, cv, xyz1, xyz2, xyz2w, points1, points2, sf, sf_feat):
    """PointConvTransFlowV2.forward as device torch ops on [B, C, N1, K] tensors"""
    Fn = torch.nn.functional
    lrelu = lambda t: Fn.leaky_relu(t, 0.1)  # noqa: E731
    Bn, _, N1 = xyz1.shape
    K = cv.nsample
    knn_idx, knn_idxw = cv.indices(xyz1, xyz2, xyz2w, sf)
    p1 = points1[:, :, :, None].expand(-1, -1, -1, K)

    def branch(idx, convs):
        direction = P.grouping_operation(xyz2, idx) - xyz1[:, :, :, None]
        x = torch.cat([p1, P.grouping_operation(points2, idx)], dim=1)
        for conv in convs:
            x = lrelu(conv(x))
        return x, direction

    q, direction = branch(knn_idx, cv.mlp_convs)
    kw, directionw = branch(knn_idxw, cv.mlp_convs2)
    a = torch.matmul(q.permute(0, 2, 3, 1), kw.permute(0, 2, 1, 3))               # [B, N1, K, K]
    w = torch.softmax(a, -2) * torch.softmax(a, -1)
    extra = [] if sf_feat is None else [sf_feat[:, :, :, None].expand(-1, -1, -1, K)]
    cq, ckw = torch.cat([q] + extra + [direction], dim=1), torch.cat([kw] + extra + [directionw], dim=1)
    for conv in cv.mlp_convs3:
        cq, ckw = lrelu(conv(cq)), lrelu(conv(ckw))
    qm = q + torch.matmul(w, kw.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
    kwm = kw + torch.matmul(q.permute(0, 2, 1, 3), w).permute(0, 2, 1, 3)
    wf, wfw = cv.weightnet1(qm), cv.weightnet1(kwm)                                 # [B, 1, N1, K]
    cost_fwd = torch.sum(torch.softmax(wf, dim=3) * cq, dim=3)
    N2, Cc = xyz2.shape[2], cq.shape[1]
    ix = knn_idxw.reshape(Bn, -1).long()
    lg = wfw.reshape(Bn, -1)
    mx = torch.full((Bn, N2), float("-inf"), device=lg.device).scatter_reduce_(1, ix, lg, "amax", include_self=True)
    e = (lg - mx.gather(1, ix)).exp()
    wb = e / torch.zeros((Bn, N2), device=lg.device).scatter_add_(1, ix, e).gather(1, ix)
    v = ckw.reshape(Bn, Cc, -1) * wb[:, None, :]
    cost_bwd = torch.zeros((Bn, Cc, N2), device=lg.device).scatter_add_(2, ix[:, None, :].expand_as(v), v)
    fwd = cost_fwd.reshape(Bn, N1, Cc).permute(0, 2, 1)                             # the view of soflow.py:490
    x = torch.cat([fwd[:, :, :, None].expand(-1, -1, -1, K), P.grouping_operation(cost_bwd, knn_idx)] + extra +
                  [direction], dim=1)
    for conv in cv.mlp_convs4:
        x = lrelu(conv(x))
    cost = x.max(-1)[0]
    for m in cv.flow_mlp_convs:
        cost = m(cost)
    flow = cv.fc(cost).clamp(-50.0, 50.0)
    if sf is not None:
        flow = flow + sf
    return cost_fwd, cost_bwd, cost, flow.clamp(-50.0, 50.0)


def timed(torch, fns, warmup, runs):
    ms = {name: [] for name, _ in fns}
    outs = {}
    for k in range(warmup + runs):
        for name, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[name] = fn()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return ms, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cv_bench.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    import torch
    from ssf import pointnet2 as P
    from ssf import tflow as F
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(20241020)
    torch.manual_seed(20241020)
    results = []
    with torch.no_grad():
        for lv in LEVELS:
            N = lv["N"]
            cfg = {k: lv[k] for k in ("nsample", "in_channel", "sf_channel", "mlp", "flow_mlp", "use_flow")}
            cv = F.CostVolume(**cfg).to(dev)
            xyz1 = torch.rand(B, 3, N, generator=gen) * 16 - 8
            move = torch.randn(B, 3, N, generator=gen) * 0.1
            xyz2 = torch.stack([(xyz1 + move)[b][:, torch.randperm(N, generator=gen)] for b in range(B)])
            xyz1, xyz2 = xyz1.to(dev), xyz2.to(dev)
            points1 = torch.randn(B, lv["in_channel"], N, generator=gen).to(dev)
            points2 = torch.randn(B, lv["in_channel"], N, generator=gen).to(dev)
            sf = sf_feat = xyz2w = None
            if lv["use_flow"]:
                sf = (move + torch.randn(B, 3, N, generator=gen) * 0.02).to(dev)
                sf_feat = torch.randn(B, lv["sf_channel"], N, generator=gen).to(dev)
                xyz2w = F.PointWarping()(xyz1, xyz2, sf, 5)
            args = (xyz1, xyz2, xyz2w, points1, points2, sf, sf_feat)
            ms, outs = timed(torch, (("fused", lambda: cv(*args)), ("unfused", lambda: unfused(torch, P, cv, *args))),
                             a.warmup, a.runs)
            row = dict(lv, B=B, runs=a.runs, warmup=a.warmup,
                       max_abs_diff=[float((x - y).abs().max()) for x, y in zip(outs["fused"], outs["unfused"])],
                       grouped_tensor_mb=B * lv["mlp"][-1] * N * lv["nsample"] * 4 / 1e6)
            for name in ms:
                row[name + "_median_ms"] = float(np.median(ms[name]))
                row[name + "_min_ms"] = float(np.min(ms[name]))
                row[name + "_max_ms"] = float(np.max(ms[name]))
            row["unfused_over_fused"] = row["unfused_median_ms"] / row["fused_median_ms"]
            print(json.dumps(row), flush=True)
            results.append(row)
        # one whole forward (seeded default initialisation; the time does not depend on the weights)
        net = F.TFlow().to(dev)
        pc1 = (torch.rand(B, 3, 8192, generator=gen) * 16 - 8).to(dev)
        pc2 = (pc1 + torch.randn(B, 3, 8192, generator=gen).to(dev) * 0.1).contiguous()
        ms, _ = timed(torch, (("tflow", lambda: net(pc1, pc2)),), a.warmup, a.runs)
        whole = dict(name="TFlow forward", B=B, N=8192, runs=a.runs, warmup=a.warmup,
                     median_ms=float(np.median(ms["tflow"])), min_ms=float(np.min(ms["tflow"])),
                     max_ms=float(np.max(ms["tflow"])))
        print(json.dumps(whole), flush=True)
    props = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/bench_cv.py", device=props.name, arch=props.gcnArchName,
               timing="HIP events around the Python call (index k-NN included in both variants), one sync per "
                      "sample, variants alternating in one process",
               unmeasured="the kernels alone (no kernel-trace run), B = 1, any counter, the unfused whole network",
               levels=results, tflow=whole)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the fused set-abstraction kernel (ssf_pn2_grouped_mlp_max, pointnet2.hip) against the
unfused device composition it replaces -- ssf_pn2_group_relative, then torch conv2d, affine, relu
per layer and max, which writes and re-reads a [B, C, S, K] tensor per step -- on the four
encoder layers of TFlow (sa1 to sa4, TFlowV3_Occlussion.py:70-77) at B = 2 (the two clouds of a
frame pair) and N = 8192 input points.

Inputs: uniform random clouds, centroids by furthest point sampling, neighbours by k-NN (so the
gathers have the locality of the real layer), seeded weights.  HIP events around each call on
the current stream, one synchronise per sample; the two variants alternate in one process;
warm-up first, median of --runs samples (>= 20).  Writes profiles/sa_bench.json."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ssf-slam_amd"))

B = 2
SHAPES = [dict(name="sa1", N=8192, S=2048, K=16, widths=[35, 32, 32, 64]),
          dict(name="sa2", N=2048, S=512, K=16, widths=[67, 64, 64, 128]),
          dict(name="sa3", N=512, S=256, K=16, widths=[131, 128, 128, 256]),
          dict(name="sa4", N=256, S=128, K=8, widths=[259, 256, 256, 512])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sa_bench.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    import torch
    from ssf import pointnet2 as P
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(20240611)
    results = []
    for sh in SHAPES:
        N, S, K, widths = sh["N"], sh["S"], sh["K"], sh["widths"]
        c = widths[0] - 3
        xyz = (torch.rand(B, 3, N, generator=gen) * 40 - 20).to(dev)
        feat = torch.randn(B, c, N, generator=gen).to(dev)
        xyz_t = xyz.permute(0, 2, 1).contiguous()
        new_xyz = P.gather_operation(xyz, P.furthest_point_sample(xyz_t, S))
        _, idx = P.knn(K, new_xyz.permute(0, 2, 1).contiguous(), xyz_t)
        ws = [(torch.randn(i, o, generator=gen) / i ** 0.5).to(dev) for i, o in zip(widths, widths[1:])]
        scs = [(torch.rand(o, generator=gen) + 0.5).to(dev) for o in widths[1:]]
        shs = [(torch.randn(o, generator=gen) * 0.2).to(dev) for o in widths[1:]]
        w4 = [w.t().contiguous()[:, :, None, None] for w in ws]

        def fused():
            return P.grouped_mlp_max(xyz, new_xyz, feat, idx, ws, scs, shs)

        def unfused():
            x = P.group_relative(xyz, new_xyz, feat, idx)
            for w, sc, sh in zip(w4, scs, shs):
                x = torch.relu(torch.nn.functional.conv2d(x, w) * sc[None, :, None, None] + sh[None, :, None, None])
            return x.max(-1)[0]

        ms = dict(fused=[], unfused=[])
        outs = {}
        for k in range(a.warmup + a.runs):
            for name, fn in (("fused", fused), ("unfused", unfused)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[name] = fn()
                e1.record()
                e1.synchronize()
                if k >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        diff = float((outs["fused"] - outs["unfused"]).abs().max())
        row = dict(sh, B=B, runs=a.runs, warmup=a.warmup, max_abs_diff=diff,
                   grouped_tensor_mb=B * max(widths) * S * K * 4 / 1e6)
        for name in ms:
            row[name + "_median_ms"] = float(np.median(ms[name]))
            row[name + "_min_ms"] = float(np.min(ms[name]))
            row[name + "_max_ms"] = float(np.max(ms[name]))
        row["unfused_over_fused"] = row["unfused_median_ms"] / row["fused_median_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)
    props = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/bench_sa.py", device=props.name, arch=props.gcnArchName,
               timing="HIP events, one sync per sample, variants alternating in one process",
               shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

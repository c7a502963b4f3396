#!/usr/bin/env python3
"""Time the ActiveSceneFlow chain (ssf.asf) and write profiles/asf_bench.json.

(a) The sampler, ssf_subsample_batch (k_subsample), on 512 clouds of 120 k points to 8192, against
    the torch op sequence that would replace it: torch.rand keys, topk(8192, largest=False, sorted)
    and a gather of the xyz into [F, 3, nb].  The parent has no sampler, so that composition is the
    yardstick; it draws other points (torch's generator), only the work is the same.
(b) One ASF pair end to end at n_points = 8192 from two 120 k clouds with foreground masks: the two
    sampler stages, the TFlow forward (seeded default initialisation; the time does not depend on
    the weights), the GMM mask and the float32 Kabsch, and the node's two publishes (host copies of
    the sampled cloud and of the pose row) -- and its two parts alone.

Nothing is asserted and no threshold is set.  HIP events around each call on the current stream,
one synchronise per sample; the variants alternate in one process; warm-up first, median of --runs
samples (>= 20)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ssf-slam_amd"))

F_CLOUDS, CLOUD, NB = 512, 120_000, 8192


def timed(torch, fns, warmup, runs):
    ms = {name: [] for name, _ in fns}
    for k in range(warmup + runs):
        for name, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return {name: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
            for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "asf_bench.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    import torch
    import ssf
    from ssf import asf
    dev = torch.device("cuda", 0)
    torch.manual_seed(20261020)
    fe = ssf.Frontend(64, device=0)
    with torch.no_grad():
        # (a) the sampler
        pts = (torch.rand(F_CLOUDS * CLOUD, 3, device=dev) * 100 - 50).contiguous()
        off, h_off = ssf.frame_offsets([CLOUD] * F_CLOUDS, dev)
        view = pts.view(F_CLOUDS, CLOUD, 3)

        def torch_ops():
            keys = torch.rand(F_CLOUDS, CLOUD, device=dev)
            idx = torch.topk(keys, NB, dim=1, largest=False, sorted=True)[1]
            xyz = torch.gather(view, 1, idx[:, :, None].expand(-1, -1, 3)).permute(0, 2, 1).contiguous()
            return idx.to(torch.int32), xyz

        sampler = timed(torch, (("k_subsample", lambda: asf.subsample(fe, pts, off, h_off, NB, 1234)),
                                ("torch_rand_topk_gather", torch_ops)), a.warmup, a.runs)
        sampler["torch_over_kernel"] = (sampler["torch_rand_topk_gather"]["median_ms"] /
                                        sampler["k_subsample"]["median_ms"])
        print(json.dumps(sampler), flush=True)
        del pts, view
        # (b) one pair end to end
        net = ssf.TFlow().to(dev)
        node = asf.ActiveSceneFlowNode(lambda topic, msg: None, net, frontend=fe, mode="gmm", n_points=NB)
        pos1 = (torch.rand(CLOUD, 3, device=dev) * torch.tensor([100.0, 100.0, 6.0], device=dev) -
                torch.tensor([50.0, 50.0, 3.0], device=dev)).contiguous()
        pos2 = (pos1 + torch.tensor([0.5, 0.05, 0.0], device=dev) + torch.randn(CLOUD, 3, device=dev) * 0.01).contiguous()
        fg1 = (torch.rand(CLOUD, device=dev) < 0.05).to(torch.uint8)
        fg2 = (torch.rand(CLOUD, device=dev) < 0.05).to(torch.uint8)
        xyz = node.sample(pos1, pos2, fg1, fg2)[1]
        pair = timed(torch, (("on_pair", lambda: node.on_pair(pos1, pos2, (0, 0), fg1, fg2)),
                             ("two_stage_sample", lambda: node.sample(pos1, pos2, fg1, fg2)),
                             ("flow_mask_pose", lambda: asf.flow_mask_pose(net, fe, xyz[0:1], xyz[1:2]))),
                     a.warmup, a.runs)
        print(json.dumps(pair), flush=True)
    props = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/bench_asf.py", device=props.name, arch=props.gcnArchName, runs=a.runs, warmup=a.warmup,
               timing="HIP events around the Python call, one sync per sample, variants alternating in one process",
               unmeasured="the kernel alone (no kernel-trace run), any counter, trained weights, B > 1",
               sampler=dict(clouds=F_CLOUDS, points_per_cloud=CLOUD, nb=NB, **sampler),
               pair=dict(points_per_cloud=CLOUD, n_points=NB, mode="gmm", reference_loader=True, **pair))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

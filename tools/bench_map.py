#!/usr/bin/env python3
"""Time the map cloud of the loop-closure back-end (ssf.MapCloud, ssf_transform_clouds_batch in
loop.hip) at K = 1024 keyframes of 4096 plane points:

  (a) the one-launch rebuild of every keyframe (the ABI call, poses already on the device), and
      the same through MapCloud.transform (with the host pose rows and their upload);
  (b) the append of one keyframe (MapCloud.store + transform of that keyframe);
  (c) filtered(0.4) of the whole map (ssf_voxel_grid_batch on one cloud of K x 4096 points);
  (d) the per-keyframe torch path (loop.transform_cloud per keyframe, then torch.cat) for
      K = 1024, sampled alternately with (a), and for K = 21 (a local map).

HIP events around each call on the current stream, one synchronise per sample, warm-up first,
median of --runs samples (>= 20).  (a) is also reported as bytes per second: 32 B per point (one
float4 read, one float4 written) over its time, against the 6.3 TB/s a float4 copy reaches on
this part; at this shape the two buffers (2 x 64 MiB) fit in the 256 MiB Infinity Cache, so the
figure is not an HBM rate.  Writes profiles/map_bench.json.  --profile-only runs (c) a few times
and nothing else, for a separate `rocprofv3 --kernel-trace --stats` run; --merge-trace adds that
run's kernel statistics (the share of k_vg_bounds in the filter) to the timing file."""
import argparse
import ctypes as C
import hashlib
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ssf-slam_amd"))

K, M_PTS = 1024, 4096
HBM_COPY_BPS = 6.3e12


def keyframe_poses(n):
    """a drive of 1 m steps that turns back every 128 keyframes, lanes 20 m apart"""
    from ssf import loop
    Ts = []
    for k in range(n):
        lane, along = divmod(k, 128)
        x = along if lane % 2 == 0 else 127 - along
        yaw = (0.0 if lane % 2 == 0 else math.pi) + 0.05 * math.sin(0.1 * k)
        Ts.append(loop.get_transformation(float(x), 20.0 * lane, 0.02 * math.sin(0.3 * k), 0.01 * math.sin(0.2 * k),
                                          0.01 * math.cos(0.2 * k), yaw))
    return Ts


def timed(fn, warmup, runs, before=None):
    import torch
    ms = []
    for k in range(warmup + runs):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), samples=len(ms))


def merge_trace(csv_path, out_path):
    """The kernel statistics of a `rocprofv3 --kernel-trace --stats -- bench_map.py --profile-only`
    run into the timing file: the filter's kernels (k_vg_*, the hipCUB sort and scan) per
    filtered() call and the share of k_vg_bounds among them.  No device needed."""
    import csv
    with open(csv_path, newline="") as f:
        rows = list(csv.DictReader(f))
    filt = [r for r in rows if "k_vg_" in r["Name"] or "rocprim" in r["Name"]]
    bounds = [r for r in filt if "k_vg_bounds" in r["Name"]]
    if len(bounds) != 1:
        raise SystemExit(f"{csv_path}: no single k_vg_bounds row")
    calls = int(bounds[0]["Calls"])
    total = sum(int(r["TotalDurationNs"]) for r in filt) / calls
    b = int(bounds[0]["TotalDurationNs"]) / calls
    with open(out_path) as f:
        out = json.load(f)
    out["c_filtered_0p4"]["kernel_trace"] = dict(
        source=os.path.relpath(csv_path, REPO), run="separate rocprofv3 --kernel-trace --stats run of --profile-only",
        filtered_calls=calls, filter_kernels_us_per_call=total / 1e3, k_vg_bounds_us_per_call=b / 1e3,
        k_vg_bounds_share=b / total)
    tf = [r for r in rows if "k_transform_clouds" in r["Name"]]
    if tf:                                                  # the map build of that run: one cold launch
        ns = int(tf[0]["TotalDurationNs"]) / int(tf[0]["Calls"])
        out["a_rebuild_abi"]["kernel_trace"] = dict(
            source=os.path.relpath(csv_path, REPO), launches=int(tf[0]["Calls"]), k_transform_clouds_us=ns / 1e3,
            bytes_per_s=out["a_rebuild_abi"]["bytes"] / (ns * 1e-9),
            share_of_float4_copy_rate=out["a_rebuild_abi"]["bytes"] / (ns * 1e-9) / HBM_COPY_BPS)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["c_filtered_0p4"]["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_bench.json"))
    ap.add_argument("--profile-only", action="store_true",
                    help="build the map, run filtered(0.4) --runs times and exit (for a kernel trace)")
    ap.add_argument("--merge-trace", default=None, metavar="KERNEL_STATS_CSV",
                    help="no GPU work: add the filter's kernel shares from that trace to --out")
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.out)
    if a.runs < 20 and not a.profile_only:
        ap.error("--runs must be at least 20")
    import torch
    from ssf import Frontend, MapCloud, _abi, loop
    from ssf.frontend import _ptr, _stream
    from ssf.map_cloud import pose_rows
    dev = torch.device("cuda", 0)
    fe = Frontend(64, device=dev)
    spare = a.warmup + a.runs + 1                           # keyframes appended by (b)
    mc = MapCloud(fe, capacity_points=(K + spare) * M_PTS, capacity_keyframes=K + spare)
    gen = torch.Generator(device="cpu").manual_seed(7)
    clouds = []
    for k in range(K + spare):                              # a plane cloud: +-40 m around the sensor, +-3 m high
        c = torch.rand((M_PTS, 4), generator=gen) * torch.tensor([80.0, 80.0, 6.0, 1800.0]) - torch.tensor([40.0, 40.0, 3.0, 0.0])
        clouds.append(c.to(dev))
    Ts = keyframe_poses(K + spare)
    for k in range(K):
        mc.store(clouds[k])
    mc.transform(0, K, Ts[:K])
    torch.cuda.synchronize()
    n = mc.n_points
    assert n == K * M_PTS and mc.generation == 0

    if a.profile_only:
        for _ in range(a.runs):
            out = mc.filtered(0.4)
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_only=True, calls=a.runs, points=n, voxels=int(out.shape[0]))))
        return

    L = _abi.lib()
    d_T = torch.from_numpy(pose_rows(Ts[:K])).to(dev)

    def rebuild_abi():
        fe._check(L.ssf_transform_clouds_batch(fe._h, _stream(dev), K, _ptr(mc.raw), _ptr(mc.d_off),
                                               C.c_void_p(mc.h_off.data_ptr()), _ptr(d_T), _ptr(mc.mapped)),
                  "ssf_transform_clouds_batch")

    def torch_path(count):
        def run():
            return torch.cat([loop.transform_cloud(clouds[k], Ts[k]) for k in range(count)])
        return run

    # (a) and (d, K = 1024) alternate sample by sample
    ms_a, ms_d = [], []
    torch_full = torch_path(K)
    for k in range(a.warmup + a.runs):
        sa = timed(rebuild_abi, 0, 1)
        sd = timed(torch_full, 0, 1)
        if k >= a.warmup:
            ms_a += sa
            ms_d += sd
    want = torch_full()
    same = bool(torch.equal(want.view(torch.int32), mc.points().view(torch.int32)))
    del want
    ms_a2 = timed(lambda: mc.transform(0, K, Ts[:K]), a.warmup, a.runs)
    ms_d21 = timed(torch_path(21), a.warmup, a.runs)
    # (c) before (b) changes the map
    ms_c = timed(lambda: mc.filtered(0.4), a.warmup, a.runs)
    voxels = int(mc.filtered(0.4).shape[0])
    # (b) each sample appends one more keyframe
    state = dict(k=K)

    def append():
        k = state["k"]
        mc.store(clouds[k])
        mc.transform(k, k + 1, [Ts[k]])
        state["k"] = k + 1

    ms_b = timed(append, a.warmup, a.runs)
    assert mc.generation == 0                               # nothing was reallocated on the way

    ra = stats(ms_a)
    nbytes = 32 * n
    ra.update(bytes=nbytes, bytes_per_s=nbytes / (ra["median_ms"] * 1e-3),
              share_of_float4_copy_rate=nbytes / (ra["median_ms"] * 1e-3) / HBM_COPY_BPS,
              note="32 B per point over the median; 2 x 64 MiB fit in the Infinity Cache, not an HBM rate")
    with open(_abi.LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()[:16]
    prop = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/bench_map.py", device=prop.name, arch=prop.gcnArchName, lib_sha16=sha,
               timing="HIP events, one sync per sample", runs=a.runs, warmup=a.warmup,
               keyframes=K, points_per_keyframe=M_PTS, points=n,
               a_rebuild_abi=ra, a_rebuild_map_cloud_transform=stats(ms_a2),
               b_append_one_keyframe=stats(ms_b),
               c_filtered_0p4=dict(stats(ms_c), voxels=voxels),   # kernel shares: --merge-trace
               d_torch_per_keyframe_k1024=dict(stats(ms_d), alternated_with="a_rebuild_abi", same_bits_as_map=same),
               d_torch_per_keyframe_k21=stats(ms_d21),
               speedup_a_over_d_k1024=float(np.median(ms_d) / np.median(ms_a)))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

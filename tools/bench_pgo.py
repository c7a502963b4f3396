#!/usr/bin/env python3
"""Time ssf_pose_graph_batch (pose_graph.hip): many medium graphs in one launch (G=256, K=512,
L=8: the bench configuration's 256 sequences per GPU closing a loop together), one long graph at
the limit of the lane-per-column kernel (G=1, K=4096, L=32), and graphs of the wide kernel: the
long graph at L = 33, 64 and 256 and a batch (G=64, K=512) at L = 64, each with its ratio to
the L = 32 line of the same G and K (`--only` picks lines by name).

HIP events around the ABI call on the current stream, one synchronise per sample, warm-up
first, median of --runs samples (>= 20).  Every sample starts from the same drifted poses (a
device-to-device copy outside the timed region).  Writes profiles/pgo_bench.json.

--robust KIND[:K] times ssf_pose_graph_batch_robust with that loss on the loop edges (and the
per-edge output) against the plain call instead: the `batch` and `long` lines, plain and robust
alternated in one process, three runs of each (every run: warm-up, then the median of --runs
samples).  Writes profiles/pgo_robust_bench.json.

--lm [RADIUS0] times ssf_pose_graph_batch_lm (step control, no loss, RADIUS0 default 1e4) against
the plain call by the same protocol, and reports the time of an attempt over the time of a plain
iteration (each call's median over the largest iteration / attempt count of its graphs).  Writes
profiles/pgo_lm_bench.json."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ssf-slam_amd"))

SHAPES = [dict(name="batch", G=256, K=512, L=8), dict(name="long", G=1, K=4096, L=32),
          dict(name="long_l33", G=1, K=4096, L=33, ref="long"), dict(name="long_l64", G=1, K=4096, L=64, ref="long"),
          dict(name="long_l256", G=1, K=4096, L=256, ref="long"),
          dict(name="batch64_l32", G=64, K=512, L=32), dict(name="batch64_l64", G=64, K=512, L=64, ref="batch64_l32")]


def circle(K, L, seed):
    """A drifting circle with L inconsistent loop edges, vectorised (q xyzw, t)."""
    rng = np.random.default_rng(seed)
    a = 2 * math.pi * np.arange(K) / K * 0.98
    r = max(5.0, K / 6.0)

    def pose(yaw, x, y):
        return np.stack([0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2), x, y, 0 * yaw], 1)

    def between(p, q):                                   # planar: yaw difference, rotated offset
        yp, yq = 2 * np.arctan2(p[:, 2], p[:, 3]), 2 * np.arctan2(q[:, 2], q[:, 3])
        dx, dy = q[:, 4] - p[:, 4], q[:, 5] - p[:, 5]
        return pose(yq - yp, np.cos(yp) * dx + np.sin(yp) * dy, -np.sin(yp) * dx + np.cos(yp) * dy)

    gt = pose(a + math.pi / 2, r * np.cos(a), r * np.sin(a))
    meas = between(gt[:-1], gt[1:])
    yaw_m = 2 * np.arctan2(meas[:, 2], meas[:, 3]) + rng.normal(2e-4, 5e-4, K - 1)
    meas = pose(yaw_m, meas[:, 4] + rng.normal(0, 5e-3, K - 1), meas[:, 5] + rng.normal(0, 5e-3, K - 1))
    poses = [gt[0]]
    yaw, x, y = a[0] + math.pi / 2, gt[0, 4], gt[0, 5]
    for m, ym in zip(meas, yaw_m):
        x, y = x + math.cos(yaw) * m[4] - math.sin(yaw) * m[5], y + math.sin(yaw) * m[4] + math.cos(yaw) * m[5]
        yaw += ym
        poses.append(pose(np.array([yaw]), np.array([x]), np.array([y]))[0])
    poses = np.array(poses)
    li = np.sort(rng.choice(np.arange(K // 2, K), L, replace=False))
    lj = rng.integers(0, K // 4, L)
    lm = between(gt[li], gt[lj])
    lm[:, 4:6] += rng.normal(0, 0.02, (L, 2))
    ij = np.concatenate([np.stack([np.arange(K - 1), np.arange(1, K)], 1), np.stack([li, lj], 1)]).astype(np.int32)
    var = np.concatenate([np.tile([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4], (K - 1, 1)), np.full((L, 6), 0.05)])
    return dict(poses=poses, edge_ij=ij, edge_meas=np.concatenate([meas, lm]), edge_var=var,
                prior_pose=gt[0], prior_var=np.array([1e-2, 1e-2, math.pi ** 2, 1e8, 1e8, 1e8]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="default: profiles/pgo_bench.json (pgo_robust_bench.json with --robust)")
    ap.add_argument("--robust", default=None, metavar="KIND[:K]",
                    help="time this loss (huber, cauchy, geman_mcclure; K default 1.345 / 0.1 / 1.0) against the plain call")
    ap.add_argument("--lm", nargs="?", const="1e4", default=None, metavar="RADIUS0",
                    help="time the step control (initial radius RADIUS0, default 1e4) against the plain call")
    ap.add_argument("--only", default="", help="comma-separated line names (default: all)")
    a = ap.parse_args()
    only = [n for n in a.only.split(",") if n]
    if any(n not in [sh["name"] for sh in SHAPES] for n in only):
        ap.error(f"--only: unknown line in {only}")
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    if (a.robust or a.lm) and only:
        ap.error("--robust and --lm time the batch and long lines: no --only")
    if a.robust and a.lm:
        ap.error("--robust or --lm, not both")
    import torch
    from ssf import Frontend, _abi
    robust = None
    if a.robust:
        from ssf.loop import parse_robust
        try:
            robust = parse_robust(a.robust)
        except ValueError as e:
            ap.error(f"--robust: {e}")
        only = ["batch", "long"]
    lm = None
    if a.lm:
        from ssf.loop import parse_lm
        try:
            lm = parse_lm(a.lm)
        except ValueError as e:
            ap.error(f"--lm: {e}")
        only = ["batch", "long"]
    a.out = a.out or os.path.join(REPO, "profiles", "pgo_robust_bench.json" if robust else
                                  "pgo_lm_bench.json" if lm else "pgo_bench.json")
    from ssf.frontend import _ptr, _stream
    dev = torch.device("cuda", 0)
    fe = Frontend(64, device=dev)
    L = _abi.lib()
    prm = _abi.PgoParams()
    L.ssf_pgo_params_default(C.byref(prm))
    results, summary = [], []
    for sh in [sh for sh in SHAPES if not only or sh["name"] in only]:
        G, K, nl = sh["G"], sh["K"], sh["L"]
        gs = [circle(K, nl, 100 + (g % 8)) for g in range(min(G, 8))]
        gs = [gs[g % len(gs)] for g in range(G)]
        cat = lambda key, dt: torch.from_numpy(np.concatenate([np.asarray(g[key], dt) for g in gs])).to(dev)  # noqa: E731
        pose0, ij = cat("poses", np.float64), cat("edge_ij", np.int32)
        meas, var = cat("edge_meas", np.float64), cat("edge_var", np.float64)
        prior = torch.from_numpy(np.stack([g["prior_pose"] for g in gs])).to(dev)
        pvar = torch.from_numpy(np.stack([g["prior_var"] for g in gs])).to(dev)
        h_noff = torch.arange(G + 1, dtype=torch.int32) * K
        h_eoff = torch.arange(G + 1, dtype=torch.int32) * (K - 1 + nl)
        d_noff, d_eoff = h_noff.to(dev), h_eoff.to(dev)
        pose = pose0.clone()
        stats = torch.zeros(G, _abi.PGO_OUT_STRIDE, dtype=torch.float64, device=dev)
        eout = torch.zeros(G * (K - 1 + nl), _abi.PGO_EDGE_OUT_STRIDE, dtype=torch.float64, device=dev)

        def call(rb):
            if rb is lm and lm is not None:
                fe._check(L.ssf_pose_graph_batch_lm(
                    fe._h, _stream(dev), G, _ptr(pose), _ptr(d_noff), C.c_void_p(h_noff.data_ptr()), _ptr(ij),
                    _ptr(meas), _ptr(var), _ptr(d_eoff), C.c_void_p(h_eoff.data_ptr()), _ptr(prior), _ptr(pvar),
                    C.byref(prm), _ptr(stats), None, None, None, C.byref(lm), None), "ssf_pose_graph_batch_lm")
                return
            args = (fe._h, _stream(dev), G, _ptr(pose), _ptr(d_noff), C.c_void_p(h_noff.data_ptr()), _ptr(ij),
                    _ptr(meas), _ptr(var), _ptr(d_eoff), C.c_void_p(h_eoff.data_ptr()), _ptr(prior), _ptr(pvar),
                    C.byref(prm), _ptr(stats), None)
            if rb is None:
                fe._check(L.ssf_pose_graph_batch(*args), "ssf_pose_graph_batch")
            else:
                fe._check(L.ssf_pose_graph_batch_robust(*args, C.byref(rb), _ptr(eout)), "ssf_pose_graph_batch_robust")

        def sample(rb):
            ms = []
            for k in range(a.warmup + a.runs):
                pose.copy_(pose0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(rb)
                e1.record()
                e1.synchronize()
                if k >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
            st = stats.cpu().numpy()
            status = sorted(set(int(v) for v in st[:, 0]))
            row = dict(sh, runs=a.runs, warmup=a.warmup, median_ms=float(np.median(ms)), min_ms=float(np.min(ms)),
                       max_ms=float(np.max(ms)), iterations=sorted(set(int(v) for v in st[:, 1])),
                       status=[_abi.PGO_STATUS[s] for s in status], cost0=float(st[0, 2]), cost=float(st[0, 3]),
                       max_iter=prm.max_iter, func_tol=prm.func_tol)
            if rb is lm and lm is not None:
                row["accepted"] = sorted(set(int(v) for v in st[:, _abi.PGO_OUT["ACCEPTED"]]))
            if any(s not in (_abi.PGO_OK, _abi.PGO_CONVERGED) for s in status):
                raise SystemExit(f"{sh['name']}: a graph failed: {row['status']}")
            return row

        if robust is not None:                       # plain and robust in turn, three runs of each
            for rep in range(3):
                for label, rb in (("plain", None), (a.robust, robust)):
                    row = dict(sample(rb), loss=label, rep=rep)
                    print(json.dumps(row), flush=True)
                    results.append(row)
            med = lambda label: [r["median_ms"] for r in results if r["name"] == sh["name"] and r["loss"] == label]  # noqa: E731
            summary.append(dict(name=sh["name"], plain_median_ms=med("plain"), robust_median_ms=med(a.robust),
                                plain_spread=max(med("plain")) / min(med("plain")) - 1.0,
                                robust_over_plain=float(np.median(med(a.robust)) / np.median(med("plain")))))
            print(json.dumps(summary[-1]), flush=True)
            continue
        if lm is not None:                           # plain and step control in turn, three runs of each
            for rep in range(3):
                for label, how in (("plain", None), ("lm", lm)):
                    row = dict(sample(how), solver=label, rep=rep)
                    print(json.dumps(row), flush=True)
                    results.append(row)
            rows = lambda label: [r for r in results if r["name"] == sh["name"] and r["solver"] == label]  # noqa: E731
            per = lambda label: float(np.median([r["median_ms"] / max(r["iterations"]) for r in rows(label)]))  # noqa: E731
            summary.append(dict(name=sh["name"], plain_median_ms=[r["median_ms"] for r in rows("plain")],
                                lm_median_ms=[r["median_ms"] for r in rows("lm")],
                                plain_iterations=rows("plain")[0]["iterations"], lm_attempts=rows("lm")[0]["iterations"],
                                lm_accepted=rows("lm")[0]["accepted"], plain_ms_per_iteration=per("plain"),
                                lm_ms_per_attempt=per("lm"), attempt_over_iteration=per("lm") / per("plain")))
            print(json.dumps(summary[-1]), flush=True)
            continue
        row = sample(None)
        ref = [r for r in results if r["name"] == sh.get("ref")]
        if ref:                                      # against the L = 32 line of the same G and K
            row["ratio_to_l32"] = row["median_ms"] / ref[0]["median_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)
    out = dict(tool="tools/bench_pgo.py", device=torch.cuda.get_device_properties(0).name,
               arch=torch.cuda.get_device_properties(0).gcnArchName, timing="HIP events, one sync per sample",
               shapes=results)
    if robust is not None:
        out.update(robust=a.robust, k=robust.k, protocol="plain and robust alternated, three runs of each", summary=summary)
    if lm is not None:
        out.update(lm=dict(radius0=lm.radius0, min_relative_decrease=lm.min_relative_decrease,
                           max_radius=lm.max_radius, min_radius=lm.min_radius),
                   protocol="plain and step control alternated, three runs of each", summary=summary)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""python -m ssf.run DATASET_PATH [--launch noSeg] [--tum traj.txt]: replay an npz scene-flow
sequence through the device front-end as one of the reference's launch files wires its nodes
(launch/run_onlyPC.launch, run_noSeg.launch, run_Seg.launch, run_noSeg_ActiveSceneFlow.launch,
run_Seg_ActiveSceneFlow.launch with --weights; ssf.nodes.LAUNCH_GRAPHS) and append
/frame_odom2 to a TUM trajectory (optionally with mapOptmization's loop closure, with
--map-cloud its accumulated map cloud saved as an npy file, and with --map-detector scan-context
its loops found by Scan Context descriptors instead of the radius search, with
--map-sc-candidates K the K best places verified by ICP in one batch)."""
from __future__ import annotations

import argparse
import json

import torch


def main(argv=None):
    from .nodes import LAUNCH_GRAPHS
    ap = argparse.ArgumentParser(prog="python -m ssf.run")
    ap.add_argument("dataset_path", help="directory of npz frames (pos1, gt = flow, s_fg_mask)")
    ap.add_argument("--launch", default="noSeg", choices=sorted(LAUNCH_GRAPHS),
                    help="node graph of launch/run_<launch>.launch")
    ap.add_argument("--tum", default=None, help="TUM output (stamp x y z qx qy qz qw), appended")
    ap.add_argument("--truncate", action="store_true", help="empty the TUM files first")
    ap.add_argument("--rows", type=int, default=64, choices=[16, 64])
    ap.add_argument("--solver", default="ceres_lm", choices=["ceres_lm", "gn"])
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None, help="np.random.seed for the GMM k-means++")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--map-tum", default=None,
                    help="also run mapOptmization (loop closure) and write its RESULT_PATH TUM file")
    ap.add_argument("--map-optimize", action="store_true",
                    help="with --map-tum: optimise the pose graph on a loop closure and rewrite the "
                         "keyframe poses (runOptimize / correctPoses)")
    ap.add_argument("--map-robust", default=None, metavar="KIND[:K]",
                    help="with --map-optimize: a robust loss on the loop edges of the pose graph, "
                         "huber, cauchy or geman_mcclure (or none), K its threshold (default 1.345 / "
                         "0.1 / 1.0)")
    ap.add_argument("--map-lm", nargs="?", const=True, default=None, metavar="RADIUS0",
                    help="with --map-optimize: Levenberg-Marquardt step control for the pose-graph solves "
                         "(no step that raises the cost is taken); RADIUS0 the initial trust-region radius "
                         "(default 1e4)")
    ap.add_argument("--map-iters", type=int, default=None, metavar="N",
                    help="with --map-optimize: the iteration limit of the pose-graph solves (default 8); "
                         "with --map-lm it bounds the attempts")
    ap.add_argument("--map-cloud", default=None, metavar="FILE.npy",
                    help="with --map-tum: keep the accumulated map cloud on the GPU, publish its 0.4 m "
                         "VoxelGrid on /sum_map_cloud_res3 and save the final one as float32 [M, 4]")
    ap.add_argument("--map-detector", default=None, metavar="radius|scan-context[:THRESHOLD]",
                    help="with --map-tum: how mapOptmization finds loops; radius (default) is the "
                         "reference's 15 m search over the estimated key positions, scan-context compares "
                         "Scan Context descriptors of the raw scans on the GPU and also finds a loop "
                         "after the odometry has drifted; THRESHOLD the acceptance distance (default 0.13)")
    ap.add_argument("--map-sc-candidates", default=None, metavar="K[:EXCLUSION]",
                    help="with --map-detector scan-context: verify the K (1 .. 8) best places by ICP in one "
                         "batch and close the loop at the one with the best fitness, instead of trying "
                         "only the nearest descriptor; no two places lie within EXCLUSION keyframes of "
                         "each other (default 10, the half-width of a local map)")
    ap.add_argument("--weights", default=None, metavar="FILE",
                    help="the ActiveSceneFlow launches: TFlow checkpoint (a state dict with the "
                         "reference's keys, a DataParallel `module.` prefix accepted)")
    ap.add_argument("--n-points", type=int, default=8192,
                    help="the ActiveSceneFlow launches: points per cloud the network takes")
    ap.add_argument("--rate-hz", type=float, default=10.0,
                    help="frame rate of the synthetic stamps (frame k at k / rate)")
    a = ap.parse_args(argv)
    from .nodes import run_sequence
    import os
    import sys
    if a.tum and os.path.exists(a.tum) and not a.truncate:
        print(f"ssf.run: appending to the existing {a.tum} (the reference's std::ios::app); "
              f"--truncate starts a new file", file=sys.stderr)
    if a.map_cloud and a.map_tum is None:
        ap.error("--map-cloud needs --map-tum")
    kw = dict(map_cloud=True) if a.map_cloud else {}
    if a.map_robust is not None:
        if not a.map_optimize:
            ap.error("--map-robust needs --map-optimize")
        from .loop import parse_robust
        try:
            kw["map_robust"] = parse_robust(a.map_robust)
        except ValueError as e:
            ap.error(f"--map-robust: {e}")
    if a.map_lm is not None:
        if not a.map_optimize:
            ap.error("--map-lm needs --map-optimize")
        from .loop import parse_lm
        try:
            kw["map_lm"] = parse_lm(a.map_lm)
        except ValueError as e:
            ap.error(f"--map-lm: {e}")
    if a.map_iters is not None:
        if not a.map_optimize:
            ap.error("--map-iters needs --map-optimize")
        if a.map_iters <= 0:
            ap.error("--map-iters: must be positive")
        kw["map_iters"] = a.map_iters
    detector = None
    if a.map_detector is not None:
        if a.map_tum is None:
            ap.error("--map-detector needs --map-tum")
        from .scan_context import parse_detector
        try:
            detector, thr = parse_detector(a.map_detector)
        except ValueError as e:
            ap.error(f"--map-detector: {e}")
        kw["map_detector"] = detector
        if thr is not None:
            kw["map_sc_threshold"] = thr
    if a.map_sc_candidates is not None:
        if detector != "scan_context":
            ap.error("--map-sc-candidates needs --map-detector scan-context[:THRESHOLD]: the candidates are "
                     "those of the Scan Context search")
        from .scan_context import parse_candidates
        try:
            kw["map_sc_candidates"], kw["map_sc_exclusion"] = parse_candidates(a.map_sc_candidates)
        except ValueError as e:
            ap.error(f"--map-sc-candidates: {e}")
    torch.cuda.set_device(a.device)
    from .nodes import ASF_LAUNCHES
    if a.launch in ASF_LAUNCHES:
        if a.weights is None:
            ap.error(f"--launch {a.launch} needs --weights (no trained weights ship with the project)")
        kw.update(weights=a.weights, n_points=a.n_points)
    res = run_sequence(a.dataset_path, a.tum, n_rows=a.rows, solver=a.solver, max_iter=a.iters,
                       seed=a.seed, launch=a.launch, map_tum_path=a.map_tum, map_optimize=a.map_optimize,
                       truncate_results=a.truncate, rate_hz=a.rate_hz, **kw)
    extra = {}
    if a.map_optimize:
        opt = res["optimization"]
        extra = {"map_optimize": None if opt is None else
                 {k: opt[k] for k in ("status_name", "iterations", "cost0", "cost", "loops")}}
        if a.map_robust is not None and opt is not None:
            extra["map_optimize"]["robust"] = a.map_robust
        if a.map_lm is not None and opt is not None:
            extra["map_optimize"]["lm"] = kw["map_lm"].radius0
            extra["map_optimize"].update(accepted=opt["accepted"], radius=opt["radius"])
        if a.map_iters is not None and opt is not None:
            extra["map_optimize"]["iters"] = a.map_iters
    if a.map_cloud:
        import numpy as np
        with open(a.map_cloud, "wb") as f:           # the name as given (np.save appends .npy to a path)
            np.save(f, res["map_cloud"])
        extra["map_cloud"] = {"file": a.map_cloud, "points": int(res["map_cloud"].shape[0]),
                              "keyframes": int(res["map_cloud_keyframes"])}
    if detector is not None:                         # "loops" below: the loops it closed
        extra["map_detector"] = {"detector": detector, "loops_closed": len(res["loops"])}
        if detector == "scan_context":
            extra["map_detector"].update(
                threshold=kw.get("map_sc_threshold", 0.13),
                matches=[{"key_cur": c.key_cur, "key_pre": c.key_pre, "dist": c.dist, "shift": c.shift}
                         for c in res["loops"]])
            if a.map_sc_candidates is not None:      # per closed loop: the places ICP was tried at
                extra["map_detector"].update(
                    candidates=kw["map_sc_candidates"], exclusion=kw["map_sc_exclusion"],
                    candidates_tried=[[{"key_pre": k, "dist": d, "shift": s, "fitness": f, "converged": ok}
                                       for k, d, s, f, ok in (c.candidates or [])] for c in res["loops"]])
    if res.get("flow_metrics"):                     # the dataset carries gt: the mean of each metric
        fm = res["flow_metrics"]
        extra["flow_metrics"] = {k: sum(m[k] for m in fm) / len(fm) for k in fm[0]}
    print(json.dumps({"launch": a.launch, "tum": a.tum, "tum_mode": "truncate" if a.truncate else "append",
                      "frames": len(res["stamps"]),
                      "odom1_poses": int(res["odom1"].shape[0]),
                      "odom2_poses": int(res["odom2"].shape[0]),
                      "final_t": res["odom2"][-1, 0:3].tolist() if len(res["odom2"]) else None,
                      "loops": len(res["loops"]), **extra}))


if __name__ == "__main__":
    main()

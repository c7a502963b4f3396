#!/usr/bin/env python3
"""Time the Scan Context loop detector (ssf.scan_context) and write profiles/sc_bench.json.

(a) The descriptor, ssf_scan_context_batch (k_sc_describe), on 256 clouds of 120 k points, xyz
    and xyzi rows.
(b) The exhaustive search, ssf_scan_context_match (k_sc_match + k_sc_select), of 1 query and of 64
    queries against 8192 descriptors, selection only (what LoopCloser calls) and with every
    pair's dist / shift written -- beside the torch op sequence that does the same exhaustive
    search: unit columns, then for each of the 60 shifts a roll of the database and an einsum over
    (ring, column), a min over the shifts and an argmin over the candidates.  The parent commit
    has no detector, so that composition is the comparison; its distances are compared with the
    kernel's (the largest difference is recorded, nothing is asserted).

--topk writes profiles/sc_topk_bench.json instead: (c) ssf_scan_context_match against
ssf_scan_context_match_topk at k = 1, 4 and 8, selection only, and (d) the batched verification of
four candidates (LoopCloser.verify_candidates) against four sequential local_map + icp pairs on the
revisit scene of the loop tests.

No threshold is set.  HIP events around each Python call on the current stream, one synchronise per
sample; the variants alternate in one process; warm-up first, median of --runs samples (>= 20)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ssf-slam_amd"))

F_CLOUDS, CLOUD, N_DB = 256, 120_000, 8192


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


def torch_match(torch, q, db):
    """The same exhaustive search in torch ops -> (idx [Q], dist [Q, N], shift [Q, N])."""
    def unit(d):
        n = d.norm(dim=1, keepdim=True)
        return torch.where(n > 0, d / n.clamp_min(1e-30), torch.zeros_like(d)), (d > 0).any(dim=1).float()
    qn, qv = unit(q)
    cn, cv = unit(db)
    ds = []
    for s in range(60):
        num = torch.einsum("qkj,nkj->qn", qn, torch.roll(cn, -s, dims=2))
        cnt = qv @ torch.roll(cv, -s, dims=1).T
        ds.append(torch.where(cnt > 0, 1.0 - num / cnt.clamp_min(1.0), torch.ones_like(num)))
    dist, shift = torch.stack(ds, dim=2).min(dim=2)
    return dist.argmin(dim=1), dist, shift


def revisit_closer(torch, ssf, fe, dev, k_cand, exclusion):
    """The revisit scene of the loop tests (30 synthetic frames forward, n_az = 600; the plane
    clouds from the device's own feature stage) in a LoopCloser, the revisit of frame 0 (yawed by
    180 degrees, 40 m of drift) as its last keyframe, and k_cand candidates for it from
    query_topk with no threshold applied (a window of `exclusion` keyframes: the scene has some
    20 keyframes, too few for k_cand places 11 apart) -> (closer, cur, candidates)."""
    from ssf import loop, scan_context as sc, synth
    scene = synth.Scene(0)
    scans = [synth.scan(0, k, n_az=600, scene=scene)["pos1"] for k in range(30)]
    turned = scans[0].clone()
    turned[:, :2] = -turned[:, :2]
    scans.append(turned)
    R0, p0 = synth.ego_pose(0, 0)
    T0 = np.eye(4); T0[:3, :3] = R0.numpy(); T0[:3, 3] = p0.numpy()
    pts = torch.cat(scans).to(dev)
    off, h_off = ssf.frame_offsets([s.shape[0] for s in scans], dev)
    pb = fe.extract_planes_batch(pts, off, h_off)
    lc = loop.LoopCloser(fe, detector="scan_context", sc=sc.sc_params(threshold=0.0), sc_candidates=k_cand)
    for i in range(31):
        R, p = synth.ego_pose(0, i % 30)
        T = np.eye(4); T[:3, :3] = R.numpy(); T[:3, 3] = p.numpy()
        T = np.linalg.inv(T0) @ T
        if i == 30:
            T = T @ loop.get_transformation(0, 0, 0, 0, 0, np.pi)
            T[1, 3] += 40.0
        yaw = np.arctan2(T[1, 0], T[0, 0])
        lc.process(pb.frame(i).clone(), (0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)), T[:3, 3],
                   0.1 * i + (30.0 if i == 30 else 0.0), scan=scans[i].to(dev))   # threshold 0: nothing is accepted
    cur = len(lc.key6d) - 1
    cands = lc.sc_db.query_topk(lc.sc_db.descriptors()[cur], k_cand, exclusion, cur)
    return lc, cur, cands


def topk(a):
    """--topk: (a) ssf_scan_context_match against ssf_scan_context_match_topk at k = 1, 4 and 8,
    selection only, 8192 descriptors, 1 and 64 queries; (b) the verification of K = 4 candidates
    on the revisit scene in one batch (LoopCloser.verify_candidates: local_maps + one icp_batch)
    against four sequential local_map + icp pairs.  The same protocol as the default mode."""
    import math
    import torch
    import ssf
    from ssf import loop, scan_context as sc
    dev = torch.device("cuda", 0)
    torch.manual_seed(20261021)
    fe = ssf.Frontend(64, device=0)
    with torch.no_grad():
        m = 3000
        r, phi = torch.rand((N_DB + 64) * m, device=dev) * 80.0, torch.rand((N_DB + 64) * m, device=dev) * (2 * np.pi)
        pts = torch.stack([r * torch.cos(phi), r * torch.sin(phi), torch.rand_like(r) * 10.0 - 2.0], dim=1).contiguous()
        o2, h2 = ssf.frame_offsets([m] * (N_DB + 64), dev)
        descs = sc.describe(fe, pts, o2, h2)
        del pts, r, phi
        db, queries = descs[:N_DB].contiguous(), descs[N_DB:].contiguous()
        select = {}
        for Q in (1, 64):
            q = queries[:Q].contiguous()
            res = timed(torch, (("match", lambda: sc.match(fe, q, db, N_DB)),
                                ("topk_k1", lambda: sc.match_topk(fe, q, db, N_DB, 1, 10)),
                                ("topk_k4", lambda: sc.match_topk(fe, q, db, N_DB, 4, 10)),
                                ("topk_k8", lambda: sc.match_topk(fe, q, db, N_DB, 8, 10))), a.warmup, a.runs)
            for k in (1, 4, 8):
                res[f"topk_k{k}_over_match"] = res[f"topk_k{k}"]["median_ms"] / res["match"]["median_ms"]
            one = sc.match(fe, q, db, N_DB)
            top = sc.match_topk(fe, q, db, N_DB, 8, 10)
            res["slot0_equals_match"] = bool(all(torch.equal(x, y[:, 0]) for x, y in zip(one, top)))
            select[f"q{Q}"] = dict(queries=Q, exclusion=10, **res)
            print(json.dumps(select[f"q{Q}"]), flush=True)
        lc, cur, cands = revisit_closer(torch, ssf, fe, dev, 4, 4)
        inv_cur = np.linalg.inv(lc._T6(cur))

        def sequential():
            out = []
            for pre, _, shift in cands:
                cur_cloud, pre_cloud = lc.local_map(cur, 0), lc.local_map(pre, lc.search_num)
                g = lc._T6(pre) @ loop.get_transformation(0.0, 0.0, 0.0, 0.0, 0.0, shift * (2.0 * math.pi / 60.0)) @ inv_cur
                out.append(loop.icp(fe, cur_cloud, pre_cloud, guess=g))
            return out
        verify = timed(torch, (("batched", lambda: lc.verify_candidates(cur, cands)), ("sequential", sequential)),
                       a.warmup, a.runs)
        verify["sequential_over_batched"] = verify["sequential"]["median_ms"] / verify["batched"]["median_ms"]
        bat, seq = lc.verify_candidates(cur, cands), sequential()
        verify["candidates"] = [dict(key_pre=cands[j][0], dist=cands[j][1], shift=cands[j][2], fitness_batched=b["fitness"],
                                     iterations_batched=b["iterations"], fitness_sequential=seq[j]["fitness"],
                                     iterations_sequential=seq[j]["iterations"]) for j, b in bat]
        verify["exclusion"] = 4
        verify["keyframes"] = len(lc.key6d)
        print(json.dumps(verify), flush=True)
    props = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/bench_sc.py --topk", device=props.name, arch=props.gcnArchName, runs=a.runs, warmup=a.warmup,
               timing="HIP events around the Python call (its small host copies and allocations included; "
                      "ssf_icp_batch is synchronous), one sync per sample, variants alternating in one process",
               unmeasured="the kernels alone (no kernel-trace run), any counter, K other than 4 for the verification",
               select=dict(database=N_DB, **select), verify=dict(k=4, **verify))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--topk", action="store_true",
                    help="time the top-K selection and the batched candidate verification instead "
                         "(default --out: profiles/sc_topk_bench.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "sc_topk_bench.json" if a.topk else "sc_bench.json")
    if a.topk:
        return topk(a)
    import torch
    import ssf
    from ssf import scan_context as sc
    dev = torch.device("cuda", 0)
    torch.manual_seed(20261021)
    fe = ssf.Frontend(64, device=0)
    with torch.no_grad():
        # (a) the descriptor: ranges to 90 m (some beyond max_range), heights -2.5 .. 8 m
        n = F_CLOUDS * CLOUD
        r, phi = torch.rand(n, device=dev) * 90.0, torch.rand(n, device=dev) * (2 * np.pi)
        xyzi = torch.stack([r * torch.cos(phi), r * torch.sin(phi), torch.rand(n, device=dev) * 10.5 - 2.5,
                            torch.rand(n, device=dev)], dim=1).contiguous()
        xyz = xyzi[:, :3].contiguous()
        del r, phi
        off, h_off = ssf.frame_offsets([CLOUD] * F_CLOUDS, dev)
        describe = timed(torch, (("k_sc_describe_xyz", lambda: sc.describe(fe, xyz, off, h_off)),
                                 ("k_sc_describe_xyzi", lambda: sc.describe(fe, xyzi, off, h_off))), a.warmup, a.runs)
        describe["gbytes_per_s_xyz"] = n * 12 / describe["k_sc_describe_xyz"]["median_ms"] / 1e6
        describe["gbytes_per_s_xyzi"] = n * 16 / describe["k_sc_describe_xyzi"]["median_ms"] / 1e6
        print(json.dumps(describe), flush=True)
        del xyz, xyzi
        # (b) the search: descriptors of 8192 + 64 sparse clouds
        m = 3000
        r, phi = torch.rand((N_DB + 64) * m, device=dev) * 80.0, torch.rand((N_DB + 64) * m, device=dev) * (2 * np.pi)
        pts = torch.stack([r * torch.cos(phi), r * torch.sin(phi), torch.rand_like(r) * 10.0 - 2.0], dim=1).contiguous()
        o2, h2 = ssf.frame_offsets([m] * (N_DB + 64), dev)
        descs = sc.describe(fe, pts, o2, h2)
        del pts, r, phi
        db, queries = descs[:N_DB].contiguous(), descs[N_DB:].contiguous()
        match = {}
        for Q in (1, 64):
            q = queries[:Q].contiguous()
            res = timed(torch, (("select_only", lambda: sc.match(fe, q, db, N_DB)),
                                ("all_pairs", lambda: sc.match(fe, q, db, N_DB, full=True)),
                                ("torch_roll_einsum", lambda: torch_match(torch, q, db))), a.warmup, a.runs)
            idx, _, _, dist, shift = sc.match(fe, q, db, N_DB, full=True)
            tidx, tdist, tshift = torch_match(torch, q, db)
            res["torch_over_select_only"] = res["torch_roll_einsum"]["median_ms"] / res["select_only"]["median_ms"]
            res["pairs_per_s_select_only"] = Q * N_DB / res["select_only"]["median_ms"] * 1e3
            res["max_abs_dist_difference"] = float((dist - tdist).abs().max())
            res["same_best"] = int((idx.long() == tidx).sum())
            res["same_shift_fraction"] = float((shift.long() == tshift).float().mean())
            match[f"q{Q}"] = dict(queries=Q, **res)
            print(json.dumps(match[f"q{Q}"]), flush=True)
    props = torch.cuda.get_device_properties(0)
    out = dict(tool="tools/bench_sc.py", device=props.name, arch=props.gcnArchName, runs=a.runs, warmup=a.warmup,
               timing="HIP events around the Python call (its small host copies and allocations included), one "
                      "sync per sample, variants alternating in one process",
               unmeasured="the kernels alone (no kernel-trace run), any counter, a VALU form of k_sc_match",
               describe=dict(clouds=F_CLOUDS, points_per_cloud=CLOUD, **describe),
               match=dict(database=N_DB, **match))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

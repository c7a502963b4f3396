"""k_plane_table*, the association and k_solve against the independent yardstick of
tests/registration_reference.py (jets, lstsq on the Jacobian, QR as mathematics) instead of the
CPU oracle that restates them line for line -- on the seeded cases of tests/registration_cases.py,
which tests/test_registration_host.py runs through the oracle with a tenth of these bars.

Every solve case carries a HAND-MADE plane table.  Launches are batched per family: brute-force
association (no search buffers), the group-mode association with the solve-side ballot compaction
(<= 16 pairs), and the lane-mode association that hands k_solve compacted records
(evaluate_load; the global-memory evaluate above 4096 records) -- each proven by
ssf.register_plan.  Asserted per pair: the 1-NN indices, the correspondence count, the number of
log rows and every status, every cost within 1e-9 relative, every logged pose and the final one
within 1e-5 m / 1e-6 rad of the yardstick, pose_abs against the yardstick's composition.
Rank-deficient pairs compare the pose projected on the row space of J through the last clear
decision and print their null-space displacement.
"""
import numpy as np
import pytest
import torch

import registration_cases as rc
import registration_reference as ref

pytestmark = pytest.mark.gpu

ABS0 = np.r_[rc.axis_angle_quat([0.3, 1.0, -0.2], 0.7), 12.0, -3.0, 0.5]


def _batch(dev, frames, bound):
    import ssf
    xyzi = torch.from_numpy(np.concatenate(frames).astype(np.float32)).to(dev)
    counts = [len(f) for f in frames]
    off, h_off = ssf.frame_offsets(counts, dev)
    return ssf.PlaneBatch(xyzi, torch.tensor(counts, dtype=torch.int32, device=dev), off, h_off, bound)


def _views(pb, P, dev):
    """frames 0 .. P-1 of pb are the current frames (pair p's records live at its offset), frames
    P .. 2P-1 the last frames"""
    import ssf
    h = [int(v) for v in pb.h_off]

    def view(lo):
        o = torch.tensor(h[lo:lo + P] + [h[lo + P]], dtype=torch.int64)
        return ssf.PlaneBatch(pb.xyzi, pb.count[lo:lo + P].contiguous(), o.to(dev), o, pb.max_points)
    return view(P), view(0)


def _launch(dev, cases, table_mode, bound=None):
    """One register() launch of `cases` (one solver, one max_iter).  table_mode: "brute" (no search
    buffers), "sorted" (plane_table's buffers, normal / valid overwritten in place), "own_strips"
    (sorted without the table's strip image: the association builds its strips itself)."""
    import ssf
    solver, iters = cases[0].solver, cases[0].max_iter
    assert all(c.solver == solver and c.max_iter == iters for c in cases)
    P = len(cases)
    fe = ssf.Frontend(64, device=dev.index, solver=solver, max_iter=iters)
    frames = [c.curr for c in cases] + [c.last for c in cases]
    bound = bound or max(len(f) for f in frames)
    pb = _batch(dev, frames, bound)
    last, curr = _views(pb, P, dev)
    h = [int(v) for v in pb.h_off]
    total = h[-1]
    nrm = np.zeros((total, 3), np.float32)
    val = np.zeros(total, np.uint8)
    for p, c in enumerate(cases):
        nrm[h[P + p]:h[P + p + 1]] = c.normal
        val[h[P + p]:h[P + p + 1]] = c.valid
    if table_mode == "brute":
        table = ssf.frontend.PlaneTable(torch.from_numpy(nrm).to(dev), torch.from_numpy(val).to(dev), None, None)
    else:
        table = fe.plane_table(pb, strips=table_mode != "own_strips")
        table[0].copy_(torch.from_numpy(nrm).to(dev))
        table[1].copy_(torch.from_numpy(val).to(dev))
    pose = torch.tensor(np.stack([c.pose0 for c in cases]), dtype=torch.float64, device=dev)
    pabs = torch.tensor(np.tile(ABS0, (P, 1)), dtype=torch.float64, device=dev)
    edges = None
    if cases[0].edges is not None:
        eframes = [c.edges[3] for c in cases] + [c.edges[0] for c in cases]
        eb = _batch(dev, eframes, max(len(f) for f in eframes))
        last_e, curr_e = _views(eb, P, dev)
        eh = [int(v) for v in eb.h_off]
        line = np.zeros((eh[-1], 6), np.float32)
        lval = np.zeros(eh[-1], np.uint8)
        for p, c in enumerate(cases):
            line[eh[P + p]:eh[P + p + 1]] = c.edges[1]
            lval[eh[P + p]:eh[P + p + 1]] = c.edges[2]
        edges = (last_e, (torch.from_numpy(line).to(dev), torch.from_numpy(lval).to(dev)), curr_e)
    res = fe.register(last, table, curr, pose, pose_abs=pabs, want_log=True, want_nn=edges is None, edges=edges)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items() if v is not None}
    out["curr_off"] = h[:P + 1]
    out["strip_image"] = getattr(table, "strips", None) is not None
    return out


def _check(case, res, p, capsys, worst):
    y = rc.yardstick(case)
    assert rc.admit(case, y) == [], case.name
    nl = int(res["nlog"][p])
    log, pose = res["log"][p, :nl], res["pose_rel"][p]
    if "nn" in res:
        o = res["curr_off"][p]
        assert np.array_equal(res["nn"][o:o + len(case.curr)], y["nn"]), case.name
    assert int(res["ncorr"][p]) == len(y["po"]), (case.name, int(res["ncorr"][p]), len(y["po"]))
    if case.edges is not None:
        assert int(res["ncorr_edge"][p]) == len(y["edges"][0]), case.name
    # pose_abs: the composition (:87-90) of the start pose with the device's own solution
    qa, ta = ref.compose(ABS0[:4], ABS0[4:], pose[:4], pose[4:])
    assert np.abs(res["pose_abs"][p] - np.r_[qa, ta]).max() < 1e-12, case.name
    if not case.asserted:
        rc.check_unasserted(case, y, log, pose)
        with capsys.disabled():
            print(f"\n  [recorded] {case.name}: device {log[:, 8].astype(int).tolist()} yardstick "
                  f"{y['sol']['log'][:, 8].astype(int).tolist()} dt {np.abs(pose[4:] - y['sol']['t']).max():.3g} "
                  f"dr {ref.quat_angle(pose[:4], y['sol']['q']):.3g}")
        return
    got = rc.compare(case, y, log, pose, rc.TOL_T, rc.TOL_R)
    for k in worst:
        worst[k] = max(worst[k], got[k])
    if nl == len(y["sol"]["log"]) and not case.rank_deficient:        # and against the yardstick's composition
        qy, ty = ref.compose(ABS0[:4], ABS0[4:], y["sol"]["q"], y["sol"]["t"])
        assert np.abs(res["pose_abs"][p, 4:] - ty).max() < rc.TOL_T and \
            ref.quat_angle(res["pose_abs"][p, :4], qy) < rc.TOL_R, case.name
    if case.rank_deficient:
        with capsys.disabled():
            print(f"\n  [recorded] {case.name}: null-space displacement {got['null']:.3g}, statuses {got['statuses']}"
                  f" (yardstick {y['sol']['log'][:, 8].astype(int).tolist()})")


def _run(dev, cases, table_mode, capsys, bound=None, what=""):
    worst = dict(dt=0.0, dr=0.0, dcost=0.0, null=0.0)
    groups = {}
    for c in cases:
        groups.setdefault((c.solver, c.max_iter), []).append(c)
    for group in groups.values():
        res = _launch(dev, group, table_mode, bound)
        for p, c in enumerate(group):
            _check(c, res, p, capsys, worst)
    with capsys.disabled():
        print(f"\n  {what}worst device-to-yardstick gaps: dt {worst['dt']:.3g} m, dr {worst['dr']:.3g} rad, "
              f"cost {worst['dcost']:.3g} rel")


@pytest.mark.parametrize("family", ["status", "quat", "rank", "scale", "norm", "edge"])
def test_solve_families_against_yardstick(dev, family, capsys):
    """every status 0 .. 6, both quaternion-update paths in LM and GN, rank-deficient geometry,
    a scene 5 km out and one below 1 mm, warm starts off the unit sphere, point-to-line blocks
    (k_solve<true>; among them a last edge cloud above k_edge_associate's LDS cap, read from
    global memory, and a two-pair launch whose last pair has an empty last edge cloud):
    brute-force association, one launch per solver and max_iter"""
    cases = [c for c in rc.solve_cases() if c.family == family]
    seen = set()
    for c in cases:
        seen |= set(rc.yardstick(c)["sol"]["log"][:, 8].astype(int).tolist())
    if family == "status":
        assert seen == set(range(7)), seen
    if family == "quat":
        for c in cases:
            assert rc.quat_paths_clear(rc.yardstick(c), c.pose0, "large" in c.name), c.name
    _run(dev, cases, "brute", capsys, what=f"{family}: ")


def res_counts(cases):
    """the valid records the yardstick's association gives each case (the device's ncorr is
    asserted equal to it in _check)"""
    return [len(rc.yardstick(c)["po"]) for c in cases]


@pytest.mark.parametrize("solver", [rc.LM, rc.GN])
def test_counts_solve_side_compaction(dev, solver, capsys):
    """nv valid records on the kernel's edges, all valid and ~50 % masked, through the group-mode
    association and k_solve's own ballot compaction (launches of at most 16 pairs); 4097 valid
    records leave the LDS for the global-memory evaluate"""
    import ssf
    cases = rc.count_cases(solver)
    cap = rc.solve_lds_cap()          # above it k_solve evaluates from global memory
    assert {cap - 1, cap, cap + 1} <= {c.note["nv"] for c in cases} and max(res_counts(cases)) > cap
    bound = max(max(len(c.last), len(c.curr)) for c in cases)
    for lo in range(0, len(cases), 12):
        group = cases[lo:lo + 12]
        plan = ssf.register_plan(len(group), bound)
        assert plan["strip_path"] and plan["group_mode"] and not plan["compacted"], plan
        _run(dev, group, "sorted", capsys, bound, what=f"ballot {lo}: ")


@pytest.mark.parametrize("solver", [rc.LM, rc.GN])
def test_counts_compacted_records(dev, solver, capsys):
    """the same counts through the lane-mode association with one work-group per pair, which hands
    k_solve compacted records: evaluate_load, and above 4096 the global-memory evaluate -- 129
    pairs in one launch (every case three or four times over: the repeats must give the first
    one's bits)"""
    import ssf
    cases = rc.count_cases(solver)
    cap = rc.solve_lds_cap()          # above it k_solve evaluates from global memory
    assert {cap - 1, cap, cap + 1} <= {c.note["nv"] for c in cases} and max(res_counts(cases)) > cap
    P = 129
    tiled = [cases[p % len(cases)] for p in range(P)]
    bound = max(max(len(c.last), len(c.curr)) for c in cases)
    plan = ssf.register_plan(P, bound)
    assert plan["strip_path"] and not plan["group_mode"] and plan["qsplit"] == 1 and plan["compacted"], plan
    res = _launch(dev, tiled, "sorted", bound)
    worst = dict(dt=0.0, dr=0.0, dcost=0.0, null=0.0)
    for p, c in enumerate(tiled):
        if p < len(cases):
            _check(c, res, p, capsys, worst)
        else:
            f = p % len(cases)
            assert int(res["ncorr"][p]) == int(res["ncorr"][f]) and int(res["nlog"][p]) == int(res["nlog"][f]), p
            assert np.array_equal(res["pose_rel"][p].view(np.uint64), res["pose_rel"][f].view(np.uint64)), p
            assert np.array_equal(res["log"][p].view(np.uint64), res["log"][f].view(np.uint64)), p
    with capsys.disabled():
        print(f"\n  compacted: worst device-to-yardstick gaps: dt {worst['dt']:.3g} m, dr {worst['dr']:.3g} rad, "
              f"cost {worst['dcost']:.3g} rel")


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def test_plane_table_against_yardstick(dev):
    """k_plane_table* on the seeded 5-point sets and pick frames: validity as the yardstick's
    (where its own margins are clear), the basic solution's zero pattern on the rank-1 / rank-2
    sets, angle(n_device, n_yardstick) <= FIT_C kappa(A) 2^-24 on full-rank sets (FIT_C: four
    times the worst ratio the CPU oracle showed, tests/test_registration_host.py)."""
    import ssf
    from registration_cases import FIT_C
    fe = ssf.Frontend(64, device=dev.index)
    fe16 = ssf.Frontend(16, device=dev.index)
    fits, picks = rc.fit_frames(), rc.pick_frames()
    for pm, front in ((0.05, fe), (0.15, fe16)):
        sel = [f for f in fits if f[2] == pm] + ([(n, fr, m, "pick") for n, fr, m in picks] if pm == 0.05 else [])
        pb = _batch(dev, [f[1] for f in sel], max(len(f[1]) for f in sel))
        normal, valid, _, _ = front.plane_table(pb)
        torch.cuda.synchronize()
        normal, valid = normal.cpu().numpy(), valid.cpu().numpy()
        h = [int(v) for v in pb.h_off]
        for k, (name, fr, _, kind) in enumerate(sel):
            for a in (range(len(fr)) if kind == "pick" else (0,)):
                pk = ref.plane_pick(fr, a)
                g, v = normal[h[k] + a], bool(valid[h[k] + a])
                if pk["pick"] is None or not pk["d2n"] < 1.0:
                    assert not v and np.all(g == 0), (name, a)
                    continue
                fit = ref.plane_fit5(fr[pk["pick"], :3], pm)
                if kind in ("rank1", "rank2"):
                    assert v == fit["valid"] and np.array_equal(g == 0, fit["x"] == 0), (name, g, fit["x"])
                    assert _angle(g, fit["normal"]) < 1e-6, name
                    continue
                if fit["rank"] < 3 or (kind == "pick" and fit["margin"] <= 1e-4):
                    continue
                assert v == fit["valid"], (name, a, fit["margin"])
                if kind != "pick" or v:
                    assert _angle(g, fit["normal"]) <= FIT_C * fit["kappa"] * 2.0 ** -24, (name, a)

"""The CPU oracle's registration stage (orc_plane_table, orc_correspond, orc_solve2 in both modes,
orc_register_pair, orc_register_pair_edges) against the independent yardstick of
tests/registration_reference.py, on the seeded cases of tests/registration_cases.py.  No GPU.

The oracle restates the kernels line for line, so every GPU test against it shares its mistakes;
the yardstick is built differently (jets, lstsq on the Jacobian, QR as mathematics).  The bars
here are a TENTH of the project's per-step pose bars, so that the device keeps nine tenths of
the room in tests/test_gpu_solve_yardstick.py.
"""
import numpy as np
import pytest

import registration_cases as rc
import registration_reference as ref

HOST_T, HOST_R = rc.TOL_T / 10.0, rc.TOL_R / 10.0
MODE = {rc.LM: 0, rc.GN: 1}
FIT_C = rc.FIT_C


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def _oracle_solve(O, case, y):
    """the oracle's own association and solve of a case (the hand-made table applied to its 1-NN)"""
    q0, t0 = case.pose0[:4], case.pose0[4:]
    nn = O.correspond(case.last, case.curr, q0, t0)
    assert np.array_equal(nn, y["nn"]), case.name
    keep = case.valid[nn] != 0
    po, pa, n = case.curr[keep, :3], case.last[nn[keep], :3], case.normal[nn[keep]]
    if case.edges is None:
        q, t, log = O.solve(po, pa, n, mode=MODE[case.solver], max_iter=case.max_iter, q_init=q0, t_init=t0)
    else:
        last_e, line, lvalid, curr_e = case.edges
        enn = O.correspond(last_e, curr_e, q0, t0)
        ek = enn >= 0                                       # an empty last edge cloud: no neighbour
        ek[ek] = lvalid[enn[ek]] != 0
        q, t, log = O.solve2(po, pa, n, curr_e[ek, :3], line[enn[ek], :3], line[enn[ek], 3:], mode=MODE[case.solver],
                             max_iter=case.max_iter, q_init=q0, t_init=t0)
        assert int(ek.sum()) == len(y["edges"][0]), case.name
    assert int(keep.sum()) == len(y["po"]), case.name
    return log, np.r_[q, t]


def _run_family(O, cases, capsys):
    worst = dict(dt=0.0, dr=0.0, dcost=0.0, null=0.0)
    for case in cases:
        y = rc.yardstick(case)
        assert rc.admit(case, y) == [], case.name
        log, pose = _oracle_solve(O, case, y)
        if not case.asserted:
            rc.check_unasserted(case, y, log, pose)
            with capsys.disabled():
                print(f"\n  [recorded] {case.name}: oracle {log[:, 8].astype(int).tolist()} yardstick "
                      f"{y['sol']['log'][:, 8].astype(int).tolist()} dt {np.abs(pose[4:] - y['sol']['t']).max():.3g} "
                      f"dr {ref.quat_angle(pose[:4], y['sol']['q']):.3g}")
            continue
        got = rc.compare(case, y, log, pose, HOST_T, HOST_R)
        for k in worst:
            worst[k] = max(worst[k], got[k])
        if case.rank_deficient:
            with capsys.disabled():
                print(f"\n  [recorded] {case.name}: null-space displacement {got['null']:.3g}, statuses {got['statuses']}"
                      f" (yardstick {y['sol']['log'][:, 8].astype(int).tolist()})")
    with capsys.disabled():
        print(f"\n  worst oracle-to-yardstick gaps: dt {worst['dt']:.3g} m, dr {worst['dr']:.3g} rad, "
              f"cost {worst['dcost']:.3g} rel")


def test_jet_jacobian_matches_central_differences():
    """the yardstick is not wrong in one place only: its jet Jacobian against central differences
    through Plus (h = 1e-6, agreement 1e-7 of the largest entry), planes, edges, outliers beyond
    the Huber knee and a non-unit quaternion"""
    by = {c.name: c for c in rc.solve_cases()}
    for name in ("clean_lm", "outliers_lm", "knee_lm", "far_a_lm", "edge_both_lm", "edge_only_lm", "norm_p1e3_lm",
                 "par_z_lm", "far5km_lm"):
        case, y = by[name], rc.yardstick(by[name])
        for q, t in ((case.pose0[:4], case.pose0[4:]), (y["sol"]["q"], y["sol"]["t"])):
            # 5 km out the residual's own rounding (2^-53 x 5e3 m) over 2h limits the differences
            bar = 1e-7 if name != "far5km_lm" else 1e-5
            assert ref.jacobian_self_check(y["po"], y["pa"], y["n"], q, t, y["edges"]) < bar, name


def test_cases_cover_what_they_claim():
    """on the yardstick's logs alone: statuses 0 .. 6 each at least once; both quaternion-update
    paths in both solvers (the first step's |d|^2 on the named side of 2^-14, every step clear of it
    by 10x, a small one in every solve); every listed count present, all-valid and masked, with its mask's runs across
    records 63|64, 511|512 and 2047|2048"""
    seen = set()
    for case in rc.solve_cases():
        y = rc.yardstick(case)
        seen |= set(y["sol"]["log"][:, 8].astype(int).tolist())
        if case.family == "quat":
            assert rc.quat_paths_clear(y, case.pose0, "large" in case.name), (case.name, rc.steps_x2(y, case.pose0))
    assert seen == set(range(7)), seen
    for solver in (rc.LM, rc.GN):
        nvs = {}
        for case in rc.count_cases(solver):
            y = rc.yardstick(case)
            assert np.array_equal(y["nn"], np.arange(len(case.curr))), case.name    # record i pairs with point i
            assert int(y["keep"].sum()) == case.note["nv"], case.name
            nvs.setdefault("mask" if "mask" in case.name else "all", []).append(case.note["nv"])
            if "mask" in case.name:
                k = y["keep"]
                assert 0.35 < k.mean() < 0.65 or len(k) < 400, (case.name, k.mean())
                for b in (64, 512, 2048):
                    if len(k) > b + 8:
                        assert k[b - 1] == k[b], (case.name, b)
        assert nvs["all"] == list(rc.COUNTS) and nvs["mask"] == list(rc.COUNTS)


@pytest.mark.parametrize("family", ["status", "quat", "rank", "scale", "norm", "edge"])
def test_oracle_solve_against_yardstick(oracle, family, capsys):
    """orc_correspond + orc_solve2 (LM and GN): the 1-NN indices equal; statuses and log length
    identical; cost within 1e-9 relative; every logged pose and the final one within a tenth of
    the project's bars.  Rank-deficient cases: cost, the pose projected on the row space of J, the
    statuses through the last clear row, 3 or 4 at the end; the null-space displacement is printed."""
    _run_family(oracle, [c for c in rc.solve_cases() if c.family == family], capsys)


@pytest.mark.parametrize("solver", [rc.LM, rc.GN])
def test_oracle_solve_counts_against_yardstick(oracle, solver, capsys):
    _run_family(oracle, rc.count_cases(solver), capsys)


def test_plane_fit_against_yardstick(oracle, capsys):
    """orc_plane_table's fit (qr_solve_5x3, normalize, the dd tests) on the seeded 5-point sets:
    picks and validity identical; on the rank-1 / rank-2 sets the basic solution has the same
    zero pattern; on full-rank sets angle(n_oracle, n_yardstick) <= FIT_C kappa(A) 2^-24."""
    worst = 0.0
    for name, fr, pm, kind in rc.fit_frames():
        pk, fit = rc._fit_of(fr, pm)
        nrm, valid, pick, gate = oracle.plane_table(fr, pm)
        assert np.array_equal(pick[0], pk["pick"]) and gate[0] == pk["n"], name
        assert bool(valid[0]) == fit["valid"], (name, valid[0], fit["margin"])
        if kind in ("rank1", "rank2"):
            assert fit["rank"] == (1 if kind == "rank1" else 2), (name, fit["pivots"])
            assert np.array_equal(nrm[0] == 0, fit["x"] == 0), (name, nrm[0], fit["x"])
            assert _angle(nrm[0], fit["normal"]) < 1e-6, name
        else:
            assert fit["rank"] == 3, name
            ratio = _angle(nrm[0], fit["normal"]) / (fit["kappa"] * 2.0 ** -24)
            worst = max(worst, ratio)
            assert ratio <= FIT_C, (name, ratio)
        if kind == "edge":
            assert fit["valid"] == ("below" in name), name
    with capsys.disabled():
        print(f"\n  worst angle / (kappa 2^-24) over the full-rank sets: {worst:.3g} (FIT_C = {FIT_C})")


def test_plane_pick_against_yardstick(oracle):
    """:173-205 for every point of the pick frames (m = 4 .. 31 points; 0, 1, 2 other-row points
    at ranks 5 .. 29; the gated d2 either side of 1 m^2): the five indices, the gated rank and,
    where the yardstick's own margins are clear, the validity."""
    others = set()
    for name, fr, pm in rc.pick_frames():
        nrm, valid, pick, gate = oracle.plane_table(fr, pm)
        for a in range(len(fr)):
            pk = ref.plane_pick(fr, a)
            if pk["pick"] is None:
                assert not valid[a] and np.all(pick[a] == -1), (name, a)
                continue
            assert min(pk["gap45"], pk["gap_n"]) > 1e-5, (name, a, "a near tie decides the pick")
            assert np.array_equal(pick[a], pk["pick"]) and gate[a] == pk["n"], (name, a, pick[a], pk)
            if name.startswith("other") and a == 0:
                others.add(pk["other"])
            assert pk["gate_gap"] > 1e-5, (name, a)
            if not pk["d2n"] < 1.0:
                assert not valid[a] and np.all(nrm[a] == 0), (name, a)
                continue
            fit = ref.plane_fit5(fr[pk["pick"], :3], pm)
            if fit["margin"] > 1e-4 and fit["rank"] == 3:
                assert bool(valid[a]) == fit["valid"], (name, a)
        if name.startswith("gate"):
            assert ref.plane_pick(fr, 0)["n"] == 5 and bool(valid[0]) == (name == "gate_inside"), name
    assert others == {0, 1, 2}, others


def test_register_pair_composition(oracle):
    """orc_register_pair / orc_register_pair_edges on a frame's OWN plane table (three walls): the
    yardstick's picks, gate and validity for every last-frame point, its 1-NN, and its solve of
    the correspondences under the oracle's normals (the fit itself is bounded in
    test_plane_fit_against_yardstick) give the oracle's count, statuses and poses; with the
    walls' corner lines as edge clouds, orc_edge_table against numpy and the planes + edges solve
    against the yardstick's."""
    last, curr, ws = rc.wall_scene()
    nrm, valid, pick, gate = oracle.plane_table(last, 0.05)
    assert 0.5 < valid.mean() <= 1.0
    for a in range(len(last)):
        pk = ref.plane_pick(last, a)
        assert min(pk["gap45"], pk["gap_n"]) > 1e-5 and pk["gate_gap"] > 1e-5, a
        assert np.array_equal(pick[a], pk["pick"]) and gate[a] == pk["n"], a
        fit = ref.plane_fit5(last[pk["pick"], :3], 0.05)
        if pk["d2n"] < 1.0 and fit["margin"] > 1e-4:
            assert bool(valid[a]) == fit["valid"], a
            if fit["valid"]:
                assert _angle(nrm[a], fit["normal"]) <= FIT_C * fit["kappa"] * 2.0 ** -24, a
    for solver in (rc.LM, rc.GN):
        case = rc.Case(f"walls_{solver}", "walls", last, nrm, valid.astype(np.uint8), curr, ws, solver, rc.ITERS[solver],
                       open_end=True)
        y = rc.yardstick(case)
        assert y["gap"].min() >= 1e-3
        q, t, log, c = oracle.register_pair(last, curr, 0.05, mode=MODE[solver], max_iter=case.max_iter,
                                            q_init=ws[:4], t_init=ws[4:])
        assert c == len(y["po"]) > 100
        rc.compare(case, y, log, np.r_[q, t], HOST_T, HOST_R)
        # and with the corner lines as edge clouds: the oracle's line table against a plain
        # numpy one (5-NN centroid, principal axis of the covariance, largest component positive),
        # then the yardstick's solve of planes + edges on the oracle's table
        last_e, curr_e = rc.wall_edges()
        line, lvalid = oracle.edge_table(last_e)
        assert lvalid.sum() > 90
        X, clear = last_e[:, :3].astype(np.float64), 0
        for a in np.nonzero(lvalid)[0]:
            d2 = ((X - X[a]) ** 2).sum(1)
            nb = X[np.lexsort((np.arange(len(X)), d2))[:5]]
            w, V = np.linalg.eigh(np.cov(nb.T, bias=True))
            u = V[:, 2] * np.sign(V[np.argmax(np.abs(V[:, 2])), 2])
            assert np.abs(line[a, :3] - nb.mean(0)).max() < 1e-5, a
            if w[2] > 10 * w[1]:                                           # off the corners: the axis is well defined
                clear += 1
                assert _angle(line[a, 3:], u) < 1e-5, a
        assert clear > 80
        ecase = rc.Case(f"walls_edges_{solver}", "walls", last, nrm, valid.astype(np.uint8), curr, ws, solver,
                        rc.ITERS[solver], edges=(last_e, line, lvalid.astype(np.uint8), curr_e), open_end=True)
        ye = rc.yardstick(ecase)
        assert rc.admit(ecase, ye) == []
        q2, t2, log2, c2, ce = oracle.register_pair_edges(last, curr, last_e, curr_e, 0.05, mode=MODE[solver],
                                                          max_iter=case.max_iter, q_init=ws[:4], t_init=ws[4:])
        assert c2 == c and ce == len(ye["edges"][0]) > 90, (c2, ce)
        rc.compare(ecase, ye, log2, np.r_[q2, t2], HOST_T, HOST_R)
        assert not np.array_equal(log2[:, :7], log[:, :7])                 # the edge blocks moved the solve

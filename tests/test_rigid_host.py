"""The CPU oracle's 3x3 algebra (orc_svd3, orc_kabsch, orc_quat_from_R, the Umeyama / convergence
block of orc_icp) against tests/rigid_reference.py, the numpy float64 yardstick that shares no
code with it.  No GPU: oracle/ssf_oracle.c and oracle/loop_oracle.c state the same sweep and the
same branch ladder as ssf-slam_amd/csrc/svd3.hpp and the device tails line for line, so a
misreading both sides share shows up here first; tests/test_gpu_rigid_tails.py then holds the
device to the same yardstick.

Bars: R 1e-9, rotation angle of Ra^T Rb 1e-6 rad, t 1e-5 m (those of test_kabsch_golden);
q 2e-9 (in the chosen branch the root's argument is >= 1, so each component is at most two
entries of R times a factor <= 0.5, plus the scale term); ICP as _check_icp of test_gpu_loop.py.
"""
import numpy as np
import pytest

import rigid_cases as RC
import rigid_reference as RR


# --------------------------------------------------------------------------- svd3
def _svd3_inputs():
    rng = np.random.default_rng(42)
    Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    M = {}
    for k in range(4):
        M[f"full{k}"] = rng.standard_normal((3, 3)) * 10.0 ** rng.integers(-3, 4)
    for k in range(3):
        a = rng.standard_normal((3, 2))
        M[f"rank2_{k}"] = a @ rng.standard_normal((2, 3))
    for k in range(3):                                    # rank 1 up to rounding
        M[f"rank1_noise{k}"] = np.outer(rng.standard_normal(3), rng.standard_normal(3))
    for k, (a, b) in enumerate([((1, 1, 0), (-1, 1, 0)), ((1, 0, 0), (1, 0, 0)), ((2, -1, 3), (1, 4, -2)),
                                ((0, 0, 5), (3, 0, 0)), ((1, 2, 2), (1, 2, 2))]):
        M[f"rank1_exact{k}"] = np.outer(np.array(a, float), np.array(b, float))
    M["zero"] = np.zeros((3, 3))
    M["equal_sv"] = 5.0 * Q
    M["diag_tiny"] = np.diag([1.0, 1.0, 1e-13])
    M["coplanar_rows"] = np.array([[3.0, 1, 0], [1, 2, 0], [0, 0, 0]])
    return M


SVD3 = _svd3_inputs()


@pytest.mark.parametrize("name", sorted(SVD3))
def test_svd3_vs_numpy(oracle, name):
    A = SVD3[name]
    U, S, Vt = oracle.svd3(A)
    Sn = np.linalg.svd(A, compute_uv=False)
    scale = max(Sn[0], np.finfo(float).tiny)
    assert np.all(S[:-1] >= S[1:]) and np.all(S >= 0)
    assert np.abs(S - Sn).max() <= 1e-12 * scale, (S, Sn)
    assert np.abs(U @ np.diag(S) @ Vt - A).max() <= 1e-12 * scale
    assert np.abs(U.T @ U - np.eye(3)).max() <= 1e-12, U
    assert np.abs(Vt @ Vt.T - np.eye(3)).max() <= 1e-12, Vt
    if name == "zero":
        assert np.array_equal(U, np.eye(3)) and np.array_equal(Vt, np.eye(3))
    if S[2] <= 1e-12 * S[0]:                 # completed columns: right-handed on both sides
        assert np.linalg.det(U) > 0 and np.linalg.det(Vt) > 0


def test_svd3_every_small_integer_rank1_matrix(oracle):
    """All outer products a b^T / 4 with entries of a, b in -2..3: exactly rank 1.  Where a's
    components have equal magnitudes the sweep leaves no exact zero but a ~1e-157 column parallel
    to u0 (920 of the 46225 gave |U^T U - I| = 1 while svd3 completed U only under sv == 0)."""
    import itertools
    vecs = [np.array(v, float) for v in itertools.product(range(-2, 4), repeat=3) if any(v)]
    worst_u = worst_a = 0.0
    for a in vecs:
        for b in vecs:
            A = np.outer(a, b) * 0.25
            U, S, Vt = oracle.svd3(A)
            worst_u = max(worst_u, np.abs(U.T @ U - np.eye(3)).max(), np.abs(Vt @ Vt.T - np.eye(3)).max())
            worst_a = max(worst_a, np.abs(U @ np.diag(S) @ Vt - A).max() / S[0])
            assert np.linalg.det(U) > 0 and np.linalg.det(Vt) > 0
    assert worst_u <= 1e-12 and worst_a <= 1e-12, (worst_u, worst_a)


# --------------------------------------------------------------------------- Kabsch + quaternion
def test_rotation_set_reaches_the_four_branches():
    """On the yardstick alone: the set takes every branch, each at a margin >= 1e-3."""
    seen = set()
    for name, R in RC.ROTATIONS:
        q, branch, margins = RR.quat_xyzw(R)
        assert min(margins) >= 1e-3, (name, margins)
        assert abs(np.linalg.norm(q) - 1) < 1e-12 and np.abs(RR.rot_from_quat(q) - R).max() < 1e-12
        seen.add(branch)
    assert seen == set(RR.BRANCHES)


FRAMES = RC.kabsch_frames(RC.MASK_POSE_N)


@pytest.mark.parametrize("k", range(len(FRAMES)), ids=[f"{f[0]}-n{f[1]}" for f in FRAMES])
def test_kabsch_and_quaternion_vs_yardstick(oracle, k):
    name, n, Rtrue, src, dst = FRAMES[k]
    Rr, tr, det = RR.kabsch(src, dst, reflection=True)
    if n > 3:                                # three points span a plane: LAPACK's third sign is free
        assert det > 0
    rc, R, t = oracle.kabsch(src, dst)
    assert rc == 0
    assert np.abs(R - Rr).max() < 1e-9 and RR.rot_angle(R, Rr) < 1e-6
    assert np.abs(t - tr).max() < 1e-5
    assert RR.rot_angle(R, Rtrue) < 1e-2    # and it is the rotation that was put in
    qr, branch, margins = RR.quat_xyzw(Rr)
    assert min(margins) >= 1e-3
    qrc, q = oracle.quat_from_R(R)
    assert qrc == 0
    assert np.abs(q - qr).max() < 2e-9, (q, qr)
    assert q["xyzw".index(branch)] > 0
    assert np.abs(RR.rot_from_quat(q) - R).max() < 1e-9


@pytest.mark.parametrize("key", ["all", "mask"])
def test_kabsch_f32_restatement_vs_yardstick(oracle, key):
    """orc_kabsch_f32 (the float32 tail k_kabsch_f32 is compared with) by the float32 rule of
    tests/test_gpu_rigid_tails.py: within 4 e_ref of the float64 yardstick per output, e_ref being
    numpy's own float32 run; rc is 0 or -3 (pyquaternion's atol 1e-8 on a float32 R), and every
    branch keeps rc-0 frames."""
    cases = RC.kabsch_f32_cases()
    err = {k: [0.0, 0.0] for k in "Rtq"}
    ok_branches = set()
    for c in cases:
        r = c["ref"][key]
        rc, R, t, q = oracle.kabsch_f32(c["dst"], c["flow"], None if key == "all" else c["mask"])
        assert rc in (0, -3), (c["name"], rc)
        pairs = [("R", R, r["R"], r["R32"]), ("t", t, r["t"], r["t32"])]
        if rc == 0:
            ok_branches.add(r["branch"])
            pairs.append(("q", q, r["q"], r["q32"]))
        for k, got, r64, r32 in pairs:
            err[k][0] = max(err[k][0], np.abs(r32 - r64).max())
            err[k][1] = max(err[k][1], np.abs(got - r64).max())
    assert ok_branches == set(RR.BRANCHES)
    for k, (e_ref, e_got) in err.items():
        assert e_ref > 0 and e_got <= 4 * e_ref, (k, e_got, e_ref)


def test_kabsch_mask_and_reflection(oracle):
    """mask rows, and a mirrored cloud: rc -2 without the fix, the yardstick's proper R with it."""
    _, _, _, src, dst = FRAMES[5]
    mask = (np.arange(len(src)) % 3 != 1).astype(np.uint8)
    Rr, tr, _ = RR.kabsch(src, dst, mask=mask)
    rc, R, t = oracle.kabsch(src, dst, mask)
    assert rc == 0 and np.abs(R - Rr).max() < 1e-9 and np.abs(t - tr).max() < 1e-5
    mir = dst * [1, 1, -1]
    Rr, tr, det = RR.kabsch(src, mir, reflection=True)
    assert det < 0 and np.linalg.det(Rr) > 0
    assert oracle.kabsch(src, mir)[0] == -2
    rc, R, t = oracle.kabsch(src, mir, reflection=1)
    assert rc == 0 and np.abs(R - Rr).max() < 1e-9 and np.abs(t - tr).max() < 1e-5


def test_kabsch_coplanar_rows(oracle):
    """Exactly coplanar rows (z = 0): H has rank 2, the proper R is unique."""
    rng = np.random.default_rng(3)
    src = np.concatenate([rng.integers(-40, 41, (60, 2)) * 0.25, np.zeros((60, 1))], axis=1)
    Rz = RR.axis_angle([0, 0, 1], 170 * RC.DEG)
    dst = src @ Rz.T + [1.0, 2.0, 0.0]
    dst[:, 2] = 0.0
    Rr, tr, _ = RR.kabsch(src, dst, reflection=True)
    rc, R, t = oracle.kabsch(src, dst)
    assert rc == 0 and np.abs(R - Rr).max() < 1e-9 and np.abs(t - tr).max() < 1e-5
    assert np.linalg.det(R) > 0


RANK_CASES = RC.rank_cases()


@pytest.mark.parametrize("name", sorted(RANK_CASES))
def test_kabsch_rank_deficient(oracle, name):
    """One row / coincident rows (H = 0): R = I, t = md - ms, as numpy gives.  Exactly collinear
    rows (H of rank 1 exactly): a proper rotation that maps the centred source on the centred
    target (the angle about the line is free)."""
    src, dst = RANK_CASES[name]
    rc, R, t = oracle.kabsch(src, dst)
    assert rc == 0
    RC.check_rank_case(name, src, dst, R, t)
    qrc, q = oracle.quat_from_R(R)
    assert qrc == 0
    if name.startswith("zero"):
        Rr, tr, _ = RR.kabsch(src, dst)
        assert np.array_equal(Rr, np.eye(3)) and np.abs(tr - t).max() < 1e-12
        assert np.array_equal(q, [0, 0, 0, 1])


# --------------------------------------------------------------------------- ICP
STEP = RC.icp_step_problems()


def test_icp_step_problems_are_well_posed():
    """On the CPU: every source point's nearest target wins by its problem's gap (any positive
    gap of grid d2 values is >= 1/16), except in the tie rows, which tie exactly; no d2 sits on
    the gate; the mirrored problem takes S(2) = -1; a wrong tie choice moves T by more than the
    bar."""
    for p, r in zip(STEP, RC.icp_step_reference()):
        tr = r["trace"][0]
        gap = tr["d2_second"] - tr["d2"]
        ties = np.zeros(len(gap), bool)
        ties[list(p["ties"])] = True
        assert np.all(gap[~ties] > p["min_gap"]), p["name"]
        assert np.all(gap[ties] == 0), p["name"]
        max_d2 = float(np.float32(p["max_corr_dist"])) ** 2
        assert np.abs(tr["d2"] - max_d2).min() > 1e-3
        assert r["state"] == "iterations" and r["iterations"] == 1
    by = {p["name"]: (p, r) for p, r in zip(STEP, RC.icp_step_reference())}
    p, r = by["gate_ns257_nt2049"]
    assert 3 <= r["n_corr"] < p["src"].shape[0]
    p, r = by["mirror_ns256_nt2048"]
    s, t = p["src"][:, :3].astype(np.float64), p["tgt"][:, :3].astype(np.float64)
    j = RR.nn1(t, s)[0]
    U, _, Vt = np.linalg.svd((t[j] - t[j].mean(0)).T @ (s - s.mean(0)))
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0
    assert np.linalg.det(r["T"][:3, :3].astype(np.float64)) > 0.999
    p, r = by["tie_ns8_nt4100"]
    s, t = p["src"][:, :3].astype(np.float64), p["tgt"][:, :3].astype(np.float64)
    j = RR.nn1(t, s)[0]
    assert j[0] == 2047 and j[1] == 4095
    for wrong in ((2048, 4095), (2047, 4096)):
        jw = j.copy()
        jw[0], jw[1] = wrong
        assert np.abs(RR.umeyama(s, t[jw])[:3, 3] - r["T"][:3, 3]).max() > 100 * 1e-4


@pytest.mark.parametrize("k", range(len(STEP)), ids=[p["name"] for p in STEP])
def test_icp_step_vs_yardstick(oracle, k):
    p, ref = STEP[k], RC.icp_step_reference()[k]
    got = oracle.icp(p["src"], p["tgt"], max_corr_dist=p["max_corr_dist"], max_iter=1, guess=p["guess"])
    assert got["n_corr"] == ref["n_corr"]
    RC.check_icp(got, ref)


OUTCOMES = [(prm, p, b, i) for b, (prm, probs) in enumerate(RC.icp_outcome_batches()) for i, p in enumerate(probs)]


def test_icp_outcomes_reach_every_state():
    states = {RC.icp_outcome_reference()[b][i]["state"] for _, p, b, i in OUTCOMES if p["expect"]}
    assert states == set(RR.ICP_STATES) - {"not_converged"}


@pytest.mark.parametrize("k", range(len(OUTCOMES)), ids=[f"b{o[2]}-{o[1]['name']}" for o in OUTCOMES])
def test_icp_outcome_vs_yardstick(oracle, k):
    prm, p, b, i = OUTCOMES[k]
    ref = RC.icp_outcome_reference()[b][i]
    got = oracle.icp(p["src"], p["tgt"], max_corr_dist=50.0, **prm)
    if p["expect"] is None:
        RC.check_icp_free_rotation(got, ref, p)
        return
    assert ref["state"] == p["expect"]
    RC.check_outcome_margins(ref, prm)
    assert got["n_corr"] == ref["n_corr"]
    RC.check_icp(got, ref, compare_rotation=not p["name"].startswith("collinear"))
    R = got["T"][:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5, R

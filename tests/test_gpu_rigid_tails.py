"""The single-lane tails every published pose ends in -- kabsch_finish of k_mask_pose (f64 and f32
storage), k_kabsch_f32, and the Umeyama / compose / convergence block of k_icp_step with the
2048-point tiles of k_icp_nn -- against tests/rigid_reference.py, the numpy float64 yardstick
(np.linalg.svd, brute-force 1-NN) that tests/test_rigid_host.py also holds the CPU oracle to.

Rotations reach all four branches of the quaternion trace method, each comparison cleared by
>= 1e-3 (tests/rigid_cases.py); point counts sit on the block / chunk / tile edges.

Bars.  f64 tails (f64 and f32 storage, the yardstick fed the same values widened): R 1e-9,
rotation angle 1e-6 rad, t 1e-5 m (test_kabsch_golden's), q 2e-9.  k_kabsch_f32: the float32
rule of tests/test_gpu_sa.py -- with e_ref = max|numpy's float32 run - yardstick| per output
(R, t, q) over the launch, max|device - yardstick| <= 4 e_ref; e_ref never comes from the device
(single special frames ride behind the rotation set, so e_ref is not one draw of numpy's rounding).
ICP: n_corr, state, iteration count and converged equal, T within 1e-5 / 1e-4 m, fitness 1e-6
relative (_check_icp of test_gpu_loop.py).

k_kabsch_f32's status: pyquaternion's orthogonality test (atol 1e-8) on a float32 R sits at the
rounding level, so at large rotations a share of the frames legitimately
report POSE_NOT_ORTHOGONAL, as the reference would raise.  There the status must equal the
oracle's float32 restatement on the same values, q is asserted on the status-0 frames, and every
branch keeps status-0 frames.
"""
import numpy as np
import pytest
import torch

import rigid_cases as RC
import rigid_reference as RR

pytestmark = pytest.mark.gpu
FACTOR = 4.0
T_, Q_, R_, ST_, NBG_ = slice(0, 3), slice(3, 7), slice(7, 16), 16, 17


def _fe(dev):
    import ssf
    return ssf.Frontend(64, device=dev.index or 0)


def _offsets(counts, dev):
    import ssf
    return ssf.frame_offsets(list(counts), dev)


def _cat(arrs, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(np.concatenate(arrs).astype(dtype))).to(dev)


def _mask_pose(fe, dev, pairs, dtype, masks=None, reflection=0):
    """pairs: [(src, dst)] float64.  The kernel takes pos = dst, flow = src - dst in `dtype` and
    forms src = pos + flow in f64.  -> (out [F, 32], [(src, dst)] as the kernel reads them: the
    stored values widened)"""
    pos = [np.asarray(d, np.float64).astype(dtype) for _, d in pairs]
    flow = [(np.asarray(s, np.float64) - np.asarray(d, np.float64)).astype(dtype) for s, d in pairs]
    masks = [np.ones(len(p), np.uint8) for p in pos] if masks is None else masks
    off, h_off = _offsets([len(p) for p in pos], dev)
    out, bg = fe.mask_pose(_cat(pos, dtype, dev), _cat(flow, dtype, dev), off, h_off, mode="given",
                           mask_in=_cat(masks, np.uint8, dev), reflection=reflection)
    torch.cuda.synchronize()
    assert np.array_equal(bg.cpu().numpy(), np.concatenate(masks))
    seen = [(p.astype(np.float64) + f.astype(np.float64), p.astype(np.float64)) for p, f in zip(pos, flow)]
    return out.cpu().numpy(), seen


def _check_f64_tail(o, src, dst, mask=None, tag=""):
    """One frame of a float64 tail against the yardstick on the values the kernel read."""
    Rr, tr, det = RR.kabsch(src, dst, mask=mask, reflection=True)
    qr, branch, margins = RR.quat_xyzw(Rr)
    assert o[ST_] == 0, (tag, o[ST_])
    R = o[R_].reshape(3, 3)
    assert np.abs(R - Rr).max() < 1e-9, (tag, np.abs(R - Rr).max())
    assert RR.rot_angle(R, Rr) < 1e-6, tag
    assert np.abs(o[T_] - tr).max() < 1e-5, (tag, np.abs(o[T_] - tr).max())
    assert np.abs(o[Q_] - qr).max() < 2e-9, (tag, o[Q_], qr)
    assert o[Q_]["xyzw".index(branch)] > 0, tag
    assert np.abs(RR.rot_from_quat(o[Q_]) - R).max() < 1e-9, tag
    assert o[NBG_] == (len(src) if mask is None else int(np.asarray(mask).sum())), tag
    return np.abs(R - Rr).max(), np.abs(o[T_] - tr).max(), np.abs(o[Q_] - qr).max(), branch


FRAMES = RC.kabsch_frames(RC.MASK_POSE_N)


# --------------------------------------------------------------------------- (a), (b)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_mask_pose_tail_rotation_set(dev, dtype):
    """kabsch_finish through fe.mask_pose(mode="given"): every rotation x every point count as
    frames of one batch, in f64 storage and in f32 storage."""
    fe = _fe(dev)
    masks = [RC.chunk_mask(f[1]) for f in FRAMES]
    out, seen = _mask_pose(fe, dev, [(f[3], f[4]) for f in FRAMES], dtype, masks)
    worst = np.zeros(3)
    branches = set()
    for k, (f, (src, dst)) in enumerate(zip(FRAMES, seen)):
        r = _check_f64_tail(out[k], src, dst, masks[k], tag=f"{f[0]}-n{f[1]}")
        worst = np.maximum(worst, r[:3])
        branches.add(r[3])
    print(f"[rigid tails] mask_pose {np.dtype(dtype).name}: max |dR| {worst[0]:.3e} |dt| {worst[1]:.3e} |dq| {worst[2]:.3e}")
    assert branches == set(RR.BRANCHES)


def test_mask_pose_far_from_the_origin(dev):
    """A 40 m cloud 5 km out, f32 storage, 170 deg: the shifted sums k[7..] - n es ed of
    kabsch_finish.  Same bars as the f32-storage batch."""
    fe = _fe(dev)
    _, src, dst = RC.far_frame()
    out, seen = _mask_pose(fe, dev, [(src, dst)], np.float32)
    r = _check_f64_tail(out[0], *seen[0], tag="far")
    print(f"[rigid tails] far origin (5 km, f32 storage): |dR| {r[0]:.3e} |dt| {r[1]:.3e} |dq| {r[2]:.3e}")


# --------------------------------------------------------------------------- (c)
def _kabsch_f32(fe, dev, cases, form, masked, reflection=0):
    off, h_off = _offsets([c["n"] for c in cases], dev)
    kw = dict(src=_cat([c["src"] for c in cases], np.float32, dev)) if form == "src" else \
        dict(flow=_cat([c["flow"] for c in cases], np.float32, dev))
    mask = _cat([c["mask"] for c in cases], np.uint8, dev) if masked else None
    out = fe.kabsch_f32(_cat([c["dst"] for c in cases], np.float32, dev), off, h_off, mask=mask,
                        reflection=reflection, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _e_ref_check(name, dev_vals, ref64, ref32):
    e_ref = max(np.abs(a - b).max() for a, b in zip(ref32, ref64))
    e_dev = max(np.abs(a - b).max() for a, b in zip(dev_vals, ref64))
    print(f"[rigid tails] {name}: e_ref {e_ref:.3e} e_dev {e_dev:.3e} ratio {e_dev / e_ref:.3f}")
    assert e_ref > 0
    assert e_dev <= FACTOR * e_ref, (name, e_dev, e_ref)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask"])
@pytest.mark.parametrize("form", ["src", "flow"])
def test_kabsch_f32_rotation_set(oracle, dev, form, masked):
    """k_kabsch_f32 over the rotation set x point counts up to the 2048-row chunk edge (2047,
    2048, 2049, 4097), src= and flow= forms, without and with a mask that drops rows on both
    sides of the chunk edges."""
    from ssf import _abi
    fe = _fe(dev)
    cases = RC.kabsch_f32_cases()
    out = _kabsch_f32(fe, dev, cases, form, masked)
    key = "mask" if masked else "all"
    refs = [c["ref"][key] for c in cases]
    ok_branches = set()
    for c, r, o in zip(cases, refs, out):
        rc, Ro, to, qo = oracle.kabsch_f32(c["dst"], c["flow"], c["mask"] if masked else None)
        assert o[ST_] == rc and rc in (0, _abi.POSE_NOT_ORTHOGONAL), (c["name"], o[ST_], rc)
        assert o[NBG_] == r["n_bg"], c["name"]
        assert np.array_equal(o[R_], o[R_].astype(np.float32)) and np.array_equal(o[T_], o[T_].astype(np.float32))
        # the oracle restates the same float32 arithmetic (bars of test_asf_f32_kabsch_tail)
        assert np.abs(o[R_].reshape(3, 3) - Ro).max() < 1e-6 and np.abs(o[T_] - to).max() < 1e-6, c["name"]
        assert np.abs(o[Q_] - qo).max() < 1e-6, c["name"]
        assert min(r["margins"]) >= 1e-3
        if rc == 0:
            ok_branches.add(r["branch"])
            assert o[Q_]["xyzw".index(r["branch"])] > 0, c["name"]
        else:
            assert np.array_equal(o[Q_], np.zeros(4)), c["name"]
    assert ok_branches == set(RR.BRANCHES)
    tag = f"kabsch_f32 {form}= {key}"
    _e_ref_check(tag + " R", [o[R_].reshape(3, 3) for o in out], [r["R"] for r in refs], [r["R32"] for r in refs])
    _e_ref_check(tag + " t", [o[T_] for o in out], [r["t"] for r in refs], [r["t32"] for r in refs])
    good = [k for k, o in enumerate(out) if o[ST_] == 0]
    _e_ref_check(tag + " q", [out[k][Q_] for k in good], [refs[k]["q"] for k in good], [refs[k]["q32"] for k in good])


def test_kabsch_f32_src_and_flow_forms_agree(dev):
    """src = f32(dst + flow) handed over as src= reads the same values as flow=: the same bits."""
    fe = _fe(dev)
    cases = RC.kabsch_f32_cases()
    a = _kabsch_f32(fe, dev, cases, "src", True)
    b = _kabsch_f32(fe, dev, cases, "flow", True)
    assert np.array_equal(a[:, :18], b[:, :18])


# --------------------------------------------------------------------------- (d)
def test_python_tail_slove_and_mask_and_pose(dev):
    """ssf.slove_RT_by_SVD and ssf.mask_and_pose (the Python boundary) on a 170 deg frame."""
    import ssf
    name, n, _, src, dst = next(f for f in FRAMES if f[0] == "y170_tilted" and f[1] == 257)
    flow = src - dst
    src_seen = dst + flow                                    # what the f64 kernel forms
    Rr, tr, det = RR.kabsch(src_seen, dst)
    assert det > 0
    qr, branch, _ = RR.quat_xyzw(Rr)
    assert branch == "y"
    R, t = ssf.slove_RT_by_SVD(src, dst, device=dev.index or 0)
    assert R.shape == (3, 3) and t.shape == (3, 1)
    assert np.abs(R - Rr).max() < 1e-9 and RR.rot_angle(R, Rr) < 1e-6 and np.abs(t.ravel() - tr).max() < 1e-5
    res = ssf.mask_and_pose(dst, flow, mode="given", gt_mask=np.ones(n, np.uint8), device=dev.index or 0)
    R1, t1, q1, bg1 = res
    assert np.abs(R1 - Rr).max() < 1e-9 and np.abs(t1.ravel() - tr).max() < 1e-5
    assert np.abs(q1 - qr).max() < 2e-9 and q1[1] > 0
    assert np.abs(res["para_t_q"][0] - np.concatenate([tr, qr])).max() < 1e-5
    assert int(res["info"]["n_bg"][0]) == n and int(bg1.sum()) == n


# --------------------------------------------------------------------------- reflection and rank
def _mirror_pair():
    _, _, _, src, dst = next(f for f in FRAMES if f[0] == "small" and f[1] == 257)
    return src, dst * [1, 1, -1]


def _kabsch_f32_with_set(fe, dev, name, d32, f32, form, reflection):
    """One more frame launched behind the rotation set of test_kabsch_f32_rotation_set, held to the
    float32 rule over that launch (R, t): a single frame's own e_ref is one draw of numpy's
    float32 rounding, the launch's is not.  -> the frame's output row"""
    cases = RC.kabsch_f32_cases()
    extra = dict(n=len(d32), dst=d32, flow=f32, src=d32 + f32, mask=np.ones(len(d32), np.uint8))
    out = _kabsch_f32(fe, dev, cases + [extra], form, False, reflection=reflection)
    Rr, tr, _ = RR.kabsch((d32 + f32).astype(np.float64), d32.astype(np.float64), reflection=True)
    R32, t32, _ = RR.kabsch(d32 + f32, d32, reflection=True, dtype=np.float32)
    refs = [c["ref"]["all"] for c in cases]
    o = out[-1]
    print(f"[rigid tails] kabsch_f32 {form}= {name} alone: |dR| {np.abs(o[R_].reshape(3, 3) - Rr).max():.3e} "
          f"(numpy f32 {np.abs(R32 - Rr).max():.3e}) |dt| {np.abs(o[T_] - tr).max():.3e} (numpy f32 {np.abs(t32 - tr).max():.3e})")
    _e_ref_check(f"kabsch_f32 {form}= set + {name} R", [x[R_].reshape(3, 3) for x in out],
                 [r["R"] for r in refs] + [Rr], [r["R32"] for r in refs] + [R32.astype(np.float64)])
    _e_ref_check(f"kabsch_f32 {form}= set + {name} t", [x[T_] for x in out],
                 [r["t"] for r in refs] + [tr], [r["t32"] for r in refs] + [t32.astype(np.float64)])
    return o


def test_reflection_in_both_kernels(oracle, dev):
    """A mirrored cloud: POSE_REFLECTION; with reflection=1 the yardstick's proper rotation."""
    from ssf import _abi
    fe = _fe(dev)
    src, mir = _mirror_pair()
    for dtype in (np.float64, np.float32):
        out, seen = _mask_pose(fe, dev, [(src, mir)], dtype)
        assert out[0, ST_] == _abi.POSE_REFLECTION
        assert RR.kabsch(*seen[0])[2] < 0
        out, seen = _mask_pose(fe, dev, [(src, mir)], dtype, reflection=1)
        _check_f64_tail(out[0], *seen[0], tag="mirror")
        assert np.linalg.det(out[0, R_].reshape(3, 3)) > 0
    d32 = mir.astype(np.float32)
    f32 = (src - mir).astype(np.float32)
    case = [dict(n=len(d32), dst=d32, flow=f32, src=d32 + f32, mask=np.ones(len(d32), np.uint8))]
    assert RR.kabsch((d32 + f32).astype(np.float64), d32.astype(np.float64))[2] < 0
    rc, Ro, to, qo = oracle.kabsch_f32(d32, f32, None, reflection=1)
    for form in ("src", "flow"):
        assert _kabsch_f32(fe, dev, case, form, False)[0, ST_] == _abi.POSE_REFLECTION
        o = _kabsch_f32_with_set(fe, dev, "mirror", d32, f32, form, 1)
        assert o[ST_] == rc and rc in (0, _abi.POSE_NOT_ORTHOGONAL)
        assert np.linalg.det(o[R_].reshape(3, 3)) > 0
        assert np.abs(o[R_].reshape(3, 3) - Ro).max() < 1e-6 and np.abs(o[T_] - to).max() < 1e-6
        assert np.abs(o[Q_] - qo).max() < 1e-6


def test_coplanar_rows_in_both_kernels(oracle, dev):
    """Exactly coplanar rows (z = 0): H has rank 2 and the proper R is unique -- the yardstick's."""
    from ssf import _abi
    fe = _fe(dev)
    rng = np.random.default_rng(3)
    src = np.concatenate([rng.integers(-40, 41, (60, 2)) * 0.25, np.zeros((60, 1))], axis=1)
    dst = src @ RR.axis_angle([0, 0, 1], 170 * RC.DEG).T + [1.0, 2.0, 0.0]
    dst[:, 2] = 0.0
    for dtype in (np.float64, np.float32):
        out, seen = _mask_pose(fe, dev, [(src, dst)], dtype)
        assert np.all(seen[0][0][:, 2] == 0) and np.all(seen[0][1][:, 2] == 0)
        _check_f64_tail(out[0], *seen[0], tag="coplanar")
        assert np.linalg.det(out[0, R_].reshape(3, 3)) > 0
    d32 = dst.astype(np.float32)
    f32 = (src - dst).astype(np.float32)
    rc, Ro, to, qo = oracle.kabsch_f32(d32, f32, None)
    o = _kabsch_f32_with_set(fe, dev, "coplanar", d32, f32, "flow", 0)
    assert o[ST_] == rc and rc in (0, _abi.POSE_NOT_ORTHOGONAL)
    assert np.linalg.det(o[R_].reshape(3, 3)) > 0
    assert np.abs(o[R_].reshape(3, 3) - Ro).max() < 1e-6 and np.abs(o[T_] - to).max() < 1e-6
    assert np.abs(o[Q_] - qo).max() < 1e-6


def test_rank_deficient_rows_in_both_kernels(oracle, dev):
    """One row / coincident rows (H = 0): status 0, R = I, t = md - ms, q = (0, 0, 0, 1), as numpy
    gives.  Exactly collinear rows (H of rank 1 exactly): status 0 and a proper rotation that
    carries the centred source onto the centred target.  f64 tails to 1e-9; k_kabsch_f32 returns
    float32 values, each entry of R rounded by <= 2^-24, so R R^T - I and the residuals are held
    to 6 * 2^-24 < 4e-7 there.  (Before svd3 completed U for an exactly zero singular value these
    were POSE_NOT_ORTHOGONAL: a zero column in U.)"""
    fe = _fe(dev)
    cases = RC.rank_cases()
    names = sorted(cases)
    for dtype in (np.float64, np.float32):
        out, seen = _mask_pose(fe, dev, [cases[k] for k in names], dtype)
        for k, name in enumerate(names):
            o = out[k]
            assert o[ST_] == 0, (name, o[ST_])
            assert np.array_equal(seen[k][0], cases[name][0]) and np.array_equal(seen[k][1], cases[name][1])
            RC.check_rank_case(name, *cases[name], o[R_].reshape(3, 3), o[T_])
            assert np.abs(RR.rot_from_quat(o[Q_]) - o[R_].reshape(3, 3)).max() < 1e-9, name
            assert o[NBG_] == len(cases[name][0])
            if name.startswith("zero"):
                assert np.array_equal(o[Q_], [0, 0, 0, 1]), (name, o[Q_])
    f32c = []
    for name in names:
        s, d = cases[name]
        d32, fl = d.astype(np.float32), (s - d).astype(np.float32)
        assert np.array_equal((d32 + fl).astype(np.float64), s)          # exact in float32
        f32c.append(dict(n=len(d), dst=d32, flow=fl, src=d32 + fl, mask=np.ones(len(d), np.uint8)))
    for form in ("src", "flow"):
        out = _kabsch_f32(fe, dev, f32c, form, False)
        for k, name in enumerate(names):
            o = out[k]
            assert o[ST_] == 0, (name, form, o[ST_])
            RC.check_rank_case(name, *cases[name], o[R_].reshape(3, 3), o[T_], tol=4e-7)
            assert np.abs(RR.rot_from_quat(o[Q_]) - o[R_].reshape(3, 3)).max() < 4e-7, name
            if name.startswith("zero"):
                assert np.array_equal(o[Q_], [0, 0, 0, 1]), (name, o[Q_])


# --------------------------------------------------------------------------- ICP
def _icp_batch(fe, dev, probs, **prm):
    import ssf
    from ssf import loop
    s = _cat([p["src"] for p in probs], np.float32, dev)
    t = _cat([p["tgt"] for p in probs], np.float32, dev)
    so, hso = ssf.frame_offsets([p["src"].shape[0] for p in probs], dev)
    to, hto = ssf.frame_offsets([p["tgt"].shape[0] for p in probs], dev)
    guess = np.stack([p.get("guess", np.eye(4, dtype=np.float32)) for p in probs])
    return loop.icp_batch(fe, s, so, hso, t, to, hto, loop.icp_params(**prm), guess)


def test_icp_one_step(dev):
    """One k_icp_nn + k_icp_step round (max_iter = 1) per problem, all problems of one gate in
    one launch: source counts around the 256-thread 1-NN block and the 1024-thread step block,
    target counts around the 2048-point tile, 5 deg and a 170 deg guess, a mirrored target
    (S(2) = -1), a coplanar target, exact ties across the tile edge and a gate between two exact
    d2 values.  (tests/test_rigid_host.py checks on the CPU that the problems are well posed.)"""
    fe = _fe(dev)
    probs, refs = RC.icp_step_problems(), RC.icp_step_reference()
    for gate in sorted({p["max_corr_dist"] for p in probs}):
        sel = [k for k, p in enumerate(probs) if p["max_corr_dist"] == gate]
        got = _icp_batch(fe, dev, [probs[k] for k in sel], max_iter=1, max_corr_dist=gate)
        for g, k in zip(got, sel):
            ref = refs[k]
            tr = ref["trace"][0]
            ties = np.zeros(len(tr["d2"]), bool)
            ties[list(probs[k]["ties"])] = True
            assert np.all((tr["d2_second"] - tr["d2"])[~ties] > probs[k]["min_gap"])
            assert ref["state"] == "iterations"
            assert g["n_corr"] == ref["n_corr"], (probs[k]["name"], g["n_corr"], ref["n_corr"])
            try:
                RC.check_icp(g, ref)
            except AssertionError as e:
                raise AssertionError(f"{probs[k]['name']}: {e}") from None


def test_icp_every_outcome(oracle, dev):
    """Every entry of _abi.ICP_STATES reached on purpose, an early finisher beside a problem
    that runs on in every launch (the `done` skip of k_icp_nn and k_icp_step).  ssf_icp_batch
    takes one parameter set per launch, so the cases are three small launches.  Every decision the
    yardstick took clears its threshold by a factor of 10 (RC.check_outcome_margins), so state,
    iterations and converged must equal the yardstick's and the oracle's."""
    from ssf import _abi
    fe = _fe(dev)
    reached = set()
    for (prm, probs), refs in zip(RC.icp_outcome_batches(), RC.icp_outcome_reference()):
        got = _icp_batch(fe, dev, probs, max_corr_dist=50.0, **prm)
        assert len({r["iterations"] for r in refs}) > 1          # early and late in one launch
        for p, g, ref in zip(probs, got, refs):
            orc = oracle.icp(p["src"], p["tgt"], max_corr_dist=50.0, **prm)
            R = g["T"][:3, :3].astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5, (p["name"], R)
            if p["expect"] is None:
                RC.check_icp_free_rotation(g, ref, p)
                RC.check_icp_free_rotation(g, orc, p)
                continue
            assert ref["state"] == p["expect"]
            RC.check_outcome_margins(ref, prm)
            try:
                assert g["n_corr"] == ref["n_corr"] == orc["n_corr"]
                RC.check_icp(g, ref, compare_rotation=not p["name"].startswith("collinear"))
                RC.check_icp(g, orc, compare_rotation=not p["name"].startswith("collinear"))
                assert np.abs(RC._apply(g["T"], p["src"]) - RC._apply(ref["T"], p["src"])).max() < 1e-4
            except AssertionError as e:
                raise AssertionError(f"{p['name']}: {e}") from None
            reached.add(g["state"])
    assert reached == set(_abi.ICP_STATES.values()) - {"not_converged"}

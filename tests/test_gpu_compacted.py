"""The compacted-record registration path that big launches take: the lane-mode
association with ONE work-group per pair writes the valid correspondences compacted in rank order
(`nnv`, the ballot / rank pass, `ncompact`), and k_solve streams them into LDS inside its first
evaluation (`evaluate_load`), or evaluates them from global memory above 4096 records.

Every test proves by ssf.register_plan that its launch took that path (lane mode, qsplit == 1,
compacted) and that its reference launch did not: a single-pair launch is the group-mode
association with the solve-side ballot compaction.  Both feed the evaluations the same records in
the same order, so poses, logs and counts are compared bit for bit; where the order of the f64
sums differs (more than 4096 records: evaluate() from global memory assigns records to threads
by position) the bar is the CPU oracle, within the project's per-step pose bars.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import frame

pytestmark = pytest.mark.gpu

TOL_T = 1e-5   # m   (BASELINE north_star)
TOL_R = 1e-6   # rad
MODE = {"ceres_lm": 0, "gn": 1}


def _quat_angle(q1, q2):
    d = abs(float(np.dot(q1 / np.linalg.norm(q1), q2 / np.linalg.norm(q2))))
    return 2.0 * np.arccos(min(1.0, d))


@functools.lru_cache(maxsize=None)
def _frames(n_az, n=7):
    """Plane clouds of frames 0 .. n-1 of sequence 3 (device tensors) and the extraction's bound
    on plane points per frame."""
    import ssf
    dev = torch.device("cuda", 0)
    fe = ssf.Frontend(64, device=0)
    clouds = [frame(3, k, n_az=n_az)[0] for k in range(n)]
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    off, h_off = ssf.frame_offsets([c.shape[0] for c in clouds], dev)
    pb = fe.extract_planes_batch(pts, off, h_off)
    torch.cuda.synchronize()
    return tuple(pb.frame(k).clone() for k in range(n)), int(pb.max_points)


@functools.lru_cache(maxsize=None)
def _planes1875(seed):
    from oracle import oracle as O
    return O.extract_planes(frame(seed, 0, n_az=1875)[0], 64)


def _tile(dev, frames, slots, bound):
    """One PlaneBatch of len(slots) frame slots, slot s holding a copy of frames[slots[s]]."""
    import ssf
    xyzi = torch.cat([frames[k] for k in slots]).contiguous()
    counts = [int(frames[k].shape[0]) for k in slots]
    off, h_off = ssf.frame_offsets(counts, dev)
    return ssf.PlaneBatch(xyzi, torch.tensor(counts, dtype=torch.int32, device=dev), off, h_off, bound)


def _pairs(pb, spec, dev):
    """spec: per pair (last slot, current slot, last-count cap or None, current-count cap or None)
    -> the (last, current) PlaneBatch views of the shared buffer."""
    import ssf
    h = [int(v) for v in pb.h_off]
    cap = lambda s, c: h[s + 1] - h[s] if c is None else min(h[s + 1] - h[s], c)  # noqa: E731

    def view(slots, caps):
        o = [h[s] for s in slots] + [max(h[s + 1] for s in slots)]
        return ssf.PlaneBatch(pb.xyzi, torch.tensor([cap(s, c) for s, c in zip(slots, caps)],
                                                    dtype=torch.int32, device=dev),
                              torch.tensor(o, dtype=torch.int64, device=dev),
                              torch.tensor(o, dtype=torch.int64), pb.max_points)
    return (view([s[0] for s in spec], [s[2] for s in spec]),
            view([s[1] for s in spec], [s[3] for s in spec]))


def _run(fe, pb, table, spec, init, dev):
    last, curr = _pairs(pb, spec, dev)
    res = fe.register(last, table, curr, init.clone(), want_log=True, want_nn=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if v is not None}


def _curr_slice(pb, s):
    """a pair's queries in the nn array: its current frame's slot, cut to its count"""
    o = int(pb.h_off[s[1]])
    m = int(pb.h_off[s[1] + 1]) - o
    return slice(o, o + (m if s[3] is None else min(m, s[3])))


def _assert_compacted_launch(P, mx):
    import ssf
    p = ssf.register_plan(P, mx)
    assert p["strip_path"] and not p["group_mode"] and p["qsplit"] == 1 and p["compacted"], (P, mx, p)
    return p


def _assert_reference_launch(mx):
    import ssf
    p = ssf.register_plan(1, mx)
    assert p["strip_path"] and p["group_mode"] and not p["compacted"], (mx, p)


def _assert_same_bits(pb, big, p, one, s):
    """pair p of the big launch against its own single-pair launch: count, pose, log, 1-NN"""
    assert int(one["ncorr"][0]) == int(big["ncorr"][p]), (p, int(one["ncorr"][0]), int(big["ncorr"][p]))
    assert np.array_equal(one["pose_rel"][0].view(np.uint64), big["pose_rel"][p].view(np.uint64)), p
    n = int(one["nlog"][0])
    assert n == int(big["nlog"][p]), p
    assert np.array_equal(one["log"][0, :n].view(np.uint64), big["log"][p, :n].view(np.uint64)), p
    sl = _curr_slice(pb, s)
    assert np.array_equal(one["nn"][sl], big["nn"][sl]), p


def _assert_oracle(oracle, pb, res, p, s, pose0, solver, iters):
    """pair p against the CPU oracle: 1-NN exact, count equal, per-step poses within the bars"""
    h = [int(v) for v in pb.h_off]
    L = pb.xyzi[h[s[0]]:h[s[0] + 1]].cpu().numpy()
    sl = _curr_slice(pb, s)
    Cc = pb.xyzi[sl].cpu().numpy()
    q0, t0 = pose0[:4], pose0[4:]
    assert np.array_equal(res["nn"][sl], oracle.correspond(L, Cc, q0, t0)), p
    q, t, log, c = oracle.register_pair(L, Cc, 0.05, mode=MODE[solver], max_iter=iters, q_init=q0, t_init=t0)
    assert int(res["ncorr"][p]) == c, (p, int(res["ncorr"][p]), c)
    nl = int(res["nlog"][p])
    assert nl == log.shape[0], (p, nl, log[:, 8])
    glog = res["log"][p, :nl]
    for k in range(nl):
        assert glog[k, 8] == log[k, 8], (p, k, "status differs")
        assert np.abs(glog[k, 4:7] - log[k, 4:7]).max() < TOL_T, (p, k)
        assert _quat_angle(glog[k, :4], log[k, :4]) < TOL_R, (p, k)
    got = res["pose_rel"][p]
    assert np.abs(got[4:] - t).max() < TOL_T and _quat_angle(got[:4], q) < TOL_R, p
    return log, c


def _warm_starts(P, seed):
    """every pair its own warm start: yaw +-0.003 rad, t_x in 0.6 .. 1.1 m"""
    rng = np.random.default_rng(seed)
    q0 = np.zeros((P, 4)); q0[:, 2] = rng.uniform(-0.003, 0.003, P); q0[:, 3] = 1.0
    q0 /= np.linalg.norm(q0, axis=1, keepdims=True)
    t0 = np.c_[rng.uniform(0.6, 1.1, P), rng.uniform(-0.05, 0.05, P), np.zeros(P)]
    return np.c_[q0, t0]


def _sequence_layout(P, n_last=6):
    """Slots 0 .. P-1: pair p's own current frame (its records live at that offset; pair 0's at
    offset 0), frame 1 + p % n_last of the sequence; slots P .. P+n_last-1: the last frames
    0 .. n_last-1.  Pair p registers frame 1 + p % n_last against frame p % n_last."""
    slots = [1 + p % n_last for p in range(P)] + list(range(n_last))
    spec = [(P + p % n_last, p, None, None) for p in range(P)]
    return slots, spec


def _same_bits_case(oracle, dev, solver, iters, P, n_az):
    import ssf
    fe = ssf.Frontend(64, device=dev.index, solver=solver, max_iter=iters)
    frames, bound = _frames(n_az)
    slots, spec = _sequence_layout(P)
    pb = _tile(dev, frames, slots, bound)
    _assert_compacted_launch(P, bound)
    _assert_reference_launch(bound)
    table = fe.plane_table(pb)
    ws = _warm_starts(P, 11)
    init = torch.tensor(ws, dtype=torch.float64, device=dev)
    big = _run(fe, pb, table, spec, init, dev)
    for p in range(P):
        one = _run(fe, pb, table, [spec[p]], init[p:p + 1], dev)
        assert int(one["ncorr"][0]) > 0, p
        _assert_same_bits(pb, big, p, one, spec[p])
    for p in range(6):                       # the distinct underlying (last, current) pairs
        _assert_oracle(oracle, pb, big, p, spec[p], ws[p], solver, iters)


@pytest.mark.parametrize("solver,iters", [("gn", 10), ("ceres_lm", 8)])
def test_compacted_same_bits_as_single_pair(oracle, dev, solver, iters):
    """130 pairs of ~1500-point frames (two rank trips of 1024) in one launch: the association
    compacts the records, the solve streams them in.  Every pair's pose, log rows, count and
    1-NN indices are bit-identical to its own single-pair launch (group-mode association,
    solve-side compaction) -- DESIGN §6.5's claim -- and the six distinct underlying pairs match
    the CPU oracle: 1-NN exact, count equal, per-step poses within the bars, same statuses."""
    frames, _ = _frames(900)
    assert all(1024 < f.shape[0] <= 2048 for f in frames), [f.shape[0] for f in frames]
    _same_bits_case(oracle, dev, solver, iters, 130, 900)


def test_compacted_small_frames_17_pairs(oracle, dev):
    """17 pairs of ~400-point frames: the plane bound (986) is within one rank trip, so the lane
    mode keeps one work-group per pair below 129 pairs and compacts; a single partial trip."""
    frames, bound = _frames(360)
    assert bound <= 1024 and all(0 < f.shape[0] < 1024 for f in frames), bound
    for solver, iters in (("gn", 10), ("ceres_lm", 8)):
        _same_bits_case(oracle, dev, solver, iters, 17, 360)


def test_compacted_rank_trip_edges(dev):
    """Current-frame counts at the edges of the rank pass: 1, a wave -1 / +0 / +1 (63, 64, 65), a
    trip of 1024 -1 / +0 / +1, and a ~3.6 k-point current frame cut to two trips (2048), two
    trips and one query (2049) and whole (four trips) -- inside one compacted launch of 130
    pairs, each pair bit-identical to its own single-pair launch."""
    import ssf
    P = 130
    fe = ssf.Frontend(64, device=dev.index, solver="gn", max_iter=10)
    f900, b900 = _frames(900)
    f1875, b1875 = _frames(1875, 2)
    assert all(f.shape[0] > 3072 for f in f1875), [f.shape[0] for f in f1875]
    frames, bound = list(f900) + list(f1875), max(b900, b1875)
    slots, spec = _sequence_layout(P)
    cuts = {5: 1, 17: 63, 29: 64, 43: 65, 55: 1023, 67: 1024, 79: 1025}
    for p, c in cuts.items():
        assert frames[slots[p]].shape[0] > c
        spec[p] = (spec[p][0], p, None, c)
    slots.append(7)                                           # slot P + 6: the big last frame
    for p, c in ((40, 2048), (41, 2049), (42, None)):         # big current frames
        slots[p] = 8
        spec[p] = (P + 6, p, None, c)
    pb = _tile(dev, frames, slots, bound)
    _assert_compacted_launch(P, bound)
    _assert_reference_launch(bound)
    table = fe.plane_table(pb)
    init = torch.tensor(_warm_starts(P, 13), dtype=torch.float64, device=dev)
    big = _run(fe, pb, table, spec, init, dev)
    for p in range(P):
        one = _run(fe, pb, table, [spec[p]], init[p:p + 1], dev)
        _assert_same_bits(pb, big, p, one, spec[p])
    for p, c in cuts.items():
        assert 0 <= int(big["ncorr"][p]) <= c, (p, int(big["ncorr"][p]))
    assert int(big["ncorr"][42]) > 1024


@pytest.mark.parametrize("solver,iters", [("gn", 10), ("ceres_lm", 8)])
def test_compacted_edge_pairs(oracle, dev, solver, iters):
    """The pairs that leave the compacted path early, inside a compacted launch of 130 pairs and
    each once as pair 0 (records at offset 0 of the scratch): a last frame of 8 and of 10 plane
    points (skipped, :158: count -1, the warm start unchanged), an empty current frame (count 0;
    also as the launch's final pair), a 3-point current frame, and a last frame with no valid
    plane (16 collinear points 5 m apart: count 0, the oracle's steps -- one invalid step for GN,
    six for LM).  Every pair bit-identical to its own single-pair launch."""
    import ssf
    P = 130
    fe = ssf.Frontend(64, device=dev.index, solver=solver, max_iter=iters)
    f900, bound = _frames(900)
    k = np.arange(16, dtype=np.float64)
    line = np.stack([10.0 + 5.0 * k, 0.0 * k, 0.0 * k, k + 0.01 * k], 1).astype(np.float32)
    assert int(oracle.plane_table(line, 0.05)[1].sum()) == 0
    frames = list(f900) + [torch.from_numpy(line).to(dev)]
    slots, spec = _sequence_layout(P)
    slots.append(7)                                           # slot P + 6: the collinear last frame
    pb = _tile(dev, frames, slots, bound)
    _assert_compacted_launch(P, bound)
    _assert_reference_launch(bound)
    table = fe.plane_table(pb)
    ws = _warm_starts(P, 17)
    init = torch.tensor(ws, dtype=torch.float64, device=dev)
    cases = {"last8": lambda s: (s[0], s[1], 8, None), "last10": lambda s: (s[0], s[1], 10, None),
             "empty": lambda s: (s[0], s[1], None, 0), "three": lambda s: (s[0], s[1], None, 3),
             "noplane": lambda s: (P + 6, s[1], None, None)}
    placed = {0: "last8", 7: "last8", 23: "last10", 38: "empty", 64: "three", 77: "noplane", 129: "empty"}

    def check(spec_v, big, p, name):
        nc = int(big["ncorr"][p])
        if name in ("last8", "last10"):
            assert nc == -1 and np.array_equal(big["pose_rel"][p].view(np.uint64), ws[p].view(np.uint64)), (p, nc)
        elif name == "empty":
            assert nc == 0, (p, nc)
        elif name == "three":
            assert 0 <= nc <= 3, (p, nc)
        else:
            h = [int(v) for v in pb.h_off]
            Cc = pb.xyzi[h[p]:h[p + 1]].cpu().numpy()
            _, _, log, c = oracle.register_pair(line, Cc, 0.05, mode=MODE[solver], max_iter=iters,
                                                q_init=ws[p, :4], t_init=ws[p, 4:])
            assert c == 0 and log.shape[0] == (1 if solver == "gn" else 6) and np.all(log[:, 8] == 2)
            nl = int(big["nlog"][p])
            assert nc == 0 and nl == log.shape[0], (p, nc, nl)
            assert np.array_equal(big["log"][p, :nl, 8], log[:, 8]), (p, big["log"][p, :nl, 8])

    for first in cases:                       # each case once as pair 0
        at = dict(placed)
        at[0] = first
        spec_v = [cases[at[p]](s) if p in at else s for p, s in enumerate(spec)]
        big = _run(fe, pb, table, spec_v, init, dev)
        for p in (range(P) if first == "last8" else (0, 1, 2)):
            one = _run(fe, pb, table, [spec_v[p]], init[p:p + 1], dev)
            _assert_same_bits(pb, big, p, one, spec_v[p])
        for p, name in at.items():
            check(spec_v, big, p, name)


def test_compacted_nan_warm_start(dev):
    """NaN warm starts in a compacted launch: every query is NaN, no candidate wins, and the
    compacted branch falls back to the last frame's first staged point (bc = -1 -> bp = 0) -- an
    index inside the frame, the same as the single-pair (group mode) launch gives."""
    import ssf
    P = 130
    fe = ssf.Frontend(64, device=dev.index)
    frames, bound = _frames(900)
    slots, spec = _sequence_layout(P)
    pb = _tile(dev, frames, slots, bound)
    _assert_compacted_launch(P, bound)
    _assert_reference_launch(bound)
    table = fe.plane_table(pb)
    init = torch.full((P, 7), float("nan"), dtype=torch.float64, device=dev)
    big = _run(fe, pb, table, spec, init, dev)
    for p in range(P):
        sl = _curr_slice(pb, spec[p])
        m_last = frames[slots[spec[p][0]]].shape[0]
        nn = big["nn"][sl]
        assert nn.size > 0 and np.all(nn == nn[0]) and 0 <= nn[0] < m_last, (p, np.unique(nn), m_last)
        one = _run(fe, pb, table, [spec[p]], init[p:p + 1], dev)
        assert np.array_equal(one["nn"][sl], nn), p


def _big_pair_case(oracle, dev, L, Cc, pose0, mx):
    """129 pairs: pair 64 registers Cc against L, the others are ~400-point frames of a sequence.
    Returns what the tests of launches with one big pair need."""
    import ssf
    P, BIG = 129, 64
    fe = ssf.Frontend(64, device=dev.index, solver="gn", max_iter=10)
    small, bound = _frames(360)
    assert bound <= mx and len(L) <= mx and len(Cc) <= mx
    frames = list(small) + [torch.from_numpy(Cc.astype(np.float32)).to(dev),
                            torch.from_numpy(L.astype(np.float32)).to(dev)]
    slots, spec = _sequence_layout(P)
    slots[BIG] = 7
    slots.append(8)                                           # slot P + 6: the big last frame
    spec[BIG] = (P + 6, BIG, None, None)
    pb = _tile(dev, frames, slots, mx)
    plan = _assert_compacted_launch(P, mx)
    _assert_reference_launch(mx)
    table = fe.plane_table(pb)
    ws = _warm_starts(P, 19)
    ws[BIG] = pose0
    init = torch.tensor(ws, dtype=torch.float64, device=dev)
    big = _run(fe, pb, table, spec, init, dev)
    _assert_oracle(oracle, pb, big, BIG, spec[BIG], ws[BIG], "gn", 10)
    return fe, pb, table, spec, init, big, plan, BIG


@pytest.mark.parametrize("staging", ["float4", "soa"])
def test_compacted_beyond_solve_lds(oracle, dev, staging):
    """One pair of a compacted launch with more than 4096 valid correspondences: the solve
    evaluates the compacted records [0, ncompact) from global memory.  That evaluation assigns
    records to threads by position and the compacted order is not the query order, so its f64
    sums differ in order from the single-pair launch's: the bar is the CPU oracle (1-NN exact,
    count equal, per-step poses within the bars, same statuses).  float4: a 6144-point frame
    against itself (4392 valid); soa: 11009 current points (above the 10752 staged) against a
    7311-point last frame (7722 valid)."""
    base = [_planes1875(s) for s in range(4)]
    if staging == "float4":
        L = Cc = np.concatenate(base[:2])[:6144]
        mx = 6144
    else:
        L, Cc = np.concatenate(base[:2]), np.concatenate(base[1:4])
        mx = len(Cc)
        assert len(L) < 10752 < mx <= 16384, (len(L), mx)
    pose0 = np.array([0.0, 0.0, 0.0, 1.0, 0.3, 0.0, 0.0])
    fe, pb, table, spec, init, big, plan, BIG = _big_pair_case(oracle, dev, L, Cc, pose0, mx)
    assert plan["soa"] == (staging == "soa") and len(L) <= plan["lds_cap"], plan
    assert int(big["ncorr"][BIG]) > 4096
    assert np.all(big["log"][BIG, :int(big["nlog"][BIG]), 8] == 6)
    for p in range(12):                       # the small pairs beside it: still their own bits
        one = _run(fe, pb, table, [spec[p]], init[p:p + 1], dev)
        _assert_same_bits(pb, big, p, one, spec[p])


def test_compacted_launch_with_unstaged_last_frame(oracle, dev):
    """One pair whose last frame is above the launch's staging capacity (10752 < m <= 16384, with
    exact duplicates: ties resolve to the lower original index) inside a launch whose other pairs
    are compacted: that pair walks the sorted last frame in global memory, writes its records in
    query order (ncompact = -1) and the solve compacts them itself.  It matches the CPU oracle;
    the small pairs stay bit-identical to their single-pair launches."""
    rng = np.random.default_rng(11 + 4)
    base = [_planes1875(s) for s in range(5)]
    L = np.concatenate(base[:4])
    L = np.concatenate([L, L[rng.choice(len(L), 300, replace=False)]])
    L = L[rng.permutation(len(L))]
    Cc = np.concatenate(base[1:])
    assert 10752 < len(L) <= 16384 and len(Cc) <= 16384, (len(L), len(Cc))
    q0 = np.array([0.0, 0.0, 0.002, 1.0]); q0 /= np.linalg.norm(q0)
    pose0 = np.array([*q0, 0.5, -0.02, 0.01])
    fe, pb, table, spec, init, big, plan, BIG = _big_pair_case(oracle, dev, L, Cc, pose0, 16384)
    assert len(L) > plan["lds_cap"], plan
    for p in range(len(spec)):
        if p != BIG:
            one = _run(fe, pb, table, [spec[p]], init[p:p + 1], dev)
            _assert_same_bits(pb, big, p, one, spec[p])

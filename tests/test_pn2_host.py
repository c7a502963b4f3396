"""The CPU oracle of the TFlow point-set operators (oracle/pn2_oracle.c through oracle.pn2_*)
against the numpy yardstick tests/pn2_reference.py, which shares no text with it or with the
kernels, on the cases of tests/pn2_cases.py.  No GPU.  tests/test_gpu_pn2_yardstick.py runs the
same cases on the device under the same bars.

Bars: the oracle equals the yardstick's float32 layer bit for bit (FPS indices, k-NN indices and
distances, gathers, interpolation, upsample).  The float32 layer agrees with its float64 layer
on every decisive (query, rank) pair (gap > 2^-20) and within 3u sum|w f| (interpolate) and
(2k + 9)u sum|w f| (upsample); the derivations are in the yardstick's docstring.

Also here: the yardstick reproduces the golden vectors of the reference's own torch operators,
the cases are checked for what they claim, and every deliberately wrong rule of the yardstick
is shown to change the output of a named case.
"""
import os

import numpy as np
import pytest

import pn2_cases as pc
import pn2_reference as ref

F32 = np.float32
GOLD = os.path.join(os.path.dirname(__file__), "golden", "pn2_ref.npz")
same = pc.bits_equal


# ------------------------------------------------------------------------------- FPS
@pytest.mark.parametrize("cs", pc.fps_cases(), ids=lambda c: c.name)
def test_oracle_fps_equals_yardstick(oracle, cs):
    y = pc.fps_yard(cs.name)
    assert same(oracle.pn2_fps(cs.xyz, cs.npoint, start=cs.start), y), cs.name
    if not cs.exact:                        # the float64 layer, following the float32 choices
        want, gap = ref.fps64(cs.xyz, y, cs.start)
        dec = gap > ref.GAP_BAR
        live = dec[:, :cs.xyz.shape[1]]         # from step n on every distance is 0: a tie by construction
        assert np.array_equal(y[dec], want[dec]) and 1 - live.mean() <= pc.MAX_UNCLEAR, (cs.name, 1 - live.mean())


def test_fps_cases_cover_what_they_claim():
    by = {c.name: c for c in pc.fps_cases()}
    assert {c.xyz.shape[1] for c in by.values()} >= set(pc.FPS_N)
    starts = [c.start for c in by.values() if c.name.startswith("fps_noise")]
    assert any(s is None for s in starts) and any(s is not None and (s < 0).all() for s in starts)
    assert any(s is not None and (s >= c.xyz.shape[1]).all() for s, c in
               zip(starts, [c for c in by.values() if c.name.startswith("fps_noise")]))
    for n in (256, 4097, 16385):
        x = by[f"fps_ties_n{n}"].xyz
        y = pc.fps_yard(f"fps_ties_n{n}")
        m = (n + 1) // 2
        assert same(x[0, :n - m], x[0, m:]) and same(x[0] * 1, np.round(x[0]))        # every point twice, integers
        assert not same(x[0], x[1]) and not same(x[1], x[2])
        # the cap decides: the second centroid of the cluster cloud is the FIRST far point, and
        # some far point is farther than it
        c = x[2]
        first = int(np.nonzero(c[:, 0] > 1e5)[0][0])
        s0 = int(y[2, 0])
        if c[s0, 0] < 1e5:
            assert y[2, 1] == first
            d = ((c.astype(np.float64) - c[s0]) ** 2).sum(-1)
            assert d.argmax() != first and d[first] > 1e10
    y = pc.fps_yard("fps_npoint_gt_n")
    assert len(set(y[0, :37].tolist())) < 37 and (y[0, 37:] == 0).all()            # duplicates leave d = 0 early
    y = pc.fps_yard("fps_npoint_gt_n_noise")
    assert sorted(y[0, :37].tolist()) == list(range(37)) and (y[0, 37:] == 0).all()
    assert pc.fps_yard("fps_equal_n8193").tolist() == [[8191, 0, 0, 0, 0]]
    assert pc.fps_yard("fps_npoint_eq_n_start_neg")[0, 0] == 0 and pc.fps_yard("fps_npoint_eq_n_start_past")[0, 0] == 36


# ------------------------------------------------------------------------------- k-NN
@pytest.mark.parametrize("cs", pc.knn_cases(), ids=lambda c: c.name)
def test_oracle_knn_equals_yardstick(oracle, cs):
    yd, yi = pc.knn_yard(cs.name)
    for k in cs.ks:
        d, i = oracle.pn2_knn(k, cs.query, cs.ref)
        assert same(i, np.ascontiguousarray(yi[..., :k])), (cs.name, k)
        assert same(d, np.ascontiguousarray(yd[..., :k])), (cs.name, k)
    if not cs.exact:
        wrong, unclear = pc.knn_unclear(cs.name)
        assert wrong == 0 and unclear <= pc.MAX_UNCLEAR, (cs.name, wrong, unclear)


def test_knn_cases_cover_what_they_claim():
    by = {c.name: c for c in pc.knn_cases()}
    split = [c for c in by.values() if c.name.startswith("knn_split_")]
    wide = [c for c in by.values() if c.name.startswith("knn_wide_")]
    fam = lambda c: c.query.shape[0] * -(-c.query.shape[1] // 256) >= 512              # noqa: E731
    assert not any(fam(c) for c in split) and all(fam(c) for c in wide)
    assert {c.ref.shape[1] for c in split} >= set(pc.KNN_N) <= {c.ref.shape[1] for c in wide}
    assert {c.query.shape[1] for c in split} >= set(pc.KNN_S)
    assert {c.query.shape[0] for c in split} >= {1, 3}
    for c in by.values():                                            # batch elements differ
        if c.ref.shape[0] > 1:
            assert not same(c.query[0], c.query[1]) and not same(c.query[0], c.query[-1]), c.name
            assert c.exact or not same(c.ref[0], c.ref[1]), c.name
    for tag in ("split", "wide"):
        d, i = pc.knn_yard(f"knn_dups_straddle_{tag}")
        assert i[0, :3, :2].tolist() == [[255, 256], [511, 512], [2047, 2048]] and (d[0, :3, :2] == 0).all()
        d, i = pc.knn_yard(f"knn_on_refs_{tag}")
        assert i[0, :, 0].tolist() == [0, 256, 512] and (d[0, :, 0] == 0).all() and (d[0, :, 1] > 0).all()
        d, i = pc.knn_yard(f"knn_lattice_{tag}")
        assert d[0, 0, :8].tolist() == [0, 1, 1, 1, 1, 1, 1, F32(np.sqrt(F32(2)))]         # 4, 5 cut the shell of 6
        assert (np.diff(i[0, 0, 1:7]) > 0).all() and d[0, 0, 7] == d[0, 0, 18] < d[0, 0, 19]    # 8, 9, 16, 17 cut the shell of 12
        d, i = pc.knn_yard(f"knn_denormal_{tag}")
        tiny = np.finfo(F32).tiny
        d2 = ref.neighbours(by[f"knn_denormal_{tag}"].query, by[f"knn_denormal_{tag}"].ref, 32)[0]
        assert (d2[d2 > 0] < 4 * tiny).all() and (d2[..., 1:] > 0).all() and (d2 < tiny).mean() > 0.5
        assert (np.diff(d2, axis=-1) == 0).any()
        d, i = pc.knn_yard(f"knn_inf_{tag}")
        assert sorted(i[0, 0, :3].tolist()) == [4, 7, 12] and np.isfinite(d[0, :, :3]).all()
        assert i[0, 0, 3:13].tolist() == [0, 1, 2, 3, 5, 6, 8, 9, 10, 11] and np.isinf(d[0, :, 3:13]).all()
        assert (i[0, :, 13:] == 0).all() and (d[0, :, 13:] == 0).all()                      # k > n
    for n in (257, 2049):
        cs = by[f"knn_fma_tail_n{n}"]
        assert pc.knn_yard(cs.name)[1][0, 0, :2].tolist() == [n - 1, 0] and n % 2048 % 2 == 1
        assert ref.knn(2, cs.query, cs.ref, "fma")[1][0, 0].tolist() == [0, n - 1]
    d, i = pc.knn_yard("knn_split_n7_s63_b1")
    assert (i[..., 7:] == 0).all() and (d[..., 7:] == 0).all() and (d[..., 1:7] > 0).all()
    assert pc.knn_unclear("knn_near_sphere")[1] > 0.5


# ------------------------------------------------------------------------------- gathers

@pytest.mark.parametrize("cs", pc.gather_cases(), ids=lambda c: c.name)
def test_oracle_gather_equals_yardstick(oracle, cs):
    y, bad = ref.gather(cs.feat, cs.idx)
    n = cs.feat.shape[2]
    flat = cs.idx.reshape(cs.idx.shape[0], -1)
    assert not bad and (flat[:, 0] == 0).all() and (flat[:, -1] == n - 1).all()
    assert same(oracle.pn2_gather(cs.feat, cs.idx), y)
    for which in pc.BAD_INDICES:
        ix, at = pc.with_bad(cs.idx, n, which)
        yb, bad = ref.gather(cs.feat, ix)
        assert bad and (yb.reshape(yb.shape[0], yb.shape[1], -1)[at[0], :, at[1]] == 0).all()
        assert np.count_nonzero(yb != y) <= cs.feat.shape[1]
        assert same(oracle.pn2_gather(cs.feat, ix), yb)


@pytest.mark.parametrize("cs", pc.rel_cases(), ids=lambda c: c.name)
def test_oracle_group_relative_equals_yardstick(oracle, cs):
    y, bad = ref.group_relative(cs.xyz, cs.new_xyz, cs.points, cs.idx)
    assert not bad
    for which in (None,) + pc.BAD_INDICES:
        ix = cs.idx if which is None else pc.with_bad(cs.idx, cs.xyz.shape[2], which)[0]
        yb, bad = ref.group_relative(cs.xyz, cs.new_xyz, cs.points, ix)
        got = oracle.pn2_gather(cs.xyz, ix) - cs.new_xyz[..., None]
        if cs.points is not None:
            got = np.concatenate([got, oracle.pn2_gather(cs.points, ix)], axis=1)
        assert same(got, yb) and bad == (which is not None)
        if which is not None:
            b, j = pc.with_bad(cs.idx, cs.xyz.shape[2], which)[1]
            K = cs.idx.shape[2]
            assert same(yb[b, :3, j // K, j % K], -cs.new_xyz[b, :, j // K]) and (yb[b, 3:, j // K, j % K] == 0).all()
            assert np.count_nonzero(yb != y) <= yb.shape[1]


@pytest.mark.parametrize("cs", pc.interp_cases(), ids=lambda c: c.name)
def test_oracle_interpolate_equals_yardstick(oracle, cs, capsys):
    m = cs.feat.shape[2]
    for which in (None,) + pc.BAD_INDICES:
        ix = cs.idx if which is None else pc.with_bad(cs.idx, m, which)[0]
        y, bad = ref.three_interpolate(cs.feat, ix, cs.weight)
        got = oracle.pn2_three_interpolate(cs.feat, ix, cs.weight)
        assert same(got, y) and bad == (which is not None), (cs.name, which)
        y64, bound = ref.three_interpolate64(cs.feat, ix, cs.weight)
        worst = pc.worst_ratio(y, y64, bound)
        assert worst <= 1.0, (cs.name, worst)
    with capsys.disabled():
        print(f"\n  {cs.name}: worst |f32 - f64| / (3u sum|w f|) = {worst:.3f}")


# ------------------------------------------------------------------------------- upsample
@pytest.mark.parametrize("cs", pc.up_cases(), ids=lambda c: c.name)
def test_oracle_upsample_equals_yardstick(oracle, cs, capsys):
    worst = {}
    for k in cs.ks:
        y, y64, bound = pc.up_yard(cs.name, k)
        assert y.shape == (cs.xyz.shape[0], cs.sfeat.shape[1], cs.xyz.shape[2])
        assert same(oracle.pn2_upsample_flow(cs.xyz, cs.sxyz, cs.sfeat, k=k), y), (cs.name, k)
        worst[k] = pc.worst_ratio(y, y64, bound)
        assert worst[k] <= 1.0, (cs.name, k, worst[k])
    wrong, unclear = pc.up_unclear(cs.name)
    assert wrong == 0 and unclear <= pc.MAX_UNCLEAR
    with capsys.disabled():
        print(f"\n  {cs.name}: worst |f32 - f64| / ((2k+9)u sum|w f|) per k = "
              + ", ".join(f"{k}: {w:.3f}" for k, w in worst.items()))


def test_upsample_cases_cover_what_they_claim():
    by = {c.name: c for c in pc.up_cases()}
    fam = lambda c: c.xyz.shape[0] * -(-c.xyz.shape[2] // 256) >= 512              # noqa: E731
    assert sum(fam(c) for c in by.values()) == 3 and sum(not fam(c) for c in by.values()) == 5
    assert {c.sxyz.shape[2] for c in by.values()} >= {1, 2, 4095, 4096}
    assert {c.xyz.shape[2] for c in by.values()} >= {1, 63, 64, 65}
    assert {c.sfeat.shape[1] for c in by.values()} == {0, 1, 3}
    cs = by["up_b3_n65_s4096_c1"]
    d2 = pc.up_nbr(cs.name)[0]
    assert (d2[:, :2, 0] == 0).all() and (d2[:, 2:, 0] > 0).all()                  # d = 0 on the coincident points
    for k in (1, 3, 16):
        y = pc.up_yard(cs.name, k)[0]
        assert y[:, 0, 0].tolist() == [100.0] * 3 and y[:, 0, 1].tolist() == [-100.0] * 3
    y = pc.up_yard("up_b1_n64_s4095_c3", 3)[0]
    raw = ref.upsample_flow(by["up_b1_n64_s4095_c3"].xyz, by["up_b1_n64_s4095_c3"].sxyz,
                            by["up_b1_n64_s4095_c3"].sfeat, 3, "noclip")[0]
    assert (np.abs(raw) > 100).any() and (np.abs(raw) < 100).any() and np.abs(y).max() == 100
    # s < k: the weights of the s neighbours alone
    cs = by["up_b3_n63_s2_c3"]
    assert same(pc.up_yard(cs.name, 16)[0], pc.up_yard(cs.name, 3)[0])
    assert not same(pc.up_yard(cs.name, 1)[0], pc.up_yard(cs.name, 3)[0])


# ------------------------------------------------------------------------------- golden
def test_yardstick_reproduces_the_reference_vectors():
    """indices exact; distances and values within the golden's existing tolerances (torch's CPU
    sqrt is not correctly rounded, its sums run in another order: tests/test_oracle_pn2.py)"""
    g = dict(np.load(GOLD))
    assert same(ref.fps(g["xyz"], g["fps_idx"].shape[1], g["fps_start"]), g["fps_idx"])
    new_xyz = np.take_along_axis(g["xyz"], g["fps_idx"][..., None].astype(np.int64), axis=1)
    d, i = ref.knn(int(g["knn_k"]), new_xyz, g["xyz"])
    assert same(i, g["knn_idx"])
    np.testing.assert_allclose(d, g["knn_dist"], rtol=2.5e-7, atol=0)
    d, i = ref.knn(3, g["xyz"], new_xyz)
    assert same(i, g["three_idx"])
    np.testing.assert_allclose(d, g["three_dist"], rtol=2.5e-7, atol=0)
    assert same(ref.gather(g["feat"], g["fps_idx"])[0], g["gathered"])
    assert same(ref.gather(g["feat"], g["knn_idx"])[0], g["grouped"])
    np.testing.assert_allclose(ref.three_interpolate(g["sfeat"], g["three_idx"], g["three_weight"])[0],
                               g["interp"], rtol=1e-5, atol=1e-6)
    xyz = np.ascontiguousarray(g["xyz"].transpose(0, 2, 1))
    sxyz = np.ascontiguousarray(new_xyz.transpose(0, 2, 1))
    for k in (3, 5):
        y, idx = ref.upsample_flow(xyz, sxyz, g["sflow"], k)
        assert np.array_equal(idx, g[f"up{k}_idx"])
        np.testing.assert_allclose(y, g[f"up{k}"], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------- wrong rules
NAMED = {
    "ties to the higher index": "knn_dups_straddle_split",
    "d2 by the expanded form": "knn_offset_1000m",
    "d2 with fused multiply-add": "knn_fma_tail_n2049",
    "d2 summed z-first": "knn_split_n257_s300_b3",
    "selection by float64 d2": "knn_near_sphere",
    "fps without the 1e10 cap": "fps_ties_n256",
    "fps last-maximum": "fps_ties_n257",
    "clamp before sqrt": "up_b3_n65_s4096_c1",
    "weights normalised after the product": "up_b3_n63_s2_c3",
    "no +-100 clip": "up_b1_n64_s4095_c3",
    "interpolate summed right to left": "interp_b3_c35_m700_n65",
}


def _changed(variant, name):
    """what of the named case's asserted output the wrong rule changes"""
    family, sw = ref.VARIANTS[variant]
    if family == "knn":
        cs = pc.knn_case(name)
        yd, yi = pc.knn_yard(name)
        d, i = ref.knn(max(pc.KS), cs.query, cs.ref, sw)
        return [w for w, a, b in (("idx", i, yi), ("dist", d, yd)) if not same(a, b)]
    if family == "fps":
        cs = next(c for c in pc.fps_cases() if c.name == name)
        return [] if same(ref.fps(cs.xyz, cs.npoint, cs.start, sw), pc.fps_yard(name)) else ["idx"]
    if family == "upsample":
        cs = pc.up_case(name)
        return [k for k in cs.ks if not same(ref.upsample_flow(cs.xyz, cs.sxyz, cs.sfeat, k, sw, nbr=pc.up_nbr(name))[0],
                                             pc.up_yard(name, k)[0])]
    cs = next(c for c in pc.interp_cases() if c.name == name)
    return [] if same(ref.three_interpolate(cs.feat, cs.idx, cs.weight, sw)[0],
                      ref.three_interpolate(cs.feat, cs.idx, cs.weight)[0]) else ["value"]


def test_every_variant_is_named():
    assert set(NAMED) == set(ref.VARIANTS)


@pytest.mark.parametrize("variant", list(ref.VARIANTS))
def test_wrong_rule_changes_a_named_case(variant, capsys):
    hit = _changed(variant, NAMED[variant])
    with capsys.disabled():
        print(f"\n  {variant}: changes {hit} of {NAMED[variant]}")
    assert hit, f"{NAMED[variant]} does not distinguish the rule {variant!r}"
    if ref.VARIANTS[variant][1] in ("ties_high", "expanded", "fma", "select_f64"):
        assert "idx" in hit                                     # a wrong neighbour, not a last bit


def test_yardstick_by_hand():
    x = np.zeros((1, 5, 3), F32)
    x[0, :, 0] = [0, 1, 2, 3, 4]
    assert ref.fps(x, 3).tolist() == [[0, 4, 2]] and ref.fps(x, 3, [9]).tolist() == [[4, 0, 2]]
    d, i = ref.knn(2, np.zeros((1, 1, 3), F32), np.array([[[1, 0, 0], [-1, 0, 0], [0, 0.5, 0]]], F32))
    assert i.tolist() == [[[2, 0]]] and d.tolist() == [[[0.5, 1.0]]]
    i64, gap = ref.knn64(2, np.zeros((1, 1, 3), F32), np.array([[[1, 0, 0], [-1, 0, 0], [0, 0.5, 0]]], F32))
    assert i64.tolist() == [[[2, 0]]] and gap.tolist() == [[[0.75, 0.0]]]
    d, i = ref.knn(3, np.zeros((1, 1, 3), F32), np.ones((1, 2, 3), F32))
    assert i.tolist() == [[[0, 1, 0]]] and d[0, 0, 2] == 0
    f = np.arange(6, dtype=F32).reshape(1, 2, 3)
    y, bad = ref.gather(f, np.array([[2, 3, -1, 0]], np.int32))
    assert bad and y.tolist() == [[[2, 0, 0, 0], [5, 0, 0, 3]]]
    y, bad = ref.three_interpolate(f, np.array([[[0, 1, 2]]], np.int32), np.array([[[0.5, 0.25, 0.25]]], F32))
    assert not bad and y.tolist() == [[[0.75], [3.75]]]
    # coincident point: the clamped distance 1e-10 dominates the weights
    xyz = np.zeros((1, 3, 1), F32)
    sx = np.array([[[0.0, 1.0, 2.0], [0, 0, 0], [0, 0, 0]]], F32)
    sf = np.array([[[7.0, 1.0, 1.0]]], F32)
    assert ref.upsample_flow(xyz, sx, sf, 3)[0].tolist() == [[[7.0]]]
    assert ref.upsample_flow(xyz + 1, sx, 300 * sf, 1)[0].tolist() == [[[100.0]]]
    with pytest.raises(AssertionError):
        ref.knn(1, np.full((1, 1, 3), np.nan, F32), np.zeros((1, 1, 3), F32))
    with pytest.raises(AssertionError):
        ref.upsample_flow(xyz, np.full((1, 3, 2), 1e20, F32), sf[..., :2], 2)

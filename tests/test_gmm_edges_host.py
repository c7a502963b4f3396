"""The CPU oracle against sklearn on tiny, tied and degenerate frames (tests/golden/gmm_edges.npz,
written by tests/golden/make_golden_gmm_edges.py from sklearn 1.7.2 and the reference's own
slove_RT_by_SVD; the generator's header lists the families and the admission rules).

Every fixture was admitted on the reference side alone: each decision of the fit (k-means++
indices, the Lloyd and EM stopping tests, the final labels) clears its threshold by a margin that
rounding cannot bridge, so the bars are equalities: centre indices, iteration counts and the
background mask array_equal, the lower bound within 1e-9 (the project's bar), and the pose
  * against the reference's R, t (R within 1e-6, t within 1e-5) where the cross-covariance of the
    background rows has full rank (sigma3 / sigma1 > 1e-6),
  * by the rank rules of DESIGN 6.2 (rigid_cases.check_rank_case) where it has not: numpy's R
    there is LAPACK's choice of a null space, not a property of the input.
edge_fixtures() / check_fit() / check_pose() are shared with tests/test_gpu_mask_edges.py.
"""
import functools
import os

import numpy as np
import pytest

import rigid_cases as RC

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "gmm_edges.npz")
FIELDS = ("pos1", "flow", "seed", "draws", "labels", "bg_label", "kmeans_pp_idx", "kmeans_n_iter",
          "gmm_n_iter", "gmm_converged", "gmm_lower_bound", "R", "t", "raised", "sv", "margins",
          "lb_scale", "zero_extent")
LB_BAR, R_BAR, T_BAR, FULL_RANK = 1e-9, 1e-6, 1e-5, 1e-6
# the fixtures with a label of coincident rows beside another label (zero_extent in the file)
ZERO_EXTENT = ["mass_150_50", "mass_50_150", "size_n2", "size_n3", "size_n5", "tie_mass_ab", "tie_mass_ba"]


def device_lower_bound_bar(fx):
    """1e-9, except on the ZERO_EXTENT fixtures.  The kernel's EM pass sums the lower bound as
    (C0 + sum_i max(delta_i, 0) + log1p(e_i)) / n with C0 = sum_i a0_i taken from the pass-0
    moments (tr(P0 S_tot), mask_gmm.hpp) and delta = a1 - a0.  Where a component's covariance is
    reg_covar alone (precision 1e6) the other label's rows have a0 = -M, M = 0.5e6 d^2 ~ 1e7..1e8
    (lb_scale in the file, from sklearn's _estimate_weighted_log_prob), which the sum of
    delta cancels: every rounding of a term of size M -- the 27 products of a quadratic form,
    twice (delta_i and C0), the n - 1 additions of each sum, the moments' own n - 1, 9 more in
    the M-step's algebra -- leaves up to 2^-53 M in the mean.  sklearn adds a_k per point and has
    no such term.  (2 n + 63) 2^-53 M bounds it; measured on MI355X: 3.1e-9 (n = 2), 1.4e-8
    (n = 3), 5.3e-9 (n = 5), 9.4e-10 and 1.1e-10 (the point masses), about 2^-53 M each."""
    if not int(fx["zero_extent"]):
        return LB_BAR
    return max(LB_BAR, (2 * len(fx["labels"]) + 63) * 2.0 ** -53 * float(fx["lb_scale"]))


@functools.lru_cache(maxsize=None)
def edge_fixtures():
    """-> ({name: {field: array}}, margin names, margin thresholds, the raw file)"""
    g = np.load(GOLDEN)
    fx = {str(k): {f: g[f"{k}/{f}"] for f in FIELDS} for k in g["names"]}
    for f in fx.values():
        f["bg_mask"] = (f["labels"] == int(f["bg_label"])).astype(np.uint8)
    return fx, [str(k) for k in g["margin_names"]], g["margin_thresholds"], g


NAMES = sorted(edge_fixtures()[0])


def check_fit(fx, c0, c1, km_iter, em_iter, converged, lower_bound, bg_mask, bg_label, n_bg, lb_bar=LB_BAR):
    """the fit fields of one result against the fixture -> the lower bound's gap"""
    assert [int(c0), int(c1)] == [int(v) for v in fx["kmeans_pp_idx"]]
    assert int(km_iter) == int(fx["kmeans_n_iter"]) and int(em_iter) == int(fx["gmm_n_iter"])
    assert int(converged) == int(fx["gmm_converged"])
    gap = abs(float(lower_bound) - float(fx["gmm_lower_bound"]))
    assert gap < lb_bar, (gap, lb_bar)
    assert np.array_equal(np.asarray(bg_mask), fx["bg_mask"])
    assert int(bg_label) == int(fx["bg_label"])
    assert int(n_bg) == int(fx["bg_mask"].sum())
    return gap


def check_pose(fx, R, t):
    """-> (|dR|, |dt|) against the reference on a full-rank background, else (nan, nan) after
    the rank rules held"""
    sv = fx["sv"]
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).ravel()
    if sv[0] > 0.0 and sv[2] / sv[0] > FULL_RANK:
        assert int(fx["raised"]) == 0
        dR, dt = np.abs(R - fx["R"]).max(), np.abs(t - fx["t"]).max()
        assert dR < R_BAR and dt < T_BAR, (dR, dt)
        return dR, dt
    m = fx["bg_mask"] != 0
    p, f = fx["pos1"][m].astype(np.float64), fx["flow"][m].astype(np.float64)
    RC.check_rank_case("zero" if sv[0] == 0.0 else "deficient", p + f, p, R, t)
    return np.nan, np.nan


def test_families_and_margins():
    """what the file holds: every family of the generator, and every stored margin at or above its
    threshold (the admission, re-checked)"""
    fx, mnames, thr, g = edge_fixtures()
    assert mnames == ["kpp", "c0", "trials", "em", "resp", "kmeans"]
    assert list(thr) == [1e-9, 1e-9, 1e-9, 1e-6, 1e-6, 1e-6]
    for n in (2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 257, 766):
        assert len(fx[f"size_n{n}"]["pos1"]) == n
    for k, f in fx.items():
        assert f["pos1"].dtype == np.float32 and f["flow"].dtype == np.float32, k
        assert f["pos1"].shape == f["flow"].shape == (len(f["labels"]), 3), k
        assert np.all(f["margins"] >= thr), (k, f["margins"])
    ties = [k for k in fx if k.startswith("tie_")]
    assert len(ties) == 6
    for k in ties:                                   # exact ties, resolved to point 0's label
        f = fx[k]
        assert 2 * int(f["bg_mask"].sum()) == len(f["labels"]), k
        assert int(f["bg_label"]) == int(f["labels"][0]), k
    assert {int(fx[k]["bg_label"]) for k in ties} == {0, 1}
    assert {int(fx[k]["labels"][0] == fx[k]["labels"][1]) for k in ties} == {0, 1}   # interleaved and blocks
    for k in ("identical_200", "zeros_200"):         # one label
        assert fx[k]["bg_mask"].all() and int(fx[k]["bg_label"]) == 0
    # the device's wider lower-bound bar reaches these seven fixtures and no other, and stays
    # three orders below what the EM stopping test (1e-3, margin 1e-6) could notice
    assert sorted(k for k, f in fx.items() if int(f["zero_extent"])) == ZERO_EXTENT
    for k, f in fx.items():
        bar = device_lower_bound_bar(f)
        assert (LB_BAR < bar < 1e-5) if k in ZERO_EXTENT else bar == LB_BAR, (k, bar)
    assert not fx["zero_flow_300"]["flow"].any()
    assert np.abs(fx["far_2000"]["pos1"]).max() > 5000
    assert int(fx["long_em"]["gmm_n_iter"]) >= 20 and int(fx["long_em"]["gmm_converged"]) == 1
    assert sum(1 for f in fx.values() if f["sv"][0] == 0.0) >= 7          # H = 0
    assert sum(1 for f in fx.values() if f["sv"][0] > 0.0 and f["sv"][2] / f["sv"][0] <= FULL_RANK) >= 1


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_sklearn(oracle, name):
    fx = edge_fixtures()[0][name]
    res = oracle.mask_and_pose(fx["pos1"], fx["flow"], fx["draws"])
    info = res["info"]
    assert res["rc"] == 0
    gap = check_fit(fx, info["center0"], info["center1"], info["kmeans_iter"], info["em_iter"],
                    info["converged"], info["lower_bound"], res["bg_mask"], info["bg_label"], info["n_bg"])
    assert np.array_equal(res["labels"], fx["labels"])
    dR, dt = check_pose(fx, res["R"], res["t"])
    print(f"{name}: n={len(fx['labels'])} lb gap {gap:.3e} dR {dR:.3e} dt {dt:.3e}")


@pytest.mark.parametrize("n", [1, 0])
def test_fewer_than_two_points_is_a_value_error(oracle, n):
    """sklearn raises ValueError on one row and on none; so does the oracle, and so does
    ssf.mask_and_pose by its contract: SSF_POSE_GMM_FAILED surfaces as ValueError."""
    from ssf import _abi, pose
    g = edge_fixtures()[3]
    assert int(g[f"sklearn_raises_valueerror_n{n}"]) == 1
    with pytest.raises(ValueError):
        oracle.mask_and_pose(np.ones((n, 3), np.float32), np.ones((n, 3), np.float32), [0.3, 0.6, 0.9])
    with pytest.raises(ValueError):
        pose._raise_status(_abi.POSE_GMM_FAILED)

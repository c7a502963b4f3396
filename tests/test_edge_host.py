"""The CPU oracle's edge selection and line table (oracle/edge_oracle.c: orc_select_edges,
orc_extract_features, orc_edge_table, orc_sym3_eig) against yardsticks that share no text with it
or with the kernels: tests/feature_reference.py (select_edges, written from the definition in the
oracle's header comment) and tests/edge_reference.py (line_table: lexsort 5-NN, np.linalg.eigh).
No GPU.  tests/test_gpu_edge_yardstick.py runs the same cases on the device under the same bars.

Bars (tests/edge_cases.py: compare_table): edge lists and counts bit for bit; valid's gate on every
point and its ratio test where the yardstick's lambda1 / (line_ratio lambda2) is further than 1e-9
from 1 (a 5-point float64 covariance and its eigenvalues carry relative errors near 1e-15) or the
covariance is diagonal; centroid equal bits on exact geometry, else equal or adjacent float32;
direction per component within 2^-23 where valid or (lambda1 - lambda2) / lambda1 >= 1/2, up to
sign where the two largest |u| components are within 1e-6; m < 5 exactly zero.

Also here: the cases are checked for what they claim on the yardstick alone, and every deliberately
wrong rule of the yardsticks is shown to change the asserted result of a named case.
"""
import functools

import numpy as np
import pytest

import edge_cases as ec
import edge_reference as er
import feature_cases as fc
import feature_reference as ref
import registration_cases as rc
from test_feature_host import bits_equal, seen_cloud

F32 = np.float32


@functools.lru_cache(maxsize=None)
def seen(n_rows, name, layout):
    """(cloud the stage sees, the yardstick's extract_planes of it) -- computed once"""
    cs = next(c for c in ec.selection_cases(n_rows) if c.name == name)
    pts, keep = fc.layout(cs, layout)
    cloud = seen_cloud(pts, keep)
    return cloud, ref.extract_planes(cloud, n_rows)


def edge_bound(n, span, n_rows):
    """Frontend.extract_features_batch's bound on a frame's edge count"""
    return min(n, n // max(1, span) + n_rows + 1)


# ------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("layout", fc.LAYOUTS)
@pytest.mark.parametrize("n_rows", [16, 64])
def test_oracle_selection_equals_yardstick(oracle, n_rows, layout):
    for cs in ec.selection_cases(n_rows):
        cloud, y = seen(n_rows, cs.name, layout)
        for tag, em, span in ec.selection_runs(n_rows):
            what = (cs.name, n_rows, layout, tag)
            E, esel = ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, em, span)
            got = oracle.select_edges(y["rx"], y["cv"], y["off"], n_rows, edge_min=float(em), edge_span=span)
            assert bits_equal(got, E), (what, "select_edges", len(got), len(E))
            P, G = oracle.extract_features(cloud, n_rows, edge_min=float(em), edge_span=span)
            assert bits_equal(P, y["planes"]), (what, "planes")
            assert bits_equal(G, E), (what, "extract_features", len(G), len(E))
            assert len(E) <= edge_bound(len(cloud), span, n_rows), what


@pytest.mark.parametrize("n_rows", [16, 64])
def test_oracle_selection_padded_past_the_single_read_capacity(oracle, n_rows):
    dense = next(c for c in fc.cases(n_rows) if c.name == "dense")
    big = fc.binned(dense)
    y = ref.extract_planes(big, n_rows)
    for tag, em, span in ec.selection_runs(n_rows):
        E, _ = ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, em, span)
        P, G = oracle.extract_features(big, n_rows, edge_min=float(em), edge_span=span)
        assert bits_equal(P, y["planes"]) and bits_equal(G, E), (tag, len(G), len(E))


@pytest.mark.parametrize("n_rows", [16, 64])
def test_selection_cases_cover_what_they_claim(n_rows):
    rows_in = fc.in_range(n_rows)
    base = ec.base_edge_min(n_rows)
    assert set(ec.SPANS) >= {1, 63, 64, 65} and max(ec.SPANS) > 128
    names = [c.name for c in ec.selection_cases(n_rows)]
    assert {"dense", "nonfinite", "threshold", "long_row", "flat"} <= set(names) and len(set(names)) == len(names)
    # rows of every length, in range
    have = set()
    for name in [n for n in names if n.startswith("lengths")]:
        _, y = seen(n_rows, name, "rowmajor")
        have |= {int(y["off"][r + 1] - y["off"][r]) for r in rows_in}
    assert have >= set(fc.row_lengths(n_rows))
    # a row of more than 4097 points whose candidates the span-1 walk takes one by one
    _, y = seen(n_rows, "long_row", "rowmajor")
    r = fc.LONG_ROW[n_rows]
    a, b = int(y["off"][r]), int(y["off"][r + 1])
    assert r in rows_in and b - a == fc.LONG_ROW_POINTS > 4097
    E, esel = ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, base, 1)
    in_row = esel[(esel >= a) & (esel < b)]
    assert np.array_equal(in_row, a + np.nonzero(y["cv"][a:b] > base)[0]) and 0.25 * (b - a) < len(in_row) < 0.75 * (b - a)
    assert np.any(np.diff(in_row) == 1) and in_row.max() - a > 4097
    assert len(E) <= len(y["rx"]) == edge_bound(len(y["rx"]), 1, n_rows)      # at span 1 the bound is the frame
    # no curvature above edge_min: an empty list from a full frame, for every run
    _, y = seen(n_rows, "flat", "rowmajor")
    for tag, em, span in ec.selection_runs(n_rows):
        assert len(y["rx"]) > 1000 and not np.any(y["cv"] > em), tag
        assert len(ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, em, span)[0]) == 0
    # edge_min at a curvature value of the named row: the strict > decides that point alone
    r, j, tg = ec.edge_min_targets(n_rows)
    _, y = seen(n_rows, "dense", "rowmajor")
    pos = int(y["off"][r]) + j
    assert r in rows_in and 5 <= j < int(y["off"][r + 1] - y["off"][r]) - 5
    assert y["cv"][pos].view(np.uint32) == tg["equal"].view(np.uint32) and tg["below"] < tg["equal"] < tg["above"]
    sels = {k: ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, t, 1)[1] for k, t in tg.items()}
    assert pos in sels["below"] and pos not in sels["equal"] and pos not in sels["above"]
    assert len(sels["below"]) == len(sels["equal"]) + 1 == len(sels["above"]) + 1
    # infinite curvature passes, NaN never does; in every layout
    zr = fc.ZERO_ROW[n_rows]
    for which in fc.LAYOUTS:
        _, y = seen(n_rows, "nonfinite", which)
        a, b = int(y["off"][zr]), int(y["off"][zr + 1])
        for span in (1, 10):
            _, esel = ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, base, span)
            assert np.isinf(y["cv"][esel]).any() and not np.isnan(y["cv"][esel]).any(), which
        _, esel = ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, base, 1)
        assert set(a + np.nonzero(np.isinf(y["cv"][a:b]))[0]) <= set(esel.tolist())
        assert np.isnan(y["cv"][a:b]).any()
    # the noisy frames hold edge and plane candidates side by side
    for name in ("dense", "dense_equal"):
        _, y = seen(n_rows, name, "rowmajor")
        a, b = y["off"][rows_in[0]], y["off"][rows_in[-1] + 1]
        share = float(np.mean(y["cv"][a:b] > base))
        assert 0.25 <= share <= 0.60, (name, share)
    # the edge walk has a jstart of its own: some edge is emitted inside a plane pick's span
    _, y = seen(n_rows, "dense", "rowmajor")
    _, esel = ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, base, 3)
    gap = esel[:, None] - y["sel"][None, :]
    assert np.any((gap > 0) & (gap < ref.PROFILES[n_rows]["span"]))


def _selection_hits(kw):
    hits = []
    for n_rows in (64, 16):
        for cs in ec.selection_cases(n_rows):
            for tag, em, span in ec.selection_runs(n_rows):
                if span + kw.get("span_delta", 0) < 1:
                    continue
                want = ref.extract_features(cs.pts, n_rows, em, span)["edges"]
                if not bits_equal(ref.extract_features(cs.pts, n_rows, em, span, **kw)["edges"], want):
                    hits.append((cs.name, n_rows, tag))
                    break
    return hits


@pytest.mark.parametrize("variant", list(ref.EDGE_VARIANTS))
def test_wrong_selection_rule_changes_an_edge_list(variant, capsys):
    hit = _selection_hits(ref.EDGE_VARIANTS[variant])
    with capsys.disabled():
        print(f"\n  {variant}: caught by {hit}")
    assert hit, f"no case distinguishes the rule {variant!r}: a case is missing"
    if variant == ">= for >":                      # the case built for it is among them
        assert any(tag == "edge_min_equal" for _, _, tag in hit), hit


def test_yardstick_selection_by_hand():
    """one row of the 16-row profile (row_start 0): curvature given by hand.  edge_min 1, span 3:
    j = 2 (5.0) is taken, j = 3 and 4 are inside its span, j = 5 (exactly 1.0) is not above 1,
    j = 6 (inf) is taken, j = 8 is NaN, j = 9 (1.0000001) is taken, j = 11 is inside its span."""
    cv = np.array([0, 0.5, 5, 7, 9, 1, np.inf, 0, np.nan, np.nextafter(F32(1), F32(2)), 0, 3], F32)
    rx = np.c_[np.arange(12), np.zeros(12), np.zeros(12), np.arange(12)].astype(F32)
    off = np.zeros(17, np.int64)
    off[1:] = 12
    E, esel = ref.select_edges(rx, cv, off, 16, 1.0, 3)
    assert esel.tolist() == [2, 6, 9] and bits_equal(E, rx[[2, 6, 9]])
    assert ref.select_edges(rx, cv, off, 16, 1.0, 1)[1].tolist() == [2, 3, 4, 6, 9, 11]
    assert ref.select_edges(rx, cv, off, 16, 1.0, 3, ge=True)[1].tolist() == [2, 5, 9]
    # the 64-row profile skips rows 0-4 and 59-63
    off64 = np.zeros(65, np.int64)
    off64[5:] = 12
    assert ref.select_edges(rx, cv, off64, 64, 1.0, 3)[1].tolist() == []          # the points are in row 4
    off64[5] = 0
    assert ref.select_edges(rx, cv, off64, 64, 1.0, 3)[1].tolist() == [2, 6, 9]   # ... in row 5


# ------------------------------------------------------------------------------- sym3_eig
def _rot(ax, ang):
    ax = np.asarray(ax, float) / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def test_sym3_eig_against_eigh(oracle):
    """orc_sym3_eig against np.linalg.eigh.  Both are backward stable: cyclic Jacobi converges on
    a 3 x 3 in at most four sweeps of three rotations, each a perturbation of a rounding or two of
    the norm, so its eigenvalues are those of A + E with |E| within about 16 roundings of |A|
    (EPS16 = 16 * 2^-52, not a measured figure); eigh's bound is of the same kind.  Eigenvalues
    agree within EPS16 |A|, the residual |A v - w v| is within 2 EPS16 |A|, V is orthonormal;
    where an eigenvalue is separated from the others by more than 1e-3 |A| its vector agrees
    with eigh's up to sign within 1e-12 (EPS16 / 1e-3 with room)."""
    EPS16 = 16 * 2.0 ** -52
    R = _rot([1, 2, 3], 0.7)
    v = np.array([0.3, -1.2, 0.5])
    mats = {
        "diagonal": np.diag([3.0, 1.0, 2.0]),
        "rank1": np.outer(v, v),
        "rank0": np.zeros((3, 3)),
        "nearly_isotropic": np.eye(3) + 1e-9 * (R @ np.diag([3.0, 2.0, 1.0]) @ R.T),
        "graded_1e12": R @ np.diag([1e12, 1.0, 1e-12]) @ R.T,
        "graded_1e12_diag": np.diag([1e-12, 1e12, 1.0]),
        # a12 = 0 and a13, a23 != 0: the first rotation of the sweep is skipped (apq == 0)
        "apq_zero_skip": np.array([[2.0, 0.0, 0.5], [0.0, 1.0, -0.25], [0.5, -0.25, 3.0]]),
        "apq_zero_twice": np.array([[2.0, 0.0, 0.0], [0.0, 1.0, -0.25], [0.0, -0.25, 3.0]]),
    }
    for name, A in mats.items():
        A = 0.5 * (A + A.T)
        w, V = oracle.sym3_eig(A)
        yw, yV = np.linalg.eigh(A)
        scale = max(np.abs(yw).max(), 1e-300)
        order = np.argsort(w, kind="stable")
        assert np.abs(w[order] - yw).max() <= EPS16 * scale, (name, w, yw)
        assert np.abs(V.T @ V - np.eye(3)).max() < 1e-14, name
        assert np.abs(A @ V - V * w[None, :]).max() <= 2 * EPS16 * scale, name
        for k, col in enumerate(order):
            sep = np.min(np.abs(np.delete(yw, k) - yw[k]))
            if sep > 1e-3 * scale:
                assert abs(abs(V[:, col] @ yV[:, k]) - 1) < 1e-12, (name, k)
        if name in ("diagonal", "graded_1e12_diag", "rank0"):
            assert np.array_equal(w, np.diag(A)) and np.array_equal(V, np.eye(3)), name     # untouched


# ------------------------------------------------------------------------------- line table
def _batch_tables(batch):
    return [(fname, fr, ec.yardstick_table(fname, fr, batch.max_nn_d2, batch.line_ratio)) for fname, fr in batch.frames]


@pytest.mark.parametrize("batch", ec.line_batches(), ids=lambda b: b.name)
def test_oracle_edge_table_against_yardstick(oracle, batch, capsys):
    worst, unclear, cen, open_signs = 0.0, 0, 0, []
    for fname, fr, y in _batch_tables(batch):
        L, V = oracle.edge_table(fr, max_nn_d2=batch.max_nn_d2, line_ratio=batch.line_ratio)
        bad, st = ec.compare_table(L, V, y, batch.max_nn_d2, batch.exact, ec.always_asserted(fname))
        assert not bad, (batch.name, fname, bad)
        worst, unclear, cen = max(worst, st["worst_dir"]), unclear + st["unclear_ratio"], cen + st["cen_differs"]
        open_signs += [(fname,) + s for s in st["signs"]]
    with capsys.disabled():
        print(f"\n  {batch.name}: worst oracle-to-yardstick direction gap {worst:.3g} (bar {ec.DIR_TOL:.3g}), {cen} centroid "
              f"rows one float off, {unclear} rows with an unasserted ratio test; open signs (frame, row, oracle, "
              f"yardstick): {open_signs[:6]}")


def test_line_cases_cover_what_they_claim():
    by = {b.name: b for b in ec.line_batches()}
    sizes = by["sizes"]
    assert [len(fr) for _, fr in sizes.frames[:len(ec.SIZES)]] == list(ec.SIZES)
    cap = rc.edge_lds_cap()
    assert cap == rc.EDGE_LDS_CAP and {cap, cap + 1} <= set(ec.SIZES) and {0, 1, 4, 5, 6, 1023, 1024, 1025} <= set(ec.SIZES)
    assert [len(fr) for _, fr in by["mixed"].frames] == [cap + 1, 6, 0, 1025]
    # every seeded frame: the ratio test of every point is clear of its threshold, no NaN
    # coordinate; the big frames hold valid and invalid rows
    for batch in (sizes, by["mixed"]):
        for fname, fr, y in _batch_tables(batch):
            assert np.isfinite(fr).all(), fname
            if len(fr) >= er.K:
                assert np.all(np.abs(y["ratio"] - 1.0) > ec.RATIO_CLEAR), (fname, np.abs(y["ratio"] - 1).min())
            if len(fr) >= 1023:
                assert 0.2 < y["valid"].mean() < 0.95, (fname, y["valid"].mean())
            if len(fr) < er.K:
                assert not y["valid"].any() and not y["line"].any()
    t = {fname: y for fname, _, y in _batch_tables(sizes)}
    fr = dict(sizes.frames)
    assert t["axes"]["valid"].mean() > 0.8 and t["random_lines"]["valid"].mean() > 0.8
    assert t["planar_blobs"]["valid"].mean() < 0.8 and t["isotropic_blobs"]["valid"].mean() < 0.5
    # planar: lambda1 ~ lambda2 >> lambda3 -- the second LARGEST eigenvalue decides
    lam = t["planar_blobs"]["lam"]
    assert np.median(lam[:, 1] / lam[:, 0]) > 0.2 and np.median(lam[:, 2] / lam[:, 0]) < 0.01
    for k in range(3):                       # each axis line: its own component the largest
        assert np.all(np.argmax(np.abs(t["axes"]["line"][40 * k:40 * (k + 1), 3:]), 1) == k)
    d = np.abs(t["diagonals"]["line"][:, 3:])
    assert np.all(np.abs(d[:40, 0] - d[:40, 1]) < 0.05) and np.all(np.abs(d[40:] - 3 ** -0.5) < 0.05)
    assert {0, 1} <= set(np.argmax(d[:40], 1).tolist())          # the largest component is the noise's choice
    assert np.linalg.norm(fr["far_5km"][:, :3], axis=1).min() > 4900
    # 2 cm apart: a point's five nearest come from both lines
    idx = t["parallel_2cm"]["idx"]
    assert np.mean((idx < 40).any(1) & (idx >= 40).any(1)) > 0.9
    # the exact frames
    r4 = {fname: y for fname, _, y in _batch_tables(by["exact_ratio4"])}
    r3 = {fname: y for fname, _, y in _batch_tables(by["exact_ratio3"])}
    g_at = {fname: y for fname, _, y in _batch_tables(by["exact_gate_at"])}
    g_ab = {fname: y for fname, _, y in _batch_tables(by["exact_gate_above"])}
    y, X = r4["exact_diag"], dict(by["exact_ratio4"].frames)["exact_diag"]
    rows = ec.exact_cluster_rows
    assert np.array_equal(X[:, :3] * 4, np.round(X[:, :3] * 4))                    # integer / 4
    A_off = lambda a: X[y["idx"][a], :3].astype(np.float64)                         # noqa: E731
    for a in range(len(X)):                                                          # diagonal or zero covariance
        v = A_off(a) - A_off(a).mean(0)
        C = v.T @ v
        assert np.count_nonzero(C - np.diag(np.diag(C))) == 0, a
        assert len(set(np.round(X[y["idx"][a], 1] / 64.0).tolist())) == 1, a         # its own cluster's points
    # ties for the 5th neighbour: the query at x = 0, the lower index wins
    for name, q, want_x, where in (("tie_low", 3, -0.75, (-1, 1)), ("tie_reversed", 2, 0.75, (-1, 1)),
                                   ("tie_after", 0, 0.75, (1, 1)), ("tie_before", 5, 0.75, (-1, -1))):
        a = rows(name)[q]
        assert X[a, 0] == 0 and y["gap5"][a] == 0 and y["d2"][a, 4] == F32(9 / 16)
        won = y["idx"][a, 4]
        assert X[won, 0] == want_x, name
        lost = [k for k in rows(name) if X[k, 0] == -want_x][0]
        assert won < lost and (np.sign(won - a), np.sign(lost - a)) == where, name
    assert np.all(y["lam"][rows("five_copies")] == 0) and not y["valid"][rows("five_copies")].any()
    assert np.all(y["lam"][rows("collinear"), 1] == 0) and y["valid"][rows("collinear")].all()
    assert np.all(y["lam"][rows("ratio4_at"), 0] == 4.0 * y["lam"][rows("ratio4_at"), 1])
    assert not y["valid"][rows("ratio4_at")].any() and y["valid"][rows("ratio4_above")].all()
    assert r3["exact_diag"]["valid"][rows("ratio4_at")].all()
    assert r3["exact_diag"]["valid"][rows("ratio3_rounding")].all() and not y["valid"][rows("ratio3_rounding")].any()
    assert np.all(np.abs(r3["exact_diag"]["ratio"][rows("ratio3_rounding")] - 1) < 1e-15)
    ends = rows("gate")[[0, 4]]
    assert np.all(y["d2"][ends, 4] == F32(ec.GATE_D2)) and np.all(y["d2"][ends, 3] == F32(9 / 16))
    assert not g_at["exact_diag"]["valid"][ends].any() and g_ab["exact_diag"]["valid"][ends].all()
    assert g_at["exact_diag"]["valid"][rows("gate")[1:4]].all()
    # exactly collinear, oblique: lambda2 is the eigensolver's rounding of zero, the sign is open
    yo = r4["exact_oblique"]
    assert np.all(np.abs(yo["lam"][:, 1]) < 1e-15 * yo["lam"][:, 0]) and yo["valid"].all()
    assert np.all(yo["sign_gap"] < ec.SIGN_CLEAR)


@pytest.mark.parametrize("variant", list(er.LINE_VARIANTS))
def test_wrong_line_rule_changes_an_asserted_result(variant, capsys):
    """the wrong table of every frame (the big ones aside: nothing is reached there that the
    small ones do not reach) goes through compare_table as an implementation's would"""
    hit = []
    for batch in ec.line_batches():
        for fname, fr, y in _batch_tables(batch):
            if len(fr) > 1100:
                continue
            w = ec.yardstick_table(fname, fr, batch.max_nn_d2, batch.line_ratio, variant)
            bad, _ = ec.compare_table(w["line"], w["valid"], y, batch.max_nn_d2, batch.exact, ec.always_asserted(fname))
            if bad:
                hit.append((batch.name, fname, bad[0][:60]))
    with capsys.disabled():
        print(f"\n  {variant}: caught by {[(b, f) for b, f, _ in hit]}")
    assert hit, f"no case distinguishes the rule {variant!r}: a case is missing"
    named = {"ties broken to the higher index": "exact_diag", "covariance divided by 4": "exact_diag",
             "the gate on d2[3]": "exact_diag", ">= in the ratio test": "exact_diag",
             "the second-largest eigenvalue taken as the smallest": "planar_blobs",
             "the sign fixed on component 0": "axes", "the point excluded from its own 5-NN": "random_lines"}
    assert any(f == named[variant] for _, f, _ in hit), (variant, hit)


def test_yardstick_line_table_by_hand():
    """five points of the x axis at 0, 1, 2, 3, 4 and a far sixth: centroid (2, 0, 0), covariance
    diag(2, 0, 0), u = +x; the gate is d2[4] = 16 for the end points and 4 for the middle one"""
    X = np.zeros((6, 4), F32)
    X[:5, 0] = np.arange(5)
    X[5, :3] = (100, 100, 100)
    y = er.line_table(X, 10.0, 3.0)
    assert np.array_equal(y["line"][:5], np.tile(F32([2, 0, 0, 1, 0, 0]), (5, 1)))
    assert np.allclose(y["lam"][:5], [[2, 0, 0]] * 5) and y["valid"].tolist() == [0, 1, 1, 1, 0, 0]
    assert y["d2"][0].tolist() == [0, 1, 4, 9, 16] and y["idx"][2].tolist() == [2, 1, 3, 0, 4]
    assert y["gap5"][2] > 0.99 and y["ratio"][0] == np.inf and y["aniso"][0] == 1.0 and y["sign_gap"][0] == 1.0
    assert not er.line_table(X[:4], 10.0, 3.0)["line"].any()


# ------------------------------------------------------------------------------- association
def test_association_fallback_cases_are_what_they_claim():
    """on the yardstick alone: edge_big_last's last edge cloud is above the LDS cap with the real
    lines from index 4100 on and all its correspondences kept; the edge_pair cases form a launch of
    their own whose last pair has no last edge point and sixty current ones"""
    cases = [c for c in rc.solve_cases() if c.family == "edge"]
    for solver in (rc.LM, rc.GN):
        mine = [c for c in cases if c.solver == solver]
        big = next(c for c in mine if c.name.startswith("edge_big_last"))
        y = rc.yardstick(big)
        assert rc.admit(big, y) == [] and len(big.edges[0]) > rc.edge_lds_cap()
        assert np.nonzero(big.edges[2])[0].min() >= 4100 and len(y["edges"][0]) == 60
        same = [c for c in mine if c.max_iter == big.max_iter]
        assert max(len(c.edges[0]) for c in same if c is not big) < rc.edge_lds_cap()       # both paths in one launch
        pair = [c for c in mine if c.max_iter == rc.ITERS[solver] + 1]
        assert [c.name.rsplit("_", 1)[0] for c in pair] == ["edge_pair_first", "edge_pair_empty_last"]
        ye = rc.yardstick(pair[1])
        assert rc.admit(pair[1], ye) == [] and rc.admit(pair[0], rc.yardstick(pair[0])) == []
        assert len(pair[1].edges[0]) == 0 and len(pair[1].edges[3]) == 60 and len(ye["edges"][0]) == 0
        assert len(rc.yardstick(pair[0])["edges"][0]) == 60 and len(ye["po"]) > 100

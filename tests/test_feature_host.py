"""The CPU oracle's feature stage and voxel grid against the numpy yardstick
(tests/feature_reference.py, written from src/frameFeature.cpp:45-123 and PCL 1.10's VoxelGrid,
independent of oracle/ and of the kernels), on the cases of tests/feature_cases.py.

Bar: bit equality.  Both evaluate the source's float expressions in the written order, one
rounding per operation.  Curvature is compared as uint32 where the yardstick's value is not NaN
and NaN-for-NaN where it is (NaN bit patterns differ between machines).

Also here: the cases are checked for what they claim to hold, every deliberately wrong rule of
the yardstick is shown to change the output of a named case, and the yardstick itself is held
to a few answers computed by hand.
"""
import numpy as np
import pytest

import feature_cases as fc
import feature_reference as ref

F32 = np.float32


def bits_equal(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def curvature_equal(got, want):
    """uint32 equality where the yardstick is not NaN, NaN where it is"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all()) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def seen_cloud(pts, keep):
    """what the stage is to extract from: the kept points' x, y, z"""
    return np.ascontiguousarray((pts if keep is None else pts[keep != 0])[:, :3])


def _check_oracle(O, cloud, n_rows, what):
    y = ref.extract_planes(cloud, n_rows)
    for chain in ("float", "double"):
        with O.ring_chain(chain):
            rx, off, src, rid = O.bin_rings(cloud, n_rows)
        assert np.array_equal(rid.astype(np.int64), y["ids"]), (what, chain, "ring ids")
        assert np.array_equal(off, y["off"]), (what, chain, "row offsets")
        assert np.array_equal(src, y["src"]), (what, chain, "partition order")
        assert bits_equal(rx, y["rx"]), (what, chain, "ring cloud")
    cv = O.curvature(y["rx"], y["off"], n_rows)
    assert curvature_equal(cv, y["cv"]), (what, "curvature")
    pl, sel = O.select(y["rx"], cv, y["off"], n_rows)
    assert np.array_equal(sel, y["sel"]), (what, "selected positions")
    assert bits_equal(pl, y["planes"]), (what, "plane list")
    assert bits_equal(O.extract_planes(cloud, n_rows), y["planes"]), (what, "extract_planes")


@pytest.mark.parametrize("layout", fc.LAYOUTS)
@pytest.mark.parametrize("n_rows", [16, 64])
def test_oracle_equals_yardstick(oracle, n_rows, layout):
    for cs in fc.cases(n_rows):
        pts, keep = fc.layout(cs, layout)
        _check_oracle(oracle, seen_cloud(pts, keep), n_rows, (cs.name, n_rows, layout))


@pytest.mark.parametrize("n_rows", [16, 64])
def test_oracle_equals_yardstick_padded_past_the_single_read_capacity(oracle, n_rows):
    dense = next(c for c in fc.cases(n_rows) if c.name == "dense")
    cloud = fc.binned(dense)
    assert len(cloud) > fc.BINNED_POINTS
    y = ref.extract_planes(cloud, n_rows)
    assert bits_equal(y["planes"], ref.extract_planes(dense.pts, n_rows)["planes"])   # NaN points: dropped
    rx, off, src, rid = oracle.bin_rings(cloud, n_rows)
    assert np.array_equal(off, y["off"]) and np.array_equal(src, y["src"]) and bits_equal(rx, y["rx"])
    assert bits_equal(oracle.extract_planes(cloud, n_rows), y["planes"])


@pytest.mark.parametrize("leaf", fc.VOXEL_LEAVES)
def test_oracle_voxel_grid_equals_yardstick(oracle, leaf):
    for name, cl in fc.voxel_clouds().items():
        want = ref.voxel_grid(cl, leaf)
        got = oracle.voxel_grid(cl, leaf) if len(cl) else np.zeros((0, 4), F32)
        assert bits_equal(got, want), (name, leaf, got.shape, want.shape)
    assert bits_equal(oracle.voxel_grid(fc.PASSTHROUGH, leaf), ref.voxel_grid(fc.PASSTHROUGH, leaf))


# ------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("n_rows", [16, 64])
def test_cases_cover_what_they_claim(n_rows):
    cases = {c.name: c for c in fc.cases(n_rows)}
    pr = ref.PROFILES[n_rows]
    rows_in = fc.in_range(n_rows)
    pm = F32(pr["plane_min"])
    # every finite kept point is clear of the bin edges, in every layout (a layout only reorders;
    # the masked one is checked on the points it keeps).  One kind of point cannot have a margin:
    # where x*x + y*y overflows float the ratio is z / inf = 0 and the angle the exact 0 in every
    # precision; for 16 rows (0 + 15) / 2 + 0.5 is the integer 8, an int() edge.  No rounding
    # happens on that path, so those points are held to angle == 0 exactly instead.
    for cs in cases.values():
        for which in fc.LAYOUTS:
            pts, keep = fc.layout(cs, which)
            cloud = seen_cloud(pts, keep)
            ids, margin = ref.ring_ids(cloud, n_rows)
            finite = np.isfinite(cloud).all(1) & (ids >= 0)
            with np.errstate(over="ignore"):
                overflow = np.isinf(cloud[:, 0] * cloud[:, 0] + cloud[:, 1] * cloud[:, 1])
            assert (margin[finite & ~overflow] >= 1e-3).all(), (cs.name, which, margin[finite & ~overflow].min())
            assert (ids[finite & overflow] == fc.ZERO_ROW[n_rows]).all()
            if which == "rowmajor":
                assert np.array_equal(ids[ids >= 0], cs.run[ids >= 0]), cs.name     # built into its row
    # lengths: every length in an in-range row; 64 rows: flat populated rows just outside the range
    have = set()
    for name in [n for n in cases if n.startswith("lengths")]:
        y = ref.extract_planes(cases[name].pts, n_rows)
        have |= {int(y["off"][r + 1] - y["off"][r]) for r in rows_in}
        assert y["off"][rows_in[0] + 1] > y["off"][rows_in[0]] and y["off"][rows_in[-1] + 1] > y["off"][rows_in[-1]]
        if n_rows == 64:
            wide = ref.extract_planes(cases[name].pts, n_rows, row_lo=-2, row_hi=2)
            for r in (3, 4, 59, 60):
                assert y["off"][r + 1] - y["off"][r] == 40
                assert np.count_nonzero((wide["sel"] >= wide["off"][r]) & (wide["sel"] < wide["off"][r + 1])) == 2
    assert have >= set(fc.row_lengths(n_rows)) >= {0, 1, 10, 11, 12, pr["span"], 64}
    # threshold: planeMin, the float below and the float above, at the index the greedy rule tests
    y = ref.extract_planes(cases["threshold"].pts, n_rows)
    tg = fc.threshold_targets(n_rows)
    c = fc.centre_index(n_rows)
    seen = {k: 0 for k in tg}
    for r in rows_in:
        v = y["cv"][y["off"][r] + c]
        taken = bool(np.isin(y["off"][r] + c, y["sel"]))
        for k, t in tg.items():
            if v.view(np.uint32) == t.view(np.uint32):
                seen[k] += 1
                assert taken == (k == "below"), (r, k)
    assert all(seen.values()), seen
    assert tg["below"] < pm < tg["above"] and tg["equal"] == pm
    # dense: the share of candidates, the row sizes
    for name in ("dense", "dense_equal"):
        assert 0.40 <= fc.candidate_share(cases[name]) <= 0.70, name
    y = ref.extract_planes(cases["dense"].pts, n_rows)
    assert {300, 2049, 4097} <= {int(y["off"][r + 1] - y["off"][r]) for r in rows_in}
    # nonfinite: NaN and inf curvature in an in-range row, in every layout; never selected
    zr = fc.ZERO_ROW[n_rows]
    assert zr in rows_in
    for which in fc.LAYOUTS:
        pts, keep = fc.layout(cases["nonfinite"], which)
        y = ref.extract_planes(seen_cloud(pts, keep), n_rows)
        v = y["cv"][y["off"][zr]:y["off"][zr + 1]]
        assert np.isnan(v).any() and np.isinf(v).any(), which
        assert np.isfinite(y["cv"][y["sel"]]).all()
        assert np.isinf(y["rx"][:, :3]).any() and not np.isnan(y["rx"]).any()      # inf kept, NaN dropped
    # equal rows where claimed
    for cs in cases.values():
        if cs.equal_rows:
            assert len(set(np.bincount(cs.run, minlength=n_rows).tolist())) == 1, cs.name


def test_voxel_cases_cover_what_they_claim():
    cl = fc.voxel_clouds()
    for leaf in fc.VOXEL_LEAVES:
        assert ref.voxel_passthrough(fc.PASSTHROUGH, leaf)
        assert bits_equal(ref.voxel_grid(fc.PASSTHROUGH, leaf), fc.PASSTHROUGH)
        assert not any(ref.voxel_passthrough(c, leaf) for c in cl.values())
        assert len(ref.voxel_grid(cl["one_voxel_700"], leaf)) == 1
        assert len(ref.voxel_grid(cl["adjacent_a"], leaf)) == 1
        assert len(ref.voxel_grid(cl["one_point"], leaf)) == 1
        assert len(ref.voxel_grid(cl["duplicates"], leaf)) <= 50
        assert len(ref.voxel_grid(cl["empty"], leaf)) == 0
        b = cl["adjacent_b"]                     # its first voxel is index 0: it holds the corner point
        assert np.array_equal(np.floor(b[0, :3] * (F32(1) / F32(leaf))), np.floor(b[:, :3].min(0) * (F32(1) / F32(leaf))))
    lat = cl["lattice"]
    assert (lat[:, :3] < 0).any() and (lat[:, :3] > 0).any()
    assert len(cl["one_voxel_700"]) > 2 * 256
    assert set(fc.VOXEL_BATCHES) == {1, 2, 3, 4, 5, 8, 9}
    for names in fc.VOXEL_BATCHES.values():
        if "adjacent_a" in names:
            assert names[names.index("adjacent_a") + 1] == "adjacent_b"


# ------------------------------------------------------------------------------- the wrong rules
def _cases_that_differ(kw, field):
    return [(cs.name, n_rows) for n_rows in (64, 16) for cs in fc.cases(n_rows)
            if not bits_equal(ref.extract_planes(cs.pts, n_rows, **kw)[field],
                              ref.extract_planes(cs.pts, n_rows)[field])]


@pytest.mark.parametrize("variant", list(ref.FEATURE_VARIANTS))
def test_wrong_feature_rule_changes_a_plane_list(variant):
    """Each wrong rule must change the plane list of some case; the case is printed.
    One rule cannot: with the intensity summed in float32, float(j) + float(row / 100.0) differs
    from float(j + row / 100.0) only for 16 (row, j) pairs of the 64-row profile, all with j <= 7
    and j >= 1 (enumerated below for every row and j < 5000), and no such point is ever in a plane
    list: j = 0 has value 0, is always taken, and the next pick is at j >= span.  That rule is held
    to the ring-ordered cloud instead, which the device tests compare bit for bit as well."""
    kw = ref.FEATURE_VARIANTS[variant]
    field = "planes"
    if variant == "intensity summed in float32":
        for n_rows in (16, 64):
            j, row = np.arange(5000)[None, :], np.arange(n_rows)[:, None]
            r, jj = np.nonzero((j + row / 100.0).astype(F32) != j.astype(F32) + (row / 100.0).astype(F32))
            assert jj.size == (16 if n_rows == 64 else 0)
            assert jj.size == 0 or (1 <= jj.min() and jj.max() <= 7 < ref.PROFILES[n_rows]["span"])
        assert not _cases_that_differ(kw, "planes")
        field = "rx"
    hit = _cases_that_differ(kw, field)
    print(f"{variant}: caught by {hit}")
    assert hit, f"no case distinguishes the rule {variant!r}: a case is missing"


@pytest.mark.parametrize("variant", list(ref.VOXEL_VARIANTS))
def test_wrong_voxel_rule_changes_an_output(variant):
    kw = ref.VOXEL_VARIANTS[variant]
    hit = [(name, leaf) for leaf in fc.VOXEL_LEAVES for name, cl in fc.voxel_clouds().items()
           if not bits_equal(ref.voxel_grid(cl, leaf, **kw), ref.voxel_grid(cl, leaf))]
    print(f"{variant}: caught by {hit}")
    assert hit, f"no cloud distinguishes the rule {variant!r}: a case is missing"


# ------------------------------------------------------------------------------- by hand
def _arc(n_rows, row, n):
    return fc.flat_row(n_rows, row, n)


def test_yardstick_64_rows_skips_row_4_and_takes_row_5_every_25():
    """frameFeature.cpp:147-152: rows 0-4 and 59-63 are skipped, planeSpan is 25.  Smooth 60-point
    arcs in rows 4, 5, 58 and 59: every value is tiny, so rows 5 and 58 give j = 0, 25, 50 and the
    others nothing.  intensity = j + row / 100."""
    pts = np.concatenate([_arc(64, r, 60) for r in (4, 5, 58, 59)])
    y = ref.extract_planes(pts, 64)
    assert y["off"][[4, 5, 6, 58, 59, 60]].tolist() == [0, 60, 120, 120, 180, 240]
    assert (y["cv"][:60] == 0).all() and (y["cv"][180:] == 0).all()             # out of range: never computed
    assert (y["cv"][65:115] > 0).all() and (y["cv"][65:115] < 1e-4).all()
    assert (y["cv"][60:65] == 0).all() and (y["cv"][115:120] == 0).all()
    assert y["sel"].tolist() == [60, 85, 110, 120, 145, 170]
    assert np.allclose(y["planes"][:, 3], [0.05, 25.05, 50.05, 0.58, 25.58, 50.58], rtol=0, atol=4e-6)
    assert bits_equal(y["planes"][:, :3], pts[[60, 85, 110, 120, 145, 170]])


def test_yardstick_16_rows_by_hand():
    """a row of 12 collinear points 1 m apart with the sixth moved by 0.1 m: value at j = 5 is
    (10 * 0.1)^2 = 1 > 0.05, at j = 6 (0.1)^2 = 0.01 < 0.05; picks j = 0, 3, 6, 9 (span 3)"""
    pts = np.zeros((12, 3))                                                    # 1 deg up: row 8
    pts[:, 1] = np.arange(12) - 5.5
    pts[:, 0] = 40.0
    pts[5, 0] += 0.1
    pts[:, 2] = 0.7
    ids, _ = ref.ring_ids(pts, 16)
    assert (ids == 8).all()
    y = ref.extract_planes(pts.astype(F32), 16)
    assert y["cv"][5] == pytest.approx(1.0, rel=1e-3) and y["cv"][6] == pytest.approx(0.01, rel=2e-2)
    assert (y["cv"][:5] == 0).all() and (y["cv"][7:] == 0).all()
    assert y["sel"].tolist() == [0, 3, 6, 9]
    assert np.allclose(y["planes"][:, 3], [0.08, 3.08, 6.08, 9.08], rtol=0, atol=1e-6)


def test_yardstick_ring_ids_by_hand():
    """int() truncates; -1 < id < N; a NaN angle drops the point; an overflowed x*x gives angle 0"""
    t = lambda deg: float(np.tan(np.radians(deg)))                             # noqa: E731
    pts = np.array([[1, 0, t(2.0)], [1, 0, t(-8.0)], [1, 0, t(-9.33)], [1, 0, t(-24.33)], [1, 0, t(2.3)],
                    [1, 0, t(-25.0)], [0, 0, 0], [np.nan, 1, 1], [3e19, 0, 5], [0, 0, 1]], F32)
    ids, margin = ref.ring_ids(pts, 64)
    # (2 - 2) * 3 + .5 -> 0;  (2 + 8) * 3 + .5 = 30.5 -> 30;  32 + int(0.5 * 2 + .5) = 33;
    # 32 + int(15.5 * 2 + .5) = 63;  (2 - 2.3) * 3 + .5 = -0.4 -> int() gives 0, not -1;
    # 32 + int(16.17 * 2 + .5) = 64 -> dropped;  0 / 0, NaN -> dropped;  angle 0 -> row 6;  90 deg -> dropped
    assert ids.tolist() == [0, 30, 33, 63, 0, -1, -1, -1, 6, -1]
    assert np.isnan(margin[6]) and np.isnan(margin[7]) and margin[1] == pytest.approx(1 / 6, abs=1e-4)
    ids16, _ = ref.ring_ids(np.array([[1, 0, t(-15)], [1, 0, t(15)], [1, 0, t(-16.5)], [1, 0, t(16.5)],
                                      [3e19, 0, 5]], F32), 16)
    # -16.5: (-1.5) / 2 + .5 = -0.25 -> int() 0;  16.5: 31.5 / 2 + .5 = 16.25 -> 16, dropped
    assert ids16.tolist() == [0, 15, 0, -1, 8]


def test_yardstick_voxel_grid_by_hand():
    """leaf 0.1 (1 / 0.1f is 10.0f): floor(-0.5) = -1, so the two negative-x points share voxel
    (-1, 0, 0) and come first; the third is voxel (0, 0, 0).  Truncation would merge all three."""
    cl = np.array([[0.05, 0.05, 0.05, 5.0], [-0.05, 0.05, 0.05, 1.0], [-0.07, 0.03, 0.01, 3.0]], F32)
    assert F32(1) / F32(0.1) == F32(10)
    out = ref.voxel_grid(cl, 0.1)
    assert out.shape == (2, 4)
    assert np.allclose(out, [[-0.06, 0.04, 0.03, 2.0], [0.05, 0.05, 0.05, 5.0]], rtol=0, atol=1e-7)
    assert bits_equal(out[0], (cl[1] + cl[2]) / F32(2)) and bits_equal(out[1], cl[0])
    assert ref.voxel_grid(cl, 0.1, truncate=True).shape == (1, 4)
    # a voxel index with all three axes: 2 x 3 x 2 voxels, points given in descending index
    g = np.array([[0.15, 0.25, 0.15, 1], [0.05, 0.25, 0.15, 2], [0.15, 0.05, 0.15, 3], [0.15, 0.25, 0.05, 4],
                  [0.05, 0.05, 0.05, 5]], F32)
    assert ref.voxel_grid(g, 0.1)[:, 3].tolist() == [5, 4, 3, 2, 1]           # 0, 5, 7, 10, 11

"""The association cases of tests/assoc_cases.py on the CPU: every case admitted on the yardstick
alone, the CPU oracle's 1-NN (orc_correspond) and the shortlisting yardstick (associate) against
the all-pairs one (associate_exact), the tie family's lowest-index rule found a second way, and
the launch plan of every shape tests/test_gpu_assoc_yardstick.py sends to the device."""
import numpy as np
import pytest

import assoc_cases as ac
import registration_reference as ref


def _all():
    return ac.cases() + (ac.hole_big(), ac.hole_dense())


def test_every_case_is_admitted(capsys):
    worst = (0, 1, 0, "")
    for cs in _all():
        assert ac.admit(cs) == [], cs.name
        n = cs.note
        if n["redrawn"] * worst[1] > worst[0] * n["nq"]:
            worst = (n["redrawn"], n["nq"], n["rounds"], cs.name)
        assert len(cs.last) > 10 and np.abs(cs.last[:, :3]).max() < ac.BOX and np.abs(cs.curr[:, :3]).max() < ac.BOX
        assert 0.15 < 1.0 - cs.valid.mean() < 0.45 or len(cs.last) < 100, cs.name      # ~30 % zeros
        assert np.abs(np.linalg.norm(cs.normal, axis=1) - 1.0).max() < 1e-6, cs.name
    assert {c.family for c in ac.cases()} == set(ac.FAMILIES)
    assert len(ac.hole_big().curr) > 1024 and len(ac.hole_dense().last) > ac.SOA_MAX
    with capsys.disabled():
        print(f"\n  most redraws: {worst[0]} of {worst[1]} queries in {worst[2]} rounds ({worst[3]}); "
              f"rounds at most {max(c.note['rounds'] for c in _all())}")


def test_level_cases_reach_their_levels():
    """level_R: every 1-NN within 3 % of 0.98 R or 1.02 R, both present; the y extent of R <= 64
    under 255 m (the narrowest strips), wider above"""
    for cs in ac.family("levels"):
        R = float(cs.name.split("_")[1])
        y = ac.yardstick(cs)
        s = ref.transform_to_last(cs.curr[:, :3], cs.pose0[:4], cs.pose0[4:]).astype(np.float64)
        d = np.sqrt(((s - cs.last[y["nn"], :3]) ** 2).sum(1)) / R
        assert np.all((np.abs(d - 0.98) < 0.03) | (np.abs(d - 1.02) < 0.03)), cs.name
        assert (d < 1.0).sum() == (32 if R <= 32 else 16) and (d > 1.0).sum() == 16, cs.name      # R <= 32: three cells
        assert (ac.solve_compared(cs) == "") == (R <= 32), (cs.name, ac.solve_compared(cs))
        assert (np.ptp(cs.last[:, 1]) < 255.0) == (R <= 64), cs.name


def _strips(cs):
    """the strip layout of the finished last cloud, and the strips of every query and of its 1-NN"""
    geo = ac.strip_geometry(cs.last[:, 1])
    s = ref.transform_to_last(cs.curr[:, :3], cs.pose0[:4], cs.pose0[4:])
    return geo, ac.strip_of(s[:, 1], geo), ac.strip_of(cs.last[ac.yardstick(cs)["nn"], 1], geo), s


def test_boundary_cases_sit_on_the_boundaries_of_the_finished_cloud():
    """The layout constants are the library's, and the cases built on a strip layout are checked
    against the layout of the cloud that is sent.  y30km: 30 km of extent, every 1-NN in the strip
    next to its query's, the boundary points the lowest / highest float32 y of their strips, at the
    far end.  strip_edges: y0 = -20, W = fl(1.001), every last point on y0 + k W."""
    from ssf import _abi
    assert (ac.IMAGE_MIN, ac.IMAGE_MAX) == (_abi.STRIP_IMAGE_MIN, _abi.STRIP_IMAGE_MAX)
    cs = next(c for c in ac.cases() if c.name == "y30km")
    geo, sq, sn, s = _strips(cs)
    assert float(geo[0]) == -15000.0 and float(cs.last[:, 1].max()) == 15000.0 and geo[3] >= ac.STRIP_MAX - 1
    assert abs(float(geo[1]) - 30000.0 / (ac.STRIP_MAX - 1)) < 1e-4
    assert np.all(np.abs(sq - sn) == 1), np.flatnonzero(np.abs(sq - sn) != 1)
    assert (sn > sq).sum() == (sn < sq).sum() == ac.Y30_FAR and min(sq.min(), sn.min()) >= geo[3] - 3 - ac.Y30_FAR
    py = cs.last[ac.yardstick(cs)["nn"], 1]
    up = sn > sq
    assert np.all(ac.strip_of(np.nextafter(py[up], np.float32(-np.inf)), geo) == sn[up] - 1)       # the lowest y of its strip
    assert np.all(ac.strip_of(np.nextafter(py[~up], np.float32(np.inf)), geo) == sn[~up] + 1)      # the highest y of its strip
    d = np.abs(s[:, 1].astype(np.float64) - py)
    assert d.min() >= 0.99 and d.max() <= 2.0
    cs, = ac.family("edges")
    geo, sq, sn, s = _strips(cs)
    assert float(geo[0]) == -20.0 and geo[1] == ac.STRIP_W and geo[3] in (39, 40)
    edges = np.array([ac.nominal_edge(k, geo) for k in range(40)])
    assert np.all(np.isin(cs.last[:, 1], edges)) and np.all(np.isin(edges, cs.last[:, 1]))
    assert np.isin(s[:, 1], edges).sum() >= 40 and (s[:, 1] < edges[0] - 200).any() and (s[:, 1] > edges[-1] + 200).any()
    assert (sq != sn).sum() >= 20                                      # 1-NNs across a boundary


def test_oracle_equals_exact(oracle):
    for cs in _all():
        got = oracle.correspond(cs.last, cs.curr, cs.pose0[:4], cs.pose0[4:])
        assert np.array_equal(got, ac.yardstick(cs)["nn"]), cs.name


def test_shortlist_yardstick_equals_exact_off_ties():
    for cs in _all():
        y = ac.yardstick(cs)
        nn, _, keep = ref.associate(cs.last, cs.curr, cs.pose0[:4], cs.pose0[4:], cs.valid)
        clear = y["gap"] >= ac.GAP
        assert np.array_equal(nn[clear], y["nn"][clear]) and np.array_equal(keep[clear], y["keep"][clear]), cs.name
        assert cs.note["tie"] or clear.all(), cs.name


def test_ties_go_to_the_lowest_index():
    cs, = ac.family("ties")
    y = ac.yardstick(cs)
    assert np.all(y["gap"] == 0.0)
    L = cs.last[:, :3].astype(np.float64)
    s = ref.transform_to_last(cs.curr[:, :3], cs.pose0[:4], cs.pose0[4:]).astype(np.float64)
    ways = set()
    for i, x in enumerate(s):
        d2 = ((x - L) ** 2).sum(1)
        tied = np.flatnonzero(d2 == d2.min())
        assert y["nn"][i] == tied[0] and len(tied) >= 2, i
        ways.add(len(tied))
        assert np.array_equal(x, np.round(2 * x) / 2)                  # halves: exact in float32
    assert {2, 4, 8} <= ways, ways
    # tied candidates that become reachable (dx^2 + dy^2 <= R^2) at different levels; the winner
    # (lowest index) is sometimes the one found first, sometimes the one found later
    first = later = 0
    for i, x in enumerate(s):
        d2 = ((x - L) ** 2).sum(1)
        tied = np.flatnonzero(d2 == d2.min())
        lv = [ac.first_level(((x - L[k])[:2] ** 2).sum()) for k in tied]
        if len(set(lv)) > 1:
            assert lv[0] in (min(lv), max(lv)) and d2.min() > min(lv) ** 2     # not settled at the first level
            first += lv[0] == min(lv)
            later += lv[0] == max(lv)
    assert first >= 4 and later >= 4 and first + later == 4 * len(ac.CROSS), (first, later)


@pytest.mark.parametrize("name", ac.FAMILIES + ("global", "all129"))
def test_launch_shapes_take_their_paths(name):
    """ssf.register_plan (host arithmetic) names the intended path for every launch shape"""
    import ssf
    if name == "global":
        rows = ac.global_rows()
        assert all(len(r[1][0].last) > ac.SOA_MAX for r in rows)
    elif name == "all129":
        rows = [("all129", ac.tile(list(ac.cases()), 129), "sorted", 1024,
                 dict(strip_path=True, group_mode=False, qsplit=1, compacted=True))]
    else:
        rows = ac.rows(name)
        assert any(len(c.curr) > 1024 for r in rows for c in r[1]) == (name == "hole")
    for row, cases, mode, bound, want in rows:
        P, b = len(cases), ac.bound_of(cases, bound)
        assert all(max(len(c.last), len(c.curr)) <= b for c in cases), row
        ac.check_plan(ssf.register_plan(P, b), want, (name, row))
        if row.startswith("group"):
            assert P <= 16
        if row.startswith("lane"):
            assert P >= 17 and (row != "lane_split" or P <= 32)
        if row == "group_image":
            assert ac.IMAGE_MIN <= b <= ac.IMAGE_MAX, (row, b)

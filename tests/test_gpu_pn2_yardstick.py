"""The TFlow point-set operators on the device (csrc/pointnet2.hip through ssf.pointnet2) against
the numpy yardstick tests/pn2_reference.py -- not against the oracle -- on the cases of
tests/pn2_cases.py: the four FPS kernels, both k-NN launch families at every list length, tile
and wave-slice edges, odd tails, ties, denormal and infinite d2, k > n, the LDS and global
gathers on both sides of n = 36864, bad indices, both upsample families and s < k.

Bars, as in tests/test_pn2_host.py: bit equality with the float32 layer for every output; then,
as a second assertion, the float64 layer's: on every decisive (query, rank) pair (gap > 2^-20)
the device's index is the float64 one, interpolation within 3u sum|w f| and upsample within
(2k + 9)u sum|w f| of the float64 value (derived in the yardstick's docstring).
"""
import numpy as np
import pytest
import torch

import pn2_cases as pc
import pn2_reference as ref

pytestmark = pytest.mark.gpu

same = pc.bits_equal


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("cs", pc.fps_cases(), ids=lambda c: c.name)
def test_fps_equals_yardstick(dev, cs):
    from ssf import pointnet2 as P
    y = pc.fps_yard(cs.name)
    got = _n(P.furthest_point_sample(_t(cs.xyz, dev), cs.npoint, start=_t(cs.start, dev)))
    assert same(got, y), (cs.name, np.argwhere(got != y)[:4].tolist())
    if not cs.exact:
        want, gap = ref.fps64(cs.xyz, got, cs.start)
        dec = gap > ref.GAP_BAR
        assert np.array_equal(got[dec], want[dec]), cs.name


@pytest.mark.parametrize("cs", pc.knn_cases(), ids=lambda c: c.name)
def test_knn_equals_yardstick(dev, cs):
    from ssf import pointnet2 as P
    yd, yi = pc.knn_yard(cs.name)
    q, r = _t(cs.query, dev), _t(cs.ref, dev)
    for k in cs.ks:
        d, i = P.knn(k, q, r)
        d, i = _n(d), _n(i)
        assert same(i, np.ascontiguousarray(yi[..., :k])), (cs.name, k, np.argwhere(i != yi[..., :k])[:4].tolist())
        assert same(d, np.ascontiguousarray(yd[..., :k])), (cs.name, k)
        if not cs.exact:
            i64, gap = pc.knn_yard64(cs.name)
            assert ref.check_decisive(i, i64[..., :k], gap[..., :k])[0] == 0, (cs.name, k)
    d3, i3 = P.three_nn(q, r)                                   # three_nn is the k = 3 rows
    assert same(_n(i3), np.ascontiguousarray(yi[..., :3])) and same(_n(d3), np.ascontiguousarray(yd[..., :3]))


@pytest.mark.parametrize("cs", pc.gather_cases(), ids=lambda c: c.name)
def test_gather_and_group_equal_yardstick(dev, cs):
    from ssf import pointnet2 as P
    op = P.gather_operation if cs.idx.ndim == 2 else P.grouping_operation
    feat, n = _t(cs.feat, dev), cs.feat.shape[2]
    assert same(_n(op(feat, _t(cs.idx, dev), check=True)), ref.gather(cs.feat, cs.idx)[0])
    for which in pc.BAD_INDICES:
        ix = pc.with_bad(cs.idx, n, which)[0]
        with pytest.raises(ValueError):
            op(feat, _t(ix, dev), check=True)
        assert same(_n(op(feat, _t(ix, dev), check=False)), ref.gather(cs.feat, ix)[0]), (cs.name, which)


@pytest.mark.parametrize("cs", pc.rel_cases(), ids=lambda c: c.name)
def test_group_relative_equals_yardstick(dev, cs):
    from ssf import pointnet2 as P
    x, nx, f = _t(cs.xyz, dev), _t(cs.new_xyz, dev), _t(cs.points, dev)
    got = _n(P.group_relative(x, nx, f, _t(cs.idx, dev), check=True))
    assert same(got, ref.group_relative(cs.xyz, cs.new_xyz, cs.points, cs.idx)[0])
    for which in pc.BAD_INDICES:
        ix = pc.with_bad(cs.idx, cs.xyz.shape[2], which)[0]
        with pytest.raises(ValueError):
            P.group_relative(x, nx, f, _t(ix, dev), check=True)
        got = _n(P.group_relative(x, nx, f, _t(ix, dev), check=False))
        assert same(got, ref.group_relative(cs.xyz, cs.new_xyz, cs.points, ix)[0]), (cs.name, which)


def test_group_relative_rejects_rows_past_the_lds_limit(dev):
    from ssf import pointnet2 as P
    x = torch.zeros((1, 3, pc.STAGE + 1), device=dev)
    with pytest.raises(ValueError):
        P.group_relative(x, x[:, :, :4].contiguous(), None, torch.zeros((1, 4, 2), dtype=torch.int32, device=dev))


@pytest.mark.parametrize("cs", pc.interp_cases(), ids=lambda c: c.name)
def test_three_interpolate_equals_yardstick(dev, cs, capsys):
    from ssf import pointnet2 as P
    feat, w, m = _t(cs.feat, dev), _t(cs.weight, dev), cs.feat.shape[2]
    for which in (None,) + pc.BAD_INDICES:
        ix = cs.idx if which is None else pc.with_bad(cs.idx, m, which)[0]
        if which is not None:
            with pytest.raises(ValueError):
                P.three_interpolate(feat, _t(ix, dev), w, check=True)
        got = _n(P.three_interpolate(feat, _t(ix, dev), w, check=which is None))
        assert same(got, ref.three_interpolate(cs.feat, ix, cs.weight)[0]), (cs.name, which)
        worst = pc.worst_ratio(got, *ref.three_interpolate64(cs.feat, ix, cs.weight))
        assert worst <= 1.0, (cs.name, which, worst)
    with capsys.disabled():
        print(f"\n  {cs.name}: worst device |f32 - f64| / (3u sum|w f|) = {worst:.3f}")


@pytest.mark.parametrize("cs", pc.up_cases(), ids=lambda c: c.name)
def test_upsample_equals_yardstick(dev, cs, capsys):
    from ssf import pointnet2 as P
    x, sx, sf = _t(cs.xyz, dev), _t(cs.sxyz, dev), _t(cs.sfeat, dev)
    worst = {}
    for k in cs.ks:
        y, y64, bound = pc.up_yard(cs.name, k)
        got = _n(P.upsample_flow(x, sx, sf, k=k))
        assert same(got, y), (cs.name, k)
        worst[k] = pc.worst_ratio(got, y64, bound)
        assert worst[k] <= 1.0, (cs.name, k, worst[k])
    with capsys.disabled():
        print(f"\n  {cs.name}: worst device |f32 - f64| / ((2k+9)u sum|w f|) per k = "
              + ", ".join(f"{k}: {w:.3f}" for k, w in worst.items()))


def test_upsample_rejects_more_than_4096_sparse_points(dev):
    from ssf import pointnet2 as P
    x = torch.zeros((1, 3, 4), device=dev)
    with pytest.raises(ValueError):
        P.upsample_flow(x, torch.zeros((1, 3, 4097), device=dev), torch.zeros((1, 1, 4097), device=dev), k=3)

"""The TFlow cost volume on the GPU: the three kernels of csrc/cost_volume.hip
(ssf_pn2_grouped_mlp, ssf_pn2_pair_attention, ssf_pn2_segment_softmax_sum), ssf.tflow's
cost_volume / CostVolume / PointWarping and the whole TFlow, against the reference's own modules
(tests/golden/cv_ref.npz, tflow_ref.npz) and the numpy float64 yardstick (tests/cv_reference.py).

The bar is the one of tests/test_gpu_sa.py: with e_ref = max|ref_f32 - ref_f64| (the float32
rounding of the reference itself on that tensor: the fixture's two runs, or CPU torch in float32
against the yardstick for the cases without a fixture -- never the device's output), the device
must have max|dev - ref_f64| <= 4 e_ref.  The device differs from the reference's float32 run
only in summation order, the BatchNorm fold and expf.  Every test prints its ratio.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cv_reference as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = {
    "A": dict(nsample=8, in_channel=12, sf_channel=10, mlp=[16, 16], flow_mlp=[16, 16], use_flow=True),
    "B": dict(nsample=5, in_channel=12, sf_channel=0, mlp=[16, 16], flow_mlp=[16, 16], use_flow=False),
}
FACTOR = 4.0
OUTS = ("cost_fwd", "cost_bwd", "cost", "flow_out")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLD, "cv_ref.npz")))


@pytest.fixture(scope="module")
def tf():
    return dict(np.load(os.path.join(GOLD, "tflow_ref.npz")))


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def state_of(g, prefix=""):
    shapes = [(str(k), tuple(int(d) for d in s.split(",") if d)) for k, s in zip(g[prefix + "keys"], g[prefix + "shapes"])]
    return {k: torch.from_numpy(v) for k, v in R.seed_state(shapes, int(g[prefix + "seed"])).items()}


def hold(name, dev_out, ref32, ref64):
    e_ref = np.abs(ref32.astype(np.float64) - ref64).max()
    e_dev = np.abs(dev_out.astype(np.float64) - ref64).max()
    print(f"[cv parity] {name}: e_ref {e_ref:.3e} e_dev {e_dev:.3e} ratio {e_dev / e_ref:.3f}")
    assert dev_out.shape == ref64.shape, (name, dev_out.shape, ref64.shape)
    assert e_ref > 0
    assert e_dev <= FACTOR * e_ref, (name, e_dev, e_ref)


# ------------------------------------------------------------------------------------------
# the fixture: cost_volume, PointWarping and the CostVolume module

def fixture_module(g, name, dev):
    from ssf import tflow as F
    cv = F.CostVolume(**CASES[name])
    cv.load_state_dict(state_of(g, name + "/"), strict=True)
    return cv.to(dev)


def fixture_inputs(g, name, dev):
    p = name + "/"
    use = CASES[name]["use_flow"]
    return dict(xyz1=_t(g[p + "xyz1"], dev), xyz2=_t(g[p + "xyz2"], dev), points1=_t(g[p + "points1"], dev),
                points2=_t(g[p + "points2"], dev), sf=_t(g[p + "flow"], dev) if use else None,
                sf_feat=_t(g.get(p + "sf_feat"), dev))


@pytest.mark.parametrize("name", ["A", "B"])
def test_cost_volume_and_warping_on_the_fixture(g, dev, name):
    from ssf import tflow as F
    p = name + "/"
    cv, x = fixture_module(g, name, dev), fixture_inputs(g, name, dev)
    with torch.no_grad():
        outs = F.cost_volume(cv.folded(), x["xyz1"], x["xyz2"], x["points1"], x["points2"],
                             _t(g[p + "knn_idx"], dev), _t(g[p + "knn_idxw"], dev), x["sf"], x["sf_feat"])
        warp = F.PointWarping()(x["xyz1"], x["xyz2"], _t(g[p + "flow"], dev), 5 if name == "A" else None)
    for n, got in zip(OUTS, outs):
        hold(f"fixture {name} cost_volume {n}", _n(got), g[p + n], g[p + n + "_f64"])
    hold(f"fixture {name} PointWarping", _n(warp), g[p + "pc2_warp"], g[p + "pc2_warp_f64"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_cost_volume_module_on_the_fixture(g, dev, name):
    p = name + "/"
    cv, x = fixture_module(g, name, dev), fixture_inputs(g, name, dev)
    xyz2w = _t(g[p + "pc2_warp"], dev) if name == "A" else None
    with torch.no_grad():
        idx, idxw = cv.indices(x["xyz1"], x["xyz2"], xyz2w, x["sf"])
        outs = cv(x["xyz1"], x["xyz2"], xyz2w, x["points1"], x["points2"], x["sf"], x["sf_feat"])
    assert np.array_equal(np.sort(_n(idx), -1), np.sort(g[p + "knn_idx"], -1))
    assert np.array_equal(np.sort(_n(idxw), -1), np.sort(g[p + "knn_idxw"], -1))
    for n, got in zip(OUTS, outs):
        hold(f"fixture {name} CostVolume {n}", _n(got), g[p + n], g[p + n + "_f64"])


# ------------------------------------------------------------------------------------------
# grouped_mlp

def make_case(seed, B, N, S, K, c_ctr, c_g, c_d, xyz, outs, slopes):
    """the generators of make_case in test_gpu_sa.py, with the two further segments"""
    rng = np.random.default_rng(seed)
    widths = [c_ctr + c_g + c_d + (3 if xyz else 0)] + list(outs)
    case = dict(
        xyz=rng.uniform(-2, 2, (B, 3, N)).astype(np.float32) if xyz else None,
        new_xyz=rng.uniform(-2, 2, (B, 3, S)).astype(np.float32) if xyz else None,
        feat=rng.standard_normal((B, c_g, N)).astype(np.float32) if c_g else None,
        ctr=rng.standard_normal((B, c_ctr, S)).astype(np.float32) if c_ctr else None,
        dense=rng.standard_normal((B, c_d, S, K)).astype(np.float32) if c_d else None,
        idx=rng.integers(0, N, (B, S, K)).astype(np.int32),
        ws=[(rng.standard_normal((i, o)) / np.sqrt(i)).astype(np.float32) for i, o in zip(widths, widths[1:])],
        scs=[rng.uniform(0.5, 1.5, o).astype(np.float32) for o in widths[1:]],
        shs=[(rng.standard_normal(o) * 0.2).astype(np.float32) for o in widths[1:]],
        slopes=list(slopes), widths=widths)
    return case


SEGS = ("idx", "ctr", "feat", "dense", "xyz", "new_xyz")


def gmlp_yardstick(case, full):
    return R.grouped_mlp(case["ws"], case["scs"], case["shs"], case["slopes"], full=full, **{k: case[k] for k in SEGS})


def gmlp_cpu_f32(case, full):
    """e_ref's float32 side: float32 grouping (exact gathers, one subtraction per coordinate),
    then the layers with CPU torch"""
    B, S, K = case["idx"].shape
    cols = []
    gather = lambda a: np.stack([a[b][:, np.where((case["idx"][b] < 0) | (case["idx"][b] >= a.shape[2]), 0,  # noqa: E731
                                                  case["idx"][b])] for b in range(B)])
    if case["ctr"] is not None:
        cols.append(np.repeat(case["ctr"][:, :, :, None], K, axis=3))
    if case["feat"] is not None:
        cols.append(gather(case["feat"]))
    if case["dense"] is not None:
        cols.append(case["dense"])
    if case["xyz"] is not None:
        cols.append(gather(case["xyz"]) - case["new_xyz"][:, :, :, None])
    x = torch.from_numpy(np.concatenate(cols, axis=1))
    assert x.dtype == torch.float32
    for w, sc, sh, sl in zip(case["ws"], case["scs"], case["shs"], case["slopes"]):
        t = torch.nn.functional.conv2d(x, torch.from_numpy(w).t().contiguous()[:, :, None, None])
        t = t * torch.from_numpy(sc)[None, :, None, None] + torch.from_numpy(sh)[None, :, None, None]
        x = torch.where(t > 0, t, sl * t)
    return (x if full else x.max(-1)[0]).numpy()


def gmlp_device(case, dev, full, sel=slice(None), check=False):
    from ssf import tflow as F
    d = lambda arrs: [_t(a, dev) for a in arrs]  # noqa: E731
    seg = {k: _t(None if case[k] is None else case[k][sel], dev) for k in SEGS}
    y = F.grouped_mlp(d(case["ws"]), d(case["scs"]), d(case["shs"]), case["slopes"], full=full, check=check, **seg)
    torch.cuda.synchronize()
    return y


L01 = (0.1, 0.1)
# (name, N, S, K, c_ctr, c_g, c_d, xyz, output widths, slopes)
GMLP_CASES = [
    ("ctr_alone", 200, 37, 5, 6, 0, 0, False, (33, 17), L01),
    ("feat_alone", 200, 37, 5, 0, 6, 0, False, (33, 17), L01),
    ("dense_alone", 200, 37, 5, 0, 0, 6, False, (33, 17), L01),
    ("xyz_alone", 200, 37, 5, 0, 0, 0, True, (33, 17), L01),
    ("all_four_k1", 200, 37, 1, 4, 5, 6, True, (33, 17), L01),
    ("all_four_k5", 200, 37, 5, 4, 5, 6, True, (33, 17), L01),
    ("all_four_k7", 200, 37, 7, 4, 5, 6, True, (33, 17), L01),
    ("all_four_k16", 200, 37, 16, 4, 5, 6, True, (33, 17), L01),
    ("all_four_k32", 200, 37, 32, 4, 5, 6, True, (33, 17), L01),
    ("s1", 200, 1, 5, 4, 5, 6, True, (33, 17), L01),
    ("9-33-17", 200, 37, 5, 2, 2, 2, True, (33, 17), L01),
    ("9-200-17", 200, 37, 7, 2, 2, 2, True, (200, 17), L01),
    ("515-256-256", 64, 5, 16, 256, 256, 0, True, (256, 256), L01),
    ("slopes_0_0.1_1", 200, 37, 5, 4, 5, 6, True, (33, 17, 9), (0.0, 0.1, 1.0)),
    ("weightnet_form_16-16-8-1", 200, 37, 8, 0, 0, 16, False, (16, 8, 1), (0.0, 0.0, 1.0)),
]


@pytest.mark.parametrize("spec", GMLP_CASES, ids=[c[0] for c in GMLP_CASES])
def test_grouped_mlp_edge_shapes_against_the_yardstick(dev, spec):
    name, N, S, K, c_ctr, c_g, c_d, xyz, outs, slopes = spec
    case = make_case(sum(outs) + K + c_ctr, 3, N, S, K, c_ctr, c_g, c_d, xyz, outs, slopes)
    for full in (False, True):
        got = gmlp_device(case, dev, full, check=True)
        assert got.shape == ((3, outs[-1], S, K) if full else (3, outs[-1], S))
        hold(f"grouped_mlp {name} {'full' if full else 'max'}", _n(got), gmlp_cpu_f32(case, full),
             gmlp_yardstick(case, full))
        alone = gmlp_device(case, dev, full, sel=slice(1, 2))
        assert torch.equal(alone[0], got[1]), "a batch element's bits depend on its batch"
        assert torch.equal(gmlp_device(case, dev, full), got), "two runs differ"


def test_grouped_mlp_equals_grouped_mlp_max(dev):
    """ctr, dense absent, slope 0, max mode: the set-abstraction kernel's arithmetic with the
    (features, direction) row order instead of (direction, features)"""
    from ssf import pointnet2 as P
    case = make_case(5, 3, 200, 37, 16, 0, 32, 0, True, (32, 32, 64), (0.0, 0.0, 0.0))
    d = lambda arrs: [_t(a, dev) for a in arrs]  # noqa: E731
    ref64, ref32 = gmlp_yardstick(case, False), gmlp_cpu_f32(case, False)
    got = _n(gmlp_device(case, dev, False))
    hold("grouped_mlp in grouped_mlp_max's form", got, ref32, ref64)
    w0 = np.concatenate([case["ws"][0][-3:], case["ws"][0][:-3]])      # (direction, features) rows
    other = _n(P.grouped_mlp_max(_t(case["xyz"], dev), _t(case["new_xyz"], dev), _t(case["feat"], dev),
                                 _t(case["idx"], dev), d([w0] + case["ws"][1:]), d(case["scs"]), d(case["shs"])))
    e_ref = np.abs(ref32.astype(np.float64) - ref64).max()
    diff = np.abs(got.astype(np.float64) - other.astype(np.float64)).max()
    print(f"[cv parity] grouped_mlp vs grouped_mlp_max: max diff {diff:.3e} ratio {diff / e_ref:.3f}")
    assert diff <= FACTOR * e_ref


def test_grouped_mlp_write_bounds_and_bad_indices(dev):
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    B, N, S, K = 2, 96, 7, 5
    case = make_case(77, B, N, S, K, 4, 5, 6, True, (33, 17), L01)
    d = lambda arrs: [_t(a, dev) for a in arrs]  # noqa: E731
    ws, scs, shs = d(case["ws"]), d(case["scs"]), d(case["shs"])
    seg = {k: _t(case[k], dev) for k in SEGS}
    ptrs = C.c_void_p * 2
    pad = 1024

    def launch(idx_np, full):
        count = B * 17 * S * (K if full else 1)
        buf = torch.full((pad + count + pad,), -777.0, dtype=torch.float32, device=dev)
        out = buf[pad:pad + count]
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        ix = _t(idx_np, dev)
        rc = _abi.lib().ssf_pn2_grouped_mlp(
            _stream(dev), B, N, S, K, 4, 5, 6, _ptr(seg["ctr"]), _ptr(seg["feat"]), _ptr(seg["dense"]),
            _ptr(seg["xyz"]), _ptr(seg["new_xyz"]), _ptr(ix), 2, (C.c_int32 * 3)(*case["widths"]),
            ptrs(*[_ptr(t) for t in ws]), ptrs(*[_ptr(t) for t in scs]), ptrs(*[_ptr(t) for t in shs]),
            (C.c_float * 2)(0.1, 0.1), int(full), _ptr(out), _ptr(bad))
        torch.cuda.synchronize()
        assert rc == 0, _abi.lib().ssf_pn2_last_error()
        assert bool((buf[:pad] == -777.0).all()) and bool((buf[pad + count:] == -777.0).all())
        assert not bool((out == -777.0).any())
        return _n(out).reshape((B, 17, S, K) if full else (B, 17, S)), int(bad.item())

    broken = dict(case, idx=case["idx"].copy())
    broken["idx"][0, 3, 2] = N
    broken["idx"][1, 6, 4] = -1
    fixed = dict(case, idx=np.where((broken["idx"] < 0) | (broken["idx"] >= N), 0, broken["idx"]).astype(np.int32))
    for full in (False, True):
        got, bad = launch(case["idx"], full)
        assert bad == 0
        hold(f"grouped_mlp bounds, valid indices, full={full}", got, gmlp_cpu_f32(case, full), gmlp_yardstick(case, full))
        got, bad = launch(broken["idx"], full)
        assert bad == 1
        hold(f"grouped_mlp bounds, index n and -1 read as 0, full={full}", got, gmlp_cpu_f32(fixed, full),
             gmlp_yardstick(fixed, full))
    with pytest.raises(ValueError, match="out of range"):
        gmlp_device(broken, dev, False, check=True)


# ------------------------------------------------------------------------------------------
# pair_attention

def attention_cpu_f32(q, kw):
    """soflow.py:420-422, :453-458 with CPU torch on [B, C, S, K] float32 tensors"""
    q, kw = torch.from_numpy(q), torch.from_numpy(kw)
    a = torch.matmul(q.permute(0, 2, 3, 1).contiguous(), kw.permute(0, 2, 1, 3).contiguous())     # [B, S, K, K]
    w = torch.softmax(a, -2) * torch.softmax(a, -1)
    qm = q + torch.matmul(w, kw.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    kwm = kw + torch.matmul(q.permute(0, 2, 1, 3).contiguous(), w).permute(0, 2, 1, 3)
    return qm.numpy(), kwm.numpy()


ATT_CASES = [(1, 1, 1.0), (16, 8, 1.0), (33, 5, 1.0), (256, 16, 0.25), (64, 32, 0.5), (16, 8, 80.0)]


@pytest.mark.parametrize("c,k,spread", ATT_CASES, ids=[f"c{c}_k{k}_logits{s:g}" for c, k, s in ATT_CASES])
def test_pair_attention_against_the_yardstick(dev, c, k, spread):
    """spread: the standard deviation of the logits a[m][m'] (80: only the max-subtraction keeps
    expf finite)"""
    from ssf import tflow as F
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    rng = np.random.default_rng(c * 100 + k)
    B, S = 3, 37
    sigma = np.sqrt(spread / np.sqrt(c))
    q = (rng.standard_normal((B, c, S, k)) * sigma).astype(np.float32)
    kw = (rng.standard_normal((B, c, S, k)) * sigma).astype(np.float32)
    ref64, ref32 = R.pair_attention(q, kw), attention_cpu_f32(q, kw)
    dq, dkw = _t(q, dev), _t(kw, dev)
    got = F.pair_attention(dq, dkw)
    again = F.pair_attention(dq, dkw)
    alone = F.pair_attention(dq[1:2], dkw[1:2])
    torch.cuda.synchronize()
    for n, a, b, al, r32, r64 in zip(("qm", "kwm"), got, again, alone, ref32, ref64):
        assert np.isfinite(_n(a)).all()
        hold(f"pair_attention c={c} k={k} logits~{spread:g} {n}", _n(a), r32, r64)
        assert torch.equal(a, b), "two runs differ"
        assert torch.equal(al[0], a[1]), "a batch element's bits depend on its batch"
    # sentinels around both outputs
    pad, count = 1024, q.size
    bufs = [torch.full((pad + count + pad,), -777.0, dtype=torch.float32, device=dev) for _ in range(2)]
    outs = [b[pad:pad + count] for b in bufs]
    rc = _abi.lib().ssf_pn2_pair_attention(_stream(dev), B, c, S, k, _ptr(dq), _ptr(dkw), _ptr(outs[0]), _ptr(outs[1]))
    torch.cuda.synchronize()
    assert rc == 0, _abi.lib().ssf_pn2_last_error()
    for b, o, a in zip(bufs, outs, got):
        assert bool((b[:pad] == -777.0).all()) and bool((b[pad + count:] == -777.0).all())
        assert torch.equal(o.view_as(a), a)


# ------------------------------------------------------------------------------------------
# segment_softmax_sum

def segment_cpu_f32(logit, val, T, idx_flat):
    """scatter_softmax, the product and scatter_sum (soflow.py:474-481) with CPU torch float32:
    logit [B, M], val [B, C, M], idx_flat [B, M] the segment of every entry"""
    lg, v, ix = torch.from_numpy(logit), torch.from_numpy(val), torch.from_numpy(idx_flat.astype(np.int64))
    B, M = lg.shape
    mx = torch.full((B, T), float("-inf")).scatter_reduce_(1, ix, lg, "amax", include_self=True)
    e = (lg - mx.gather(1, ix)).exp()
    w = e / torch.zeros(B, T).scatter_add_(1, ix, e).gather(1, ix)
    return torch.zeros(B, v.shape[1], T).scatter_add_(2, ix[:, None, :].expand_as(v), v * w[:, None, :]).numpy()


def knn_targets(rng, B, S, K, T):
    """a k-NN scatter index: the K nearest of T targets for each of S points"""
    a, t = rng.uniform(-2, 2, (B, S, 3)), rng.uniform(-2, 2, (B, T, 3))
    d = ((a[:, :, None, :] - t[:, None, :, :]) ** 2).sum(-1)
    return np.argsort(d, axis=-1, kind="stable")[:, :, :K].astype(np.int32)


SEG_CASES = [("uniform", 16, 1.0), ("csr_knn", 16, 1.0), ("one_segment_of_592", 16, 1.0), ("csr_knn_logits80", 16, 80.0),
             ("uniform_logits80", 16, 80.0), ("csr_knn_c1", 1, 1.0), ("csr_knn_c259", 259, 1.0), ("uniform_c259", 259, 1.0)]


@pytest.mark.parametrize("name,c,spread", SEG_CASES, ids=[s[0] for s in SEG_CASES])
def test_segment_softmax_sum_against_the_yardstick(dev, name, c, spread):
    from ssf import tflow as F
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    rng = np.random.default_rng(len(name) * 1000 + c)
    B, S, K, T = 3, 37, 16, 43                            # targets 40 to 42: nobody chooses them
    M = S * K
    logit = (rng.standard_normal((B, M)) * spread).astype(np.float32)
    val = rng.standard_normal((B, c, M)).astype(np.float32)
    if name.startswith("uniform"):
        T, idx, off, order = S, np.repeat(np.arange(S), K)[None].repeat(B, 0).reshape(B, S, K), None, None
    else:
        idx = np.full((B, S, K), 3, np.int32) if name.startswith("one_segment") else knn_targets(rng, B, S, K, 40)
        off, order = F.segments(_t(idx, dev), T)
        roff, rorder = R.segments(idx, T)
        assert np.array_equal(_n(off), roff) and np.array_equal(_n(order), rorder)
    ref64 = R.segment_softmax_sum(logit, val, T, None if off is None else _n(off), None if off is None else _n(order))
    ref32 = segment_cpu_f32(logit, val, T, idx.reshape(B, M))
    dl, dv = _t(logit, dev), _t(val, dev)
    got = F.segment_softmax_sum(dl, dv, T, off, order, check=True)
    again = F.segment_softmax_sum(dl, dv, T, off, order)
    alone = F.segment_softmax_sum(dl[1:2], dv[1:2], T, None if off is None else off[1:2], None if off is None else order[1:2])
    torch.cuda.synchronize()
    assert np.isfinite(_n(got)).all()
    hold(f"segment_softmax_sum {name} c={c}", _n(got), ref32, ref64)
    assert torch.equal(got, again), "two runs differ"
    assert torch.equal(alone[0], got[1]), "a batch element's bits depend on its batch"
    if off is not None:
        empty = _n(off)[:, 1:] == _n(off)[:, :-1]
        assert empty.any() and bool((got.permute(0, 2, 1)[torch.from_numpy(empty).to(dev)] == 0).all())

    def launch(order_t):
        pad, count = 1024, B * c * T
        buf = torch.full((pad + count + pad,), -777.0, dtype=torch.float32, device=dev)
        out = buf[pad:pad + count]
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = _abi.lib().ssf_pn2_segment_softmax_sum(_stream(dev), B, c, M, T, 0 if off is not None else K, _ptr(dl),
                                                    _ptr(dv), _ptr(off), _ptr(order_t), _ptr(out), _ptr(bad))
        torch.cuda.synchronize()
        assert rc == 0, _abi.lib().ssf_pn2_last_error()
        assert bool((buf[:pad] == -777.0).all()) and bool((buf[pad + count:] == -777.0).all())
        return out.view(B, c, T), int(bad.item())

    out, bad = launch(order)
    assert bad == 0 and torch.equal(out, got)
    if name == "csr_knn":
        # entries M and -1 of the order list read as entry 0 and set the flag
        broken = _n(order).copy()
        broken[0, 5], broken[2, M - 1] = M, -1
        out, bad = launch(_t(broken, dev))
        assert bad == 1
        fixed = np.where((broken < 0) | (broken >= M), 0, broken)
        ref64 = R.segment_softmax_sum(logit, val, T, _n(off), fixed)
        e_ref = np.abs(ref32.astype(np.float64) - R.segment_softmax_sum(logit, val, T, _n(off), _n(order))).max()
        e_dev = np.abs(_n(out).astype(np.float64) - ref64).max()
        print(f"[cv parity] segment_softmax_sum bad entries read as 0: e_dev {e_dev:.3e} ratio {e_dev / e_ref:.3f}")
        assert e_dev <= FACTOR * e_ref
        with pytest.raises(ValueError, match="out of range"):
            F.segment_softmax_sum(dl, dv, T, off, _t(broken, dev), check=True)


# ------------------------------------------------------------------------------------------
# the whole network

def test_tflow_on_the_fixture(tf, dev):
    import ssf
    net = ssf.TFlow()
    net.load_state_dict(state_of(tf), strict=True)
    net = net.to(dev)
    pc1, pc2 = _t(tf["pc1"], dev), _t(tf["pc2"], dev)
    flows, fps = net(pc1, pc2)
    flows2, fps2 = net(pc1, pc2)
    torch.cuda.synchronize()
    for i in range(3):
        assert np.array_equal(_n(fps[i]), tf[f"fps_inds{i}"]), f"fps_inds[{i}]"
    for i in range(4):
        f = _n(flows[i])
        assert f.shape == tf[f"flow{i}"].shape and np.isfinite(f).all() and np.abs(f).max() <= 50.0
        assert torch.equal(flows[i], flows2[i]), f"two forwards differ in flows[{i}]"
    hold("TFlow flows[3] (flow3_r, 256 points)", _n(flows[3]), tf["flow3"], tf["flow3_f64"])
    # from flow2_r on, k-NN runs on computed coordinates: a low-bit difference can swap a neighbour
    # and move a point's flow discontinuously, so these are reported, not asserted
    for i in range(3):
        ref64 = tf[f"flow{i}_f64"]
        e_ref = np.abs(tf[f"flow{i}"].astype(np.float64) - ref64).max()
        err = np.abs(_n(flows[i]).astype(np.float64) - ref64).max(axis=1)
        print(f"[cv parity] TFlow flows[{i}]: e_ref {e_ref:.3e} max {err.max():.3e} median {np.median(err):.3e} "
              f"points beyond 4 e_ref {100.0 * (err > FACTOR * e_ref).mean():.2f}%")

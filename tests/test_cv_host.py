"""Host side of the TFlow cost volume (ssf_pn2_grouped_mlp, ssf_pn2_pair_attention,
ssf_pn2_segment_softmax_sum, ssf.tflow): argument checks before any HIP call, the refusal of host
tensors, state_dict compatibility with the reference's modules, the folds, segments(), and the tie
between the numpy yardstick (tests/cv_reference.py) and the reference's own float64 outputs in
tests/golden/cv_ref.npz (made by tests/golden/make_golden_cv.py).  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cv_reference as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = {
    "A": dict(nsample=8, in_channel=12, sf_channel=10, mlp=[16, 16], flow_mlp=[16, 16], use_flow=True),
    "B": dict(nsample=5, in_channel=12, sf_channel=0, mlp=[16, 16], flow_mlp=[16, 16], use_flow=False),
}


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLD, "cv_ref.npz")))


@pytest.fixture(scope="module")
def tf():
    return dict(np.load(os.path.join(GOLD, "tflow_ref.npz")))


def shapes_of(g, prefix=""):
    return [(str(k), tuple(int(d) for d in s.split(",") if d))
            for k, s in zip(g[prefix + "keys"], g[prefix + "shapes"])]


def state_of(g, prefix=""):
    return R.seed_state(shapes_of(g, prefix), int(g[prefix + "seed"]))


def torch_state(state):
    return {k: torch.from_numpy(v) for k, v in state.items()}


def _gmlp(L, n_layers=2, widths=(20, 8, 8), k=3, c_ctr=6, c_g=6, c_d=5, xyz=1, idx=1, b=1, s=4, n=8, ptr=1,
          slope=1, out=1):
    w = (C.c_int32 * len(widths))(*widths)
    p = (C.c_void_p * 3)(ptr, ptr, ptr)
    sl = (C.c_float * 3)(0.0, 0.1, 1.0) if slope else None
    return L.ssf_pn2_grouped_mlp(None, b, n, s, k, c_ctr, c_g, c_d, 1, 1, 1, xyz, 1, idx, n_layers, w, p, p, p,
                                 sl, 1, out, 1)


@pytest.mark.parametrize("kw", [
    dict(n_layers=0), dict(n_layers=4, widths=(20, 8, 8, 8, 8)), dict(k=0), dict(k=33),
    dict(widths=(21, 8, 8)), dict(widths=(767, 8, 8), c_d=752), dict(widths=(20, 513, 8)), dict(widths=(20, 0, 8)),
    dict(idx=None), dict(ptr=None), dict(slope=0), dict(out=None), dict(b=-1), dict(s=-1), dict(n=0),
    dict(widths=(17, 8, 8), xyz=None, idx=None),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_grouped_mlp_arg_checks_before_any_hip_call(kw):
    """every pointer here is the invalid address 1 and no device exists: a call that got past
    the checks would fault or return SSF_E_HIP"""
    from ssf import _abi
    L = _abi.lib()
    assert _gmlp(L, **kw) == _abi.SSF_E_ARG
    assert b"grouped_mlp:" in L.ssf_pn2_last_error()


def test_pair_attention_and_segment_arg_checks_before_any_hip_call():
    from ssf import _abi
    L = _abi.lib()
    att = lambda b=1, c=4, s=4, k=3, q=1, o=1: L.ssf_pn2_pair_attention(None, b, c, s, k, q, 1, o, 1)  # noqa: E731
    for kw in (dict(k=0), dict(k=33), dict(c=0), dict(c=513), dict(q=None), dict(o=None), dict(b=-1), dict(s=-1)):
        assert att(**kw) == _abi.SSF_E_ARG, kw
        assert b"pair_attention" in L.ssf_pn2_last_error()
    seg = lambda b=1, c=4, m=12, t=4, k=3, lg=1, off=None, order=None, out=1, bad=1: \
        L.ssf_pn2_segment_softmax_sum(None, b, c, m, t, k, lg, 1, off, order, out, bad)  # noqa: E731
    for kw in (dict(off=1), dict(order=1), dict(k=0), dict(k=4), dict(m=13), dict(lg=None), dict(out=None),
               dict(bad=None), dict(b=-1), dict(c=-1), dict(t=-1), dict(off=1, order=1, lg=None)):
        assert seg(**kw) == _abi.SSF_E_ARG, kw
        assert b"segment_softmax_sum" in L.ssf_pn2_last_error()


def test_host_tensors_refused():
    from ssf import tflow as F
    w, sc = [torch.zeros(9, 4)], [torch.zeros(4)]
    with pytest.raises(ValueError, match="CUDA"):
        F.grouped_mlp(w, sc, sc, [0.0], idx=torch.zeros(1, 2, 3, dtype=torch.int32), feat=torch.zeros(1, 6, 8),
                      xyz=torch.zeros(1, 3, 8), new_xyz=torch.zeros(1, 3, 2))
    with pytest.raises(ValueError, match="CUDA"):
        F.pair_attention(torch.zeros(1, 4, 2, 3), torch.zeros(1, 4, 2, 3))
    with pytest.raises(ValueError, match="CUDA"):
        F.segment_softmax_sum(torch.zeros(1, 6), torch.zeros(1, 4, 6), 2)
    cv = F.CostVolume(**CASES["B"])
    with pytest.raises(ValueError, match="CUDA"):
        cv(torch.zeros(1, 3, 16), torch.zeros(1, 3, 16), None, torch.zeros(1, 12, 16), torch.zeros(1, 12, 16))
    with pytest.raises(ValueError, match="CUDA"):
        F.PointWarping()(torch.zeros(1, 3, 16), torch.zeros(1, 3, 16), torch.zeros(1, 3, 16), 5)
    with pytest.raises(ValueError, match="CUDA"):
        F.TFlow()(torch.zeros(1, 3, 64), torch.zeros(1, 3, 64))


def test_reference_key_lists_load_strict(g, tf):
    import ssf
    from ssf import tflow as F
    for name, cfg in CASES.items():
        state = torch_state(state_of(g, name + "/"))
        cv = F.CostVolume(**cfg)
        cv.load_state_dict(state, strict=True)
        assert sorted(cv.state_dict()) == sorted(state) and not cv.training
        assert {k: tuple(v.shape) for k, v in cv.state_dict().items()} == dict(shapes_of(g, name + "/"))
        reg = F.RefineFlowRegressor(cfg["nsample"], cfg["in_channel"], cfg["sf_channel"], cfg["mlp"],
                                    cfg["flow_mlp"], cfg["use_flow"])
        reg.load_state_dict({"cost." + k: v for k, v in state.items()}, strict=True)
        assert sorted(reg.state_dict()) == sorted("cost." + k for k in state)
    state = torch_state(state_of(tf))
    assert len(state) == 317 and sum(v.numel() for v in state.values()) == 2268852
    assert "flow0_r.cost.weightnet1.4.num_batches_tracked" in state
    assert "flow2_r.cost.flow_mlp_convs.1.composed_module.0.bias" in state and "deconv3_2.composed_module.0.weight" in state
    net = ssf.TFlow()
    net.load_state_dict(state, strict=True)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(shapes_of(tf))
    assert not net.training


def test_folds(g):
    from ssf import tflow as F
    cfg = CASES["A"]
    cv = F.CostVolume(**cfg)
    before = cv.folded()["weightnet"][1][0].clone()
    st = state_of(g, "A/")
    cv.load_state_dict(torch_state(st), strict=True)
    p = cv.folded()
    assert not torch.equal(before, p["weightnet"][1][0])                 # the cache was rebuilt by the load
    c, f = 16, 10
    # bias as shift under a scale of 1, slope 0.1
    ws, scs, shs, sl = p["mlp1"]
    assert sl == [0.1, 0.1] and all(w.is_contiguous() and w.dtype == torch.float32 for w in ws)
    for i in range(2):
        assert np.array_equal(ws[i].numpy(), st[f"mlp_convs.{i}.weight"][:, :, 0, 0].T)
        assert np.array_equal(shs[i].numpy(), st[f"mlp_convs.{i}.bias"]) and bool((scs[i] == 1).all())
    assert np.array_equal(p["mlp2"][0][0].numpy(), st["mlp_convs2.0.weight"][:, :, 0, 0].T)
    # weightnet1: BatchNorm folded in float64, ReLU, ReLU, then bias only without activation
    ws, scs, shs, sl = p["weightnet"]
    assert sl == [0.0, 0.0, 1.0] and [tuple(w.shape) for w in ws] == [(16, 16), (16, 8), (8, 1)]
    for i, bn in enumerate(("weightnet1.1", "weightnet1.4")):
        gam, bet, mu, var = (st[f"{bn}.{n}"].astype(np.float64) for n in ("weight", "bias", "running_mean", "running_var"))
        scale = gam / np.sqrt(var + 1e-5)
        assert np.array_equal(scs[i].numpy(), scale.astype(np.float32))
        assert np.array_equal(shs[i].numpy(), (bet - mu * scale).astype(np.float32))
    assert np.array_equal(shs[2].numpy(), st["weightnet1.6.bias"]) and bool((scs[2] == 1).all())
    # mlp_convs3: (features, sf_feat, direction) -> (sf_feat, features, direction)
    w3 = st["mlp_convs3.0.weight"][:, :, 0, 0].T                          # [16 + 10 + 3, 16]
    assert np.array_equal(p["mlp3"][0][0].numpy(), np.concatenate([w3[c:c + f], w3[:c], w3[c + f:]]))
    # mlp_convs4: (cost_fwd, cost_bwd, sf_feat, direction) -> (cost_fwd, sf_feat, cost_bwd, direction)
    w4 = st["mlp_convs4.0.weight"][:, :, 0, 0].T                          # [16 + 16 + 10 + 3, 16]
    assert np.array_equal(p["mlp4"][0][0].numpy(),
                          np.concatenate([w4[:c], w4[2 * c:2 * c + f], w4[c:2 * c], w4[2 * c + f:]]))
    assert np.array_equal(p["mlp4"][0][1].numpy(), st["mlp_convs4.1.weight"][:, :, 0, 0].T)
    # without sf_feat the permutations are the identity
    cvb = F.CostVolume(**CASES["B"])
    cvb.load_state_dict(torch_state(state_of(g, "B/")), strict=True)
    assert np.array_equal(cvb.folded()["mlp4"][0][0].numpy(), state_of(g, "B/")["mlp_convs4.0.weight"][:, :, 0, 0].T)
    # a move drops the cache too
    cv.float()
    assert cv._folded is None


def test_segments_against_a_stable_argsort():
    from ssf import tflow as F
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 9, (2, 7, 4))
    idx[idx == 5] = 6                                     # target 5: nobody chose it
    idx[1] = 2                                            # batch element 1: everybody chose target 2
    off, order = F.segments(torch.from_numpy(idx), 11)    # targets 9 and 10 are empty too
    assert off.dtype == order.dtype == torch.int32 and off.shape == (2, 12) and order.shape == (2, 28)
    roff, rorder = R.segments(idx, 11)
    assert np.array_equal(off.numpy(), roff) and np.array_equal(order.numpy(), rorder)
    flat = idx.reshape(2, -1)
    for b in range(2):
        assert np.array_equal(order[b].numpy(), np.argsort(flat[b], kind="stable"))
        for t in range(11):
            seg = order[b, off[b, t]:off[b, t + 1]].numpy()
            assert np.array_equal(seg, np.nonzero(flat[b] == t)[0])       # ascending flat entries
    assert off[0, 5] == off[0, 6] and off[1, 2] == 0 and off[1, 3] == 28
    with pytest.raises(ValueError):
        F.segments(torch.from_numpy(idx), 2)              # batch element 1 names target 2


def test_train_raises():
    from ssf import tflow as F
    for m in (F.CostVolume(**CASES["A"]), F.RefineFlowRegressor(), F.TFlow()):
        with pytest.raises(NotImplementedError):
            m.train()
        assert m.eval() is m and not m.training
    with pytest.raises(NotImplementedError):
        F.CostVolume(8, 12, 0, [16, 16, 16, 16], [16])


@pytest.mark.parametrize("name", ["A", "B"])
def test_yardstick_reproduces_the_reference_f64_outputs(g, name):
    """tests/cv_reference.py against the reference modules' own float64 outputs"""
    p = name + "/"
    cfg = CASES[name]
    sf = g[p + "flow"] if cfg["use_flow"] else None
    outs = R.cost_volume(state_of(g, p), 2, 2, g[p + "xyz1"], g[p + "xyz2"], g[p + "points1"], g[p + "points2"],
                         g[p + "knn_idx"], g[p + "knn_idxw"], sf, g.get(p + "sf_feat"))
    assert int(g[p + "knn_idxw"].max()) + 1 == g[p + "xyz2"].shape[2]
    for n, got in zip(("cost_fwd", "cost_bwd", "cost", "flow_out"), outs):
        ref = g[p + n + "_f64"]
        assert got.shape == ref.shape, n
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (n, np.abs(got - ref).max())
        e = np.abs(g[p + n].astype(np.float64) - ref).max()
        assert 0 < e < 1e-5 * np.abs(ref).max(), (n, e)
    warp = R.point_warping(g[p + "xyz1"], g[p + "xyz2"], g[p + "flow"], g[p + "warp_idx"])
    ref = g[p + "pc2_warp_f64"]
    assert np.abs(warp - ref).max() <= 1e-12 * np.abs(ref).max()
    assert 0 < np.abs(g[p + "pc2_warp"].astype(np.float64) - ref).max() < 1e-5 * np.abs(ref).max()

"""Host side of the fused set-abstraction layers (ssf_pn2_grouped_mlp_max, ssf.pointnet2's
SetAbstraction / SetUpConv): argument checks before any HIP call, the refusal of host tensors,
state_dict compatibility with the reference's modules, the BatchNorm fold, and the tie between
the numpy yardstick (tests/sa_reference.py) and the reference's own float64 outputs in
tests/golden/sa_ref.npz (made by tests/golden/make_golden_sa.py).  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sa_reference as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "sa_ref.npz")
SA_ARGS = dict(npoint=37, radius=0.5, nsample=16, in_channel=6, mlp=[16, 24, 40])
SU_ARGS = dict(nsample=5, radius=2.4, f1_channel=7, f2_channel=40, mlp=[24, 20], mlp2=[12])


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def state_of(g, prefix):
    return {k[len(prefix) + 1:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix + "/")}


def _call(L, n_layers=3, widths=(9, 8, 8, 8), k=3, c=6, idx=1, b=1, s=4, ptr=1):
    w = (C.c_int32 * len(widths))(*widths)
    p = (C.c_void_p * 3)(ptr, ptr, ptr)
    return L.ssf_pn2_grouped_mlp_max(None, b, 8, s, k, c, 1, 1, 1, idx, n_layers, w, p, p, p, 1, 1)


@pytest.mark.parametrize("kw", [
    dict(n_layers=0), dict(n_layers=4, widths=(9, 8, 8, 8, 8)), dict(widths=(9, 8, 513, 8)),
    dict(widths=(9, 8, 0, 8)), dict(widths=(10, 8, 8, 8)), dict(k=33), dict(k=0), dict(idx=None),
    dict(b=-1), dict(s=-1), dict(ptr=None),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_arg_checks_before_any_hip_call(kw):
    """every pointer here is the invalid address 1 and no device exists: a call that got past
    the checks would fault or return SSF_E_HIP"""
    from ssf import _abi
    L = _abi.lib()
    assert _call(L, **kw) == _abi.SSF_E_ARG
    assert b"grouped_mlp" in L.ssf_pn2_last_error()


def test_host_tensors_refused():
    from ssf import pointnet2 as P
    w = [torch.zeros(9, 4)]
    sc = [torch.zeros(4)]
    with pytest.raises(ValueError, match="CUDA"):
        P.grouped_mlp_max(torch.zeros(1, 3, 8), torch.zeros(1, 3, 2), torch.zeros(1, 6, 8),
                          torch.zeros(1, 2, 3, dtype=torch.int32), w, sc, sc)
    with pytest.raises(ValueError, match="CUDA"):
        P.SetAbstraction(**SA_ARGS)(torch.zeros(1, 3, 64), torch.zeros(1, 6, 64))
    with pytest.raises(ValueError, match="CUDA"):
        P.SetUpConv(**SU_ARGS)(torch.zeros(1, 3, 64), torch.zeros(1, 3, 8), torch.zeros(1, 7, 64),
                               torch.zeros(1, 40, 8))


def test_reference_state_dicts_load_strict(g):
    from ssf import pointnet2 as P
    sa, su = P.SetAbstraction(**SA_ARGS), P.SetUpConv(**SU_ARGS)
    sa_state, su_state = state_of(g, "sa_state"), state_of(g, "su_state")
    assert "mlp_convs.0.weight" in sa_state and sa_state["mlp_convs.0.weight"].shape == (16, 9, 1, 1)
    assert "mlp_bns.2.running_var" in sa_state and "mlp2_convs.0.1.running_mean" in su_state
    sa.load_state_dict(sa_state, strict=True)
    su.load_state_dict(su_state, strict=True)
    assert sorted(sa.state_dict()) == sorted(sa_state) and sorted(su.state_dict()) == sorted(su_state)
    assert not sa.training and not su.training


def test_bn_fold_is_the_f64_formula_and_follows_a_load(g):
    from ssf import pointnet2 as P
    sa = P.SetAbstraction(**SA_ARGS)
    before = [t.clone() for t in sa.folded()[1]]
    st = state_of(g, "sa_state")
    sa.load_state_dict(st, strict=True)
    ws, scs, shs = sa.folded()
    assert not torch.equal(before[0], scs[0])            # the cache was rebuilt by the load
    for i in range(3):
        gam, bet, mu, var = (st[f"mlp_bns.{i}.{n}"].numpy().astype(np.float64)
                             for n in ("weight", "bias", "running_mean", "running_var"))
        scale = gam / np.sqrt(var + 1e-5)
        shift = bet - mu * scale
        assert scs[i].dtype == torch.float32 and np.array_equal(scs[i].numpy(), scale.astype(np.float32))
        assert np.array_equal(shs[i].numpy(), shift.astype(np.float32))
        assert np.array_equal(ws[i].numpy(), st[f"mlp_convs.{i}.weight"].numpy()[:, :, 0, 0].T)
        assert ws[i].is_contiguous()
    # SetUpConv: (features, pos_diff) rows of the first layer become (pos_diff, features)
    su = P.SetUpConv(**SU_ARGS)
    su.load_state_dict(state_of(g, "su_state"), strict=True)
    w0 = g["su_state/mlp1_convs.0.0.weight"][:, :, 0, 0].T               # [43, 24]
    assert np.array_equal(su.folded()[0][0].numpy(), np.concatenate([w0[40:], w0[:40]]))


def test_train_and_unsupported_options_raise():
    from ssf import pointnet2 as P
    sa, su = P.SetAbstraction(**SA_ARGS), P.SetUpConv(**SU_ARGS)
    for m in (sa, su):
        with pytest.raises(NotImplementedError):
            m.train()
        assert m.eval() is m and not m.training
    with pytest.raises(NotImplementedError):
        P.SetAbstraction(use_instance_norm=True, **SA_ARGS)
    with pytest.raises(NotImplementedError):
        P.SetUpConv(knn=False, **SU_ARGS)
    with pytest.raises(NotImplementedError):
        P.SetUpConv(**dict(SU_ARGS, mlp=[]))
    with pytest.raises(NotImplementedError):
        su(None, None, None, None, sf1=torch.zeros(1))


def test_yardstick_reproduces_the_reference_f64_outputs(g):
    """tests/sa_reference.py against the reference modules' own .double() outputs"""
    new_xyz, sa_out = R.set_abstraction(state_of_np(g, "sa_state"), 3, g["xyz"], g["points"],
                                        g["fps_idx"], g["sa_knn_idx"])
    assert np.array_equal(new_xyz.astype(np.float32), g["sa_new_xyz"])
    assert np.abs(sa_out - g["sa_out_f64"]).max() <= 1e-12 * np.abs(g["sa_out_f64"]).max()
    su_out = R.set_upconv(state_of_np(g, "su_state"), 2, 1, g["xyz"], g["sa_new_xyz"], g["feat1"],
                          g["sa_out"], g["su_knn_idx"])
    assert su_out.shape == g["su_out_f64"].shape == (2, 12, 512)
    assert np.abs(su_out - g["su_out_f64"]).max() <= 1e-12 * np.abs(g["su_out_f64"]).max()
    # the fixture itself: float32 and float64 runs of the reference differ by rounding only
    for name in ("sa_out", "su_out"):
        e = np.abs(g[name].astype(np.float64) - g[name + "_f64"]).max()
        assert 0 < e < 1e-5 * np.abs(g[name + "_f64"]).max(), (name, e)


def state_of_np(g, prefix):
    return {k[len(prefix) + 1:]: v for k, v in g.items() if k.startswith(prefix + "/")}

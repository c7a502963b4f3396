"""The fused set-abstraction kernel (ssf_pn2_grouped_mlp_max, csrc/pointnet2.hip) and the two
modules on it (ssf.pointnet2.SetAbstraction / SetUpConv) on the GPU, against the reference's own
modules (tests/golden/sa_ref.npz) and the numpy float64 yardstick (tests/sa_reference.py).

The bar, for features only: with e_ref = max|ref_f32 - ref_f64| (the float32 rounding of the
reference itself on that case: the fixture's two runs, or CPU torch in float32 against the
yardstick for the cases without a fixture -- never the device's output), the device must have
max|dev - ref_f64| <= 4 e_ref.  Both are float32 evaluations of the same arithmetic in another
summation order, and the device folds BatchNorm where torch does not.  Indices and coordinates
(fps_idx, new_xyz) are bit-exact.  Every test prints its ratio.
"""
import os

import numpy as np
import pytest
import torch

import sa_reference as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "sa_ref.npz")
SA_ARGS = dict(npoint=37, radius=0.5, nsample=16, in_channel=6, mlp=[16, 24, 40])
SU_ARGS = dict(nsample=5, radius=2.4, f1_channel=7, f2_channel=40, mlp=[24, 20], mlp2=[12])
FACTOR = 4.0


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def state_of(g, prefix):
    return {k[len(prefix) + 1:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix + "/")}


def hold(name, dev_out, ref32, ref64):
    e_ref = np.abs(ref32.astype(np.float64) - ref64).max()
    e_dev = np.abs(dev_out.astype(np.float64) - ref64).max()
    print(f"[sa parity] {name}: e_ref {e_ref:.3e} e_dev {e_dev:.3e} ratio {e_dev / e_ref:.3f}")
    assert e_ref > 0
    assert e_dev <= FACTOR * e_ref, (name, e_dev, e_ref)


def make_case(seed, B, N, S, K, c, widths):
    """numpy-seeded inputs, weights of unit-variance layers, non-trivial scale and shift"""
    rng = np.random.default_rng(seed)
    assert widths[0] == 3 + c
    xyz = rng.uniform(-2, 2, (B, 3, N)).astype(np.float32)
    new_xyz = rng.uniform(-2, 2, (B, 3, S)).astype(np.float32)
    feat = rng.standard_normal((B, c, N)).astype(np.float32) if c else None
    idx = rng.integers(0, N, (B, S, K)).astype(np.int32)
    ws = [(rng.standard_normal((i, o)) / np.sqrt(i)).astype(np.float32) for i, o in zip(widths, widths[1:])]
    scs = [rng.uniform(0.5, 1.5, o).astype(np.float32) for o in widths[1:]]
    shs = [(rng.standard_normal(o) * 0.2).astype(np.float32) for o in widths[1:]]
    return dict(xyz=xyz, new_xyz=new_xyz, feat=feat, idx=idx, ws=ws, scs=scs, shs=shs)


def torch_layers(x, ws, scs, shs):
    """the layers on a grouped [B, C, S, K] tensor with torch ops (any device, float32)"""
    for w, sc, sh in zip(ws, scs, shs):
        x = torch.nn.functional.conv2d(x, w.t().contiguous()[:, :, None, None])
        x = torch.relu(x * sc[None, :, None, None] + sh[None, :, None, None])
    return x.max(-1)[0]


def cpu_torch_f32(case):
    """e_ref's float32 side: the same layers evaluated with CPU torch"""
    B, _, N = case["xyz"].shape
    ix = np.where((case["idx"] < 0) | (case["idx"] >= N), 0, case["idx"]).astype(np.int64)
    # the float32 grouping: one subtraction per coordinate, exact gathers
    x = np.stack([case["xyz"][b][:, ix[b]] - case["new_xyz"][b][:, :, None] for b in range(B)])
    if case["feat"] is not None:
        x = np.concatenate([x, np.stack([case["feat"][b][:, ix[b]] for b in range(B)])], axis=1)
    assert x.dtype == np.float32
    f = lambda arrs: [torch.from_numpy(a) for a in arrs]  # noqa: E731
    return torch_layers(torch.from_numpy(x), f(case["ws"]), f(case["scs"]), f(case["shs"])).numpy()


def run_device(case, dev, sel=slice(None), out=None, check=False):
    from ssf import pointnet2 as P
    d = lambda arrs: [_t(a, dev) for a in arrs]  # noqa: E731
    feat = None if case["feat"] is None else _t(case["feat"][sel], dev)
    y = P.grouped_mlp_max(_t(case["xyz"][sel], dev), _t(case["new_xyz"][sel], dev), feat,
                          _t(case["idx"][sel], dev), d(case["ws"]), d(case["scs"]), d(case["shs"]), check=check)
    torch.cuda.synchronize()
    return y


def yardstick(case):
    return R.grouped_mlp_max(case["xyz"], case["new_xyz"], case["feat"], case["idx"], case["ws"],
                             case["scs"], case["shs"])


def test_modules_against_the_reference_fixture(g, dev):
    from ssf import pointnet2 as P
    sa, su = P.SetAbstraction(**SA_ARGS), P.SetUpConv(**SU_ARGS)
    sa.load_state_dict(state_of(g, "sa_state"), strict=True)
    su.load_state_dict(state_of(g, "su_state"), strict=True)
    sa, su = sa.to(dev), su.to(dev)
    xyz, points = _t(g["xyz"], dev), _t(g["points"], dev)
    with torch.no_grad():
        new_xyz, new_points, fps_idx = sa(xyz, points)
        again = sa(xyz, points, fps_idx)
        # the fixture's own centroids and features feed the decoder layer, as in make_golden_sa.py
        up = su(xyz, _t(g["sa_new_xyz"], dev), _t(g["feat1"], dev), _t(g["sa_out"], dev))
    assert np.array_equal(fps_idx.cpu().numpy(), g["fps_idx"])
    assert np.array_equal(new_xyz.cpu().numpy().view(np.uint32), g["sa_new_xyz"].view(np.uint32))
    assert torch.equal(again[1], new_points) and torch.equal(again[0], new_xyz)
    assert new_points.shape == (2, 40, 37) and up.shape == (2, 12, 512)
    hold("fixture SetAbstraction", new_points.cpu().numpy(), g["sa_out"], g["sa_out_f64"])
    hold("fixture SetUpConv", up.cpu().numpy(), g["su_out"], g["su_out_f64"])


# (name, N, S, K, c, widths): the issue's shapes, then one case per remaining column-tile path
# (64 columns; 32 columns with the two largest LDS images: DESIGN.md §6.9)
EDGE_CASES = [
    ("k1_9-1", 200, 37, 1, 6, [9, 1]),
    ("k5_9-33-17", 200, 37, 5, 6, [9, 33, 17]),
    ("k32_s1_xyz_only", 131, 1, 32, 0, [3, 8]),
    ("k16_sa1_35-32-32-64", 200, 37, 16, 32, [35, 32, 32, 64]),
    ("k5_s1_one_layer", 64, 1, 5, 6, [9, 24]),
    ("k7_tile64_9-200-17", 200, 37, 7, 6, [9, 200, 17]),
    ("k3_tile32_512x4", 64, 5, 3, 509, [512, 512, 512, 512]),
]


@pytest.mark.parametrize("name,N,S,K,c,widths", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_edge_shapes_against_the_yardstick(dev, name, N, S, K, c, widths):
    case = make_case(sum(widths) + K, 3, N, S, K, c, widths)
    ref64 = yardstick(case)
    got = run_device(case, dev, check=True)
    assert got.shape == (3, widths[-1], S)
    hold(name, got.cpu().numpy(), cpu_torch_f32(case), ref64)
    alone = run_device(case, dev, sel=slice(1, 2))
    assert torch.equal(alone[0], got[1]), "a batch element's bits depend on its batch"


@pytest.fixture(scope="module")
def sa4():
    case = make_case(4, 1, 256, 128, 8, 256, [259, 256, 256, 512])
    return case, yardstick(case), cpu_torch_f32(case)


def test_widest_layer_sa4(dev, sa4):
    case, ref64, ref32 = sa4
    got = run_device(case, dev, check=True)
    hold("sa4 259-256-256-512", got.cpu().numpy(), ref32, ref64)


def test_sa4_is_deterministic(dev, sa4):
    a, b = run_device(sa4[0], dev), run_device(sa4[0], dev)
    assert torch.equal(a, b)


def test_write_bounds_and_bad_indices(dev):
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    import ctypes as C
    B, N, S, K, c, widths = 2, 96, 7, 5, 6, [9, 33, 17]
    case = make_case(77, B, N, S, K, c, widths)
    d = lambda arrs: [_t(a, dev) for a in arrs]  # noqa: E731
    ws, scs, shs = d(case["ws"]), d(case["scs"]), d(case["shs"])
    xyz, nx, ft = _t(case["xyz"], dev), _t(case["new_xyz"], dev), _t(case["feat"], dev)
    pad, count = 1024, B * widths[-1] * S
    ptrs = C.c_void_p * 2

    def launch(idx_np):
        buf = torch.full((pad + count + pad,), -777.0, dtype=torch.float32, device=dev)
        out = buf[pad:pad + count]
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        ix = _t(idx_np, dev)
        rc = _abi.lib().ssf_pn2_grouped_mlp_max(
            _stream(dev), B, N, S, K, c, _ptr(xyz), _ptr(nx), _ptr(ft), _ptr(ix), 2,
            (C.c_int32 * 3)(*widths), ptrs(*[_ptr(t) for t in ws]), ptrs(*[_ptr(t) for t in scs]),
            ptrs(*[_ptr(t) for t in shs]), _ptr(out), _ptr(bad))
        torch.cuda.synchronize()
        assert rc == 0, _abi.lib().ssf_pn2_last_error()
        assert bool((buf[:pad] == -777.0).all()) and bool((buf[pad + count:] == -777.0).all())
        return out.view(B, widths[-1], S).cpu().numpy(), int(bad.item())

    got, bad = launch(case["idx"])
    assert bad == 0
    assert not (got == -777.0).any()
    hold("bounds, valid indices", got, cpu_torch_f32(case), yardstick(case))
    broken = dict(case, idx=case["idx"].copy())
    broken["idx"][0, 3, 2] = N
    broken["idx"][1, 6, 4] = -1
    got, bad = launch(broken["idx"])
    assert bad == 1
    fixed = dict(case, idx=broken["idx"].copy())
    fixed["idx"][0, 3, 2] = 0
    fixed["idx"][1, 6, 4] = 0
    hold("bounds, index n and -1 read as 0", got, cpu_torch_f32(fixed), yardstick(fixed))
    with pytest.raises(ValueError, match="out of range"):
        run_device(broken, dev, check=True)


def test_fused_against_the_unfused_device_composition(dev):
    """group_relative, then torch conv2d, affine, relu and max on the device"""
    from ssf import pointnet2 as P
    case = make_case(5, 2, 300, 37, 16, 32, [35, 32, 32, 64])
    d = lambda arrs: [_t(a, dev) for a in arrs]  # noqa: E731
    grouped = P.group_relative(_t(case["xyz"], dev), _t(case["new_xyz"], dev), _t(case["feat"], dev),
                               _t(case["idx"], dev), check=True)
    unfused = torch_layers(grouped, d(case["ws"]), d(case["scs"]), d(case["shs"])).cpu().numpy()
    ref64, ref32 = yardstick(case), cpu_torch_f32(case)
    fused = run_device(case, dev).cpu().numpy()
    hold("fused", fused, ref32, ref64)
    e_ref = np.abs(ref32.astype(np.float64) - ref64).max()
    d_fu = np.abs(fused.astype(np.float64) - unfused.astype(np.float64)).max()
    e_un = np.abs(unfused.astype(np.float64) - ref64).max()
    print(f"[sa parity] unfused device composition: e_dev {e_un:.3e} ratio {e_un / e_ref:.3f}")
    print(f"[sa parity] fused vs unfused: max diff {d_fu:.3e} ratio {d_fu / e_ref:.3f}")
    assert d_fu <= FACTOR * e_ref

"""TFlow point-set operators on the GPU: the `lib.pointnet2_utils`
("pointutils") surface that scripts/ActiveSceneFlow/utils/utils.py:7 and utils/soflow.py:7
import, over the C ABI in include/ssf_pointnet2.h (hand-written HIP, csrc/pointnet2.hip).

Same names, argument order and layouts as the calls in the reference network:

    furthest_point_sample(xyz_t [B,N,3], npoint)            utils.py:226  -> int32 [B,npoint]
    gather_operation(features [B,C,N], idx [B,S])           utils.py:228  -> [B,C,S]
    knn(k, query [B,S,3], ref [B,N,3])                      utils.py:229  -> (dist, idx) [B,S,k]
    grouping_operation(features [B,C,N], idx [B,S,K])       utils.py:231  -> [B,C,S,K]
    three_nn(unknown [B,N,3], known [B,M,3])                utils.py:560  -> (dist, idx) [B,N,3]
    three_interpolate(features [B,C,M], idx, weight)        utils.py:662  -> [B,C,N]
    UpsampleFlow()(xyz [B,3,N], sparse_xyz [B,3,S], sparse_flow [B,C,S], k)  soflow.py:1442
    group_relative(xyz, new_xyz, points, idx)   utils.py:228-234 (grouping block, fused)
    grouped_mlp_max(xyz, new_xyz, points, idx, weights, scales, shifts)
                                                utils.py:231-247 (grouping + mlp + max, fused)
    SetAbstraction(npoint, radius, nsample, in_channel, mlp)     utils.py:185-248 (inference)
    SetUpConv(nsample, radius, f1_channel, f2_channel, mlp, mlp2)  utils.py:250-315 (inference)

Inputs are CUDA tensors (float32 coordinates/features, integer indices); there is no CPU path.
Invalid arguments raise ValueError; a failing launch raises SSFError.
"""
from __future__ import annotations

import ctypes

import torch

from . import _abi
from .frontend import _ptr, _stream

__all__ = ["furthest_point_sample", "gather_operation", "knn", "grouping_operation", "three_nn",
           "three_interpolate", "upsample_flow", "UpsampleFlow", "group_relative", "grouped_mlp_max",
           "fold_batchnorm", "SetAbstraction", "SetUpConv"]


def _check(rc, what):
    if rc == 0:
        return
    msg = _abi.lib().ssf_pn2_last_error().decode(errors="replace")
    if rc == -1:
        raise ValueError(f"{what}: {msg}")
    raise _abi.SSFError(f"{what}: {msg}")


def _f32(t, name, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor")
    if t.dim() != dims:
        raise ValueError(f"{name} must have {dims} dimensions, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _i32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor")
    return t.detach().to(torch.int32).contiguous()


def _bad_flag(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def _raise_if_bad(bad, check, what):
    if check and int(bad.item()) != 0:
        raise ValueError(f"{what}: index out of range")


def furthest_point_sample(xyz, npoint, start=None):
    """pointutils.furthest_point_sample (torch restatement: utils.py:68-89).  start: optional
    [B] first centroids (default 0)."""
    x = _f32(xyz, "xyz", 3)
    B, N, c3 = x.shape
    if c3 != 3:
        raise ValueError("xyz must be [B, N, 3]")
    out = torch.empty((B, int(npoint)), dtype=torch.int32, device=x.device)
    st = None
    if start is not None:
        st = _i32(torch.as_tensor(start, device=x.device), "start")
        if st.numel() != B:
            raise ValueError("start must hold one index per batch element")
    tmp = torch.empty((B, N), dtype=torch.float32, device=x.device) if N > 16384 else None
    rc = _abi.lib().ssf_pn2_furthest_point_sample(_stream(x.device), B, N, int(npoint), _ptr(x),
                                                  _ptr(st), _ptr(tmp), _ptr(out))
    _check(rc, "furthest_point_sample")
    return out


def knn(k, query, ref):
    """pointutils.knn(k, query, ref) (torch restatement knn_point, utils.py:92-108):
    -> (dist = sqrt of the squared distance, idx int32), both [B, S, k], ascending."""
    q = _f32(query, "query", 3)
    r = _f32(ref, "ref", 3)
    B, S, _ = q.shape
    if r.shape[0] != B or r.shape[2] != 3 or q.shape[2] != 3:
        raise ValueError("query [B, S, 3] and ref [B, N, 3] expected")
    N = r.shape[1]
    k = int(k)
    if not (0 < k <= _abi.PN2_KNN_MAX) or N == 0:
        raise ValueError(f"knn: need 0 < k <= {_abi.PN2_KNN_MAX} and a non-empty reference set")
    dist = torch.empty((B, S, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, S, k), dtype=torch.int32, device=q.device)
    _check(_abi.lib().ssf_pn2_knn(_stream(q.device), B, S, N, k, _ptr(q), _ptr(r), _ptr(dist),
                                  _ptr(idx)), "knn")
    return dist, idx


def three_nn(unknown, known):
    """pointutils.three_nn(unknown [B,N,3], known [B,M,3]) -> (dist, idx) [B, N, 3]."""
    return knn(3, unknown, known)


def _gather(features, idx, check, what):
    f = _f32(features, "features", 3)
    ix = _i32(idx, "idx")
    B, Cc, N = f.shape
    if ix.shape[0] != B:
        raise ValueError(f"{what}: batch sizes differ")
    g = int(ix[0].numel()) if B else 0
    out = torch.empty((B, Cc) + tuple(ix.shape[1:]), dtype=torch.float32, device=f.device)
    bad = _bad_flag(f.device)
    _check(_abi.lib().ssf_pn2_gather(_stream(f.device), B, Cc, N, g, _ptr(f), _ptr(ix), _ptr(out),
                                     _ptr(bad)), what)
    _raise_if_bad(bad, check, what)
    return out


def gather_operation(features, idx, check=False):
    """pointutils.gather_operation(features [B,C,N], idx [B,S]) -> [B,C,S]."""
    return _gather(features, idx, check, "gather_operation")


def grouping_operation(features, idx, check=False):
    """pointutils.grouping_operation(features [B,C,N], idx [B,S,K]) -> [B,C,S,K]."""
    return _gather(features, idx, check, "grouping_operation")


def group_relative(xyz, new_xyz, points, idx, check=False):
    """The grouping block of PointNetSetAbstraction.forward (utils.py:228-234), one call:
    cat([grouping_operation(xyz, idx) - new_xyz.unsqueeze(-1), grouping_operation(points, idx)],
    dim=1).  xyz [B,3,N] (N <= 36864), new_xyz [B,3,S], points [B,C,N] or None, idx [B,S,K]
    -> [B, 3 + C, S, K]."""
    x = _f32(xyz, "xyz", 3)
    nx = _f32(new_xyz, "new_xyz", 3)
    ix = _i32(idx, "idx")
    B, c3, N = x.shape
    if c3 != 3 or nx.shape[:2] != (B, 3) or ix.dim() != 3 or ix.shape[:2] != (B, nx.shape[2]):
        raise ValueError("xyz [B,3,N], new_xyz [B,3,S] and idx [B,S,K] expected")
    S, K = ix.shape[1], ix.shape[2]
    f = None
    Cc = 0
    if points is not None:
        f = _f32(points, "points", 3)
        if f.shape[0] != B or f.shape[2] != N:
            raise ValueError("points must be [B, C, N]")
        Cc = f.shape[1]
    out = torch.empty((B, 3 + Cc, S, K), dtype=torch.float32, device=x.device)
    bad = _bad_flag(x.device)
    _check(_abi.lib().ssf_pn2_group_relative(_stream(x.device), B, N, S, K, Cc, _ptr(x), _ptr(nx),
                                             _ptr(f), _ptr(ix), _ptr(out), _ptr(bad)),
           "group_relative")
    _raise_if_bad(bad, check, "group_relative")
    return out


def three_interpolate(features, idx, weight, check=False):
    """pointutils.three_interpolate(features [B,C,M], idx [B,N,3], weight [B,N,3]) -> [B,C,N]."""
    f = _f32(features, "features", 3)
    ix = _i32(idx, "idx")
    w = _f32(weight, "weight", 3)
    B, Cc, M = f.shape
    if ix.shape != w.shape or ix.dim() != 3 or ix.shape[0] != B or ix.shape[2] != 3:
        raise ValueError("idx and weight must both be [B, N, 3]")
    N = ix.shape[1]
    out = torch.empty((B, Cc, N), dtype=torch.float32, device=f.device)
    bad = _bad_flag(f.device)
    _check(_abi.lib().ssf_pn2_three_interpolate(_stream(f.device), B, Cc, M, N, _ptr(f), _ptr(ix),
                                                _ptr(w), _ptr(out), _ptr(bad)), "three_interpolate")
    _raise_if_bad(bad, check, "three_interpolate")
    return out


def upsample_flow(xyz, sparse_xyz, sparse_flow, k=3):
    """UpsampleFlow.forward (soflow.py:1442-1470), one fused kernel: xyz [B,3,N],
    sparse_xyz [B,3,S] (S <= 4096), sparse_flow [B,C,S] -> [B,C,N]."""
    x = _f32(xyz, "xyz", 3)
    sx = _f32(sparse_xyz, "sparse_xyz", 3)
    sf = _f32(sparse_flow, "sparse_flow", 3)
    B, c3, N = x.shape
    S = sx.shape[2]
    if c3 != 3 or sx.shape[:2] != (B, 3) or sf.shape[0] != B or sf.shape[2] != S:
        raise ValueError("xyz [B,3,N], sparse_xyz [B,3,S], sparse_flow [B,C,S] expected")
    if not (0 < S <= _abi.PN2_UPSAMPLE_MAX_SPARSE) or not (0 < int(k) <= 16):
        raise ValueError(f"upsample_flow: need 0 < S <= {_abi.PN2_UPSAMPLE_MAX_SPARSE}, 0 < k <= 16")
    out = torch.empty((B, sf.shape[1], N), dtype=torch.float32, device=x.device)
    if out.numel() == 0:                # no channels (or points): empty tensors have no address
        return out
    _check(_abi.lib().ssf_pn2_upsample_flow(_stream(x.device), B, N, S, sf.shape[1], int(k),
                                            _ptr(x), _ptr(sx), _ptr(sf), _ptr(out)),
           "upsample_flow")
    return out


class UpsampleFlow(torch.nn.Module):
    """soflow.py:1442 UpsampleFlow (no parameters): forward(xyz, sparse_xyz, sparse_flow, k=3)."""

    def forward(self, xyz, sparse_xyz, sparse_flow, k=3):
        return upsample_flow(xyz, sparse_xyz, sparse_flow, k)


def grouped_mlp_max(xyz, new_xyz, points, idx, weights, scales, shifts, check=False):
    """ssf_pn2_grouped_mlp_max: the grouping block above, the shared mlp and the max over the K
    samples in one kernel.  xyz [B,3,N], new_xyz [B,3,S], points [B,C,N] or None, idx [B,S,K];
    weights[l] [width_l, width_{l+1}] (input-major, width_0 = 3 + C), scales[l] / shifts[l]
    [width_{l+1}] (the folded eval-mode BatchNorm); 1 to 3 layers -> [B, width_L, S]."""
    x = _f32(xyz, "xyz", 3)
    nx = _f32(new_xyz, "new_xyz", 3)
    ix = _i32(idx, "idx")
    B, c3, N = x.shape
    if c3 != 3 or nx.shape[:2] != (B, 3) or ix.dim() != 3 or ix.shape[:2] != (B, nx.shape[2]):
        raise ValueError("xyz [B,3,N], new_xyz [B,3,S] and idx [B,S,K] expected")
    S, K = ix.shape[1], ix.shape[2]
    f = None
    Cc = 0
    if points is not None:
        f = _f32(points, "points", 3)
        if f.shape[0] != B or f.shape[2] != N:
            raise ValueError("points must be [B, C, N]")
        Cc = f.shape[1]
    L = len(weights)
    if not (1 <= L <= _abi.PN2_MLP_MAX_LAYERS) or len(scales) != L or len(shifts) != L:
        raise ValueError(f"grouped_mlp_max: need 1 to {_abi.PN2_MLP_MAX_LAYERS} layers, each with "
                         f"a weight, a scale and a shift")
    w = [_f32(t, f"weights[{l}]", 2) for l, t in enumerate(weights)]
    sc = [_f32(t, f"scales[{l}]", 1) for l, t in enumerate(scales)]
    sh = [_f32(t, f"shifts[{l}]", 1) for l, t in enumerate(shifts)]
    widths = [3 + Cc]
    for l in range(L):
        if w[l].shape[0] != widths[-1] or sc[l].shape != (w[l].shape[1],) or sh[l].shape != sc[l].shape:
            raise ValueError(f"grouped_mlp_max: layer {l} needs weights [{widths[-1]}, out] and "
                             f"scale / shift [out], got {tuple(w[l].shape)}, {tuple(sc[l].shape)}, "
                             f"{tuple(sh[l].shape)}")
        widths.append(w[l].shape[1])
    out = torch.empty((B, widths[-1], S), dtype=torch.float32, device=x.device)
    bad = _bad_flag(x.device)
    ptrs = ctypes.c_void_p * L
    _check(_abi.lib().ssf_pn2_grouped_mlp_max(
        _stream(x.device), B, N, S, K, Cc, _ptr(x), _ptr(nx), _ptr(f), _ptr(ix), L,
        (ctypes.c_int32 * (L + 1))(*widths), ptrs(*[_ptr(t) for t in w]),
        ptrs(*[_ptr(t) for t in sc]), ptrs(*[_ptr(t) for t in sh]), _ptr(out), _ptr(bad)),
        "grouped_mlp_max")
    _raise_if_bad(bad, check, "grouped_mlp_max")
    return out


def fold_batchnorm(bn):
    """Eval-mode BatchNorm as y = x * scale + shift: scale = gamma / sqrt(var + eps), shift =
    beta - mean * scale, computed in float64 and rounded once to float32."""
    g, b = bn.weight.detach().double(), bn.bias.detach().double()
    scale = g / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = b - bn.running_mean.detach().double() * scale
    return scale.float(), shift.float()


class _FusedMlp(torch.nn.Module):
    """Inference-only base of the two layer types: the (conv, BatchNorm) pairs of the grouped mlp
    are folded once into the kernel's operands and cached until parameters are loaded or moved."""

    def __init__(self):
        super().__init__()
        self._folded = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._drop_folded())

    def _drop_folded(self):
        self._folded = None

    def _apply(self, fn, *args, **kwargs):
        self._folded = None
        return super()._apply(fn, *args, **kwargs)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError(f"{type(self).__name__} is inference-only: batch statistics "
                                      f"are not implemented (call .eval())")
        return super().train(False)

    def _pairs(self):
        raise NotImplementedError

    def _first_layer_rows(self, w):
        return w

    def folded(self):
        """(weights, scales, shifts) of grouped_mlp_max on the parameters' device."""
        if self._folded is None:
            ws, scs, shs = [], [], []
            for l, (conv, bn) in enumerate(self._pairs()):
                w = conv.weight.detach().float().reshape(conv.out_channels, conv.in_channels).t()
                if l == 0:
                    w = self._first_layer_rows(w)
                sc, sh = fold_batchnorm(bn)
                ws.append(w.contiguous())
                scs.append(sc.contiguous())
                shs.append(sh.contiguous())
            self._folded = (ws, scs, shs)
        return self._folded


class SetAbstraction(_FusedMlp):
    """PointNetSetAbstraction (utils.py:185-248; TFlow's sa1 to sa4) for inference.  Parameter
    names are the reference's (mlp_convs.{i}.weight, mlp_bns.{i}.*), so its state_dict loads with
    strict=True.  forward(xyz [B,3,N], points [B,D,N], fps_idx=None) -> (new_xyz [B,3,npoint],
    new_points [B,mlp[-1],npoint], fps_idx): furthest_point_sample, gather_operation and knn,
    then one grouped_mlp_max call.  radius is kept for the signature; the reference groups by
    k-NN and never reads it."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all=False,
                 use_instance_norm=False):
        super().__init__()
        if use_instance_norm:
            raise NotImplementedError("SetAbstraction: use_instance_norm=True is not implemented")
        if not (1 <= len(mlp) <= _abi.PN2_MLP_MAX_LAYERS):
            raise NotImplementedError(f"SetAbstraction: mlp must have 1 to {_abi.PN2_MLP_MAX_LAYERS} layers")
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.mlp_convs = torch.nn.ModuleList()
        self.mlp_bns = torch.nn.ModuleList()
        last = in_channel + 3
        for out_channel in mlp:
            self.mlp_convs.append(torch.nn.Conv2d(last, out_channel, 1, bias=False))
            self.mlp_bns.append(torch.nn.BatchNorm2d(out_channel))
            last = out_channel
        super().train(False)

    def _pairs(self):
        return list(zip(self.mlp_convs, self.mlp_bns))

    def forward(self, xyz, points, fps_idx=None):
        x = _f32(xyz, "xyz", 3)
        xyz_t = x.permute(0, 2, 1).contiguous()
        if fps_idx is None:
            fps_idx = furthest_point_sample(xyz_t, self.npoint)             # utils.py:226
        new_xyz = gather_operation(x, fps_idx)                              # :228
        _, knn_idx = knn(self.nsample, new_xyz.permute(0, 2, 1).contiguous(), xyz_t)   # :229
        w, sc, sh = self.folded()
        return new_xyz, grouped_mlp_max(x, new_xyz, points, knn_idx, w, sc, sh), fps_idx


class SetUpConv(_FusedMlp):
    """PointNetSetUpConv (utils.py:250-315; TFlow's su0 to su3) for inference with knn=True.
    Parameter names are the reference's (mlp1_convs.{i}.{0,1}.*, mlp2_convs.{i}.{0,1}.*).  The
    reference feeds mlp1 cat([feat2_grouped, pos_diff]) (features first, :303); the kernel's
    column order is (pos_diff, features), so the first layer's input rows are permuted once when
    the operands are folded.  mlp2 (pointwise Conv1d + BatchNorm1d + ReLU) runs as torch ops."""

    def __init__(self, nsample, radius, f1_channel, f2_channel, mlp, mlp2, knn=True):
        super().__init__()
        if not knn:
            raise NotImplementedError("SetUpConv: knn=False (ball query) is not implemented")
        if len(mlp) == 0:
            raise NotImplementedError("SetUpConv: an empty mlp is not implemented")
        if len(mlp) > _abi.PN2_MLP_MAX_LAYERS:
            raise NotImplementedError(f"SetUpConv: mlp must have at most {_abi.PN2_MLP_MAX_LAYERS} layers")
        self.nsample, self.radius, self.knn = nsample, radius, knn
        self.mlp1_convs = torch.nn.ModuleList()
        self.mlp2_convs = torch.nn.ModuleList()
        last = f2_channel + 3
        for out_channel in mlp:
            self.mlp1_convs.append(torch.nn.Sequential(torch.nn.Conv2d(last, out_channel, 1, bias=False),
                                                       torch.nn.BatchNorm2d(out_channel),
                                                       torch.nn.ReLU(inplace=False)))
            last = out_channel
        last = mlp[-1] + f1_channel
        for out_channel in mlp2:
            self.mlp2_convs.append(torch.nn.Sequential(torch.nn.Conv1d(last, out_channel, 1, bias=False),
                                                       torch.nn.BatchNorm1d(out_channel),
                                                       torch.nn.ReLU(inplace=False)))
            last = out_channel
        super().train(False)

    def _pairs(self):
        return [(seq[0], seq[1]) for seq in self.mlp1_convs]

    def _first_layer_rows(self, w):
        return torch.cat([w[-3:], w[:-3]], dim=0)            # (features, pos_diff) -> (pos_diff, features)

    def forward(self, pos1, pos2, feature1, feature2, sf1=None, sf2=None):
        if sf1 is not None or sf2 is not None:
            raise NotImplementedError("SetUpConv: sf1 / sf2 are not implemented")
        p1 = _f32(pos1, "pos1", 3)
        p2 = _f32(pos2, "pos2", 3)
        _, idx = knn(self.nsample, p1.permute(0, 2, 1).contiguous(), p2.permute(0, 2, 1).contiguous())  # :291
        w, sc, sh = self.folded()
        feat_new = grouped_mlp_max(p2, p1, feature2, idx, w, sc, sh)        # :296-307
        if feature1 is not None:
            feat_new = torch.cat([feat_new, _f32(feature1, "feature1", 3)], dim=1)   # :310
        for conv in self.mlp2_convs:
            feat_new = conv(feat_new)
        return feat_new

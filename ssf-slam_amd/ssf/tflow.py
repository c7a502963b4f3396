"""The TFlow scene-flow network (scripts/ActiveSceneFlow/TFlowV3_Occlussion_addSeg.py:65-199) on
the GPU, for inference: the cost volume PointConvTransFlowV2 (utils/soflow.py:281-525),
PointWarping (:1222-1257), RefineFlowRegressor (TFlowV3_Occlussion_addSeg.py:41-62) and the
network that joins them with ssf.pointnet2's SetAbstraction / SetUpConv / UpsampleFlow.

    grouped_mlp(...)            ssf_pn2_grouped_mlp: the grouped MLP with a four-segment input
    pair_attention(q, kw)       ssf_pn2_pair_attention: soflow.py:420-458
    segment_softmax_sum(...)    ssf_pn2_segment_softmax_sum: soflow.py:469-486
    segments(idx, n_targets)    CSR (offsets, order) of a scatter index (torch ops)
    cost_volume(params, ...)    PointConvTransFlowV2.forward with both index sets given
    CostVolume, PointWarping, RefineFlowRegressor, TFlow      the reference's modules

Parameter names are the reference's, so its checkpoints load with strict=True.  Inputs are CUDA
tensors; there is no CPU path.  Everything is inference-only (add_Seg_after_FLow = False, the
value at utils/datasets/carla.py:9).
"""
from __future__ import annotations

import ctypes

import torch

from . import _abi
from .frontend import _ptr, _stream
from .pointnet2 import (SetAbstraction, SetUpConv, UpsampleFlow, _bad_flag, _check, _f32, _i32,
                        _raise_if_bad, fold_batchnorm, grouping_operation, knn, three_nn)

__all__ = ["grouped_mlp", "pair_attention", "segment_softmax_sum", "segments", "cost_volume",
           "CostVolume", "PointWarping", "RefineFlowRegressor", "TFlow"]

LEAKY_RATE = 0.1                                  # soflow.py:17


def grouped_mlp(weights, scales, shifts, slopes, idx=None, ctr=None, feat=None, dense=None, xyz=None,
                new_xyz=None, full=False, check=False):
    """ssf_pn2_grouped_mlp.  Per centroid j and sample m the input column is
    cat(ctr[:, j], feat[:, idx[j, m]], dense[:, j, m], xyz[:, idx[j, m]] - new_xyz[:, j]); every
    segment is optional.  ctr [B,Cc,S], feat [B,Cg,N], dense [B,Cd,S,K], xyz [B,3,N] with new_xyz
    [B,3,S], idx [B,S,K] (needed with feat or xyz).  weights[l] [width_l, width_{l+1}] (input-major),
    scales[l] / shifts[l] [width_{l+1}], slopes[l] a float (0 ReLU, 0.1 LeakyReLU, 1 none); 1 to 3
    layers.  -> [B, width_L, S] (the max over K) or, with full=True, [B, width_L, S, K]."""
    B = S = K = None
    ix = None
    if idx is not None:
        ix = _i32(idx, "idx")
        if ix.dim() != 3:
            raise ValueError("idx must be [B, S, K]")
        B, S, K = ix.shape
    d = None
    if dense is not None:
        d = _f32(dense, "dense", 4)
        if B is not None and (d.shape[0], d.shape[2], d.shape[3]) != (B, S, K):
            raise ValueError("dense must be [B, Cd, S, K]")
        B, _, S, K = d.shape
    if B is None:
        raise ValueError("grouped_mlp: idx or dense is needed (they fix S and K)")
    ct = None
    if ctr is not None:
        ct = _f32(ctr, "ctr", 3)
        if (ct.shape[0], ct.shape[2]) != (B, S):
            raise ValueError("ctr must be [B, Cc, S]")
    N = 0
    f = None
    if feat is not None:
        f = _f32(feat, "feat", 3)
        if f.shape[0] != B or ix is None:
            raise ValueError("feat must be [B, Cg, N] and needs idx")
        N = f.shape[2]
    x = nx = None
    if xyz is not None:
        x = _f32(xyz, "xyz", 3)
        nx = _f32(new_xyz, "new_xyz", 3)
        if ix is None or x.shape[:2] != (B, 3) or nx.shape != (B, 3, S) or (f is not None and x.shape[2] != N):
            raise ValueError("xyz [B,3,N], new_xyz [B,3,S] and idx [B,S,K] expected")
        N = x.shape[2]
    L = len(weights)
    if not (1 <= L <= _abi.PN2_MLP_MAX_LAYERS) or not (len(scales) == len(shifts) == len(slopes) == L):
        raise ValueError(f"grouped_mlp: need 1 to {_abi.PN2_MLP_MAX_LAYERS} layers, each with a weight, "
                         f"a scale, a shift and a slope")
    w = [_f32(t, f"weights[{l}]", 2) for l, t in enumerate(weights)]
    sc = [_f32(t, f"scales[{l}]", 1) for l, t in enumerate(scales)]
    sh = [_f32(t, f"shifts[{l}]", 1) for l, t in enumerate(shifts)]
    cc, cg, cd = (0 if t is None else t.shape[1] for t in (ct, f, d))
    widths = [cc + cg + cd + (3 if x is not None else 0)]
    for l in range(L):
        if w[l].shape[0] != widths[-1] or sc[l].shape != (w[l].shape[1],) or sh[l].shape != sc[l].shape:
            raise ValueError(f"grouped_mlp: layer {l} needs weights [{widths[-1]}, out] and scale / shift "
                             f"[out], got {tuple(w[l].shape)}, {tuple(sc[l].shape)}, {tuple(sh[l].shape)}")
        widths.append(w[l].shape[1])
    dev = w[0].device
    out = torch.empty((B, widths[-1], S, K) if full else (B, widths[-1], S), dtype=torch.float32, device=dev)
    bad = _bad_flag(dev)
    ptrs = ctypes.c_void_p * L
    _check(_abi.lib().ssf_pn2_grouped_mlp(
        _stream(dev), B, N, S, K, cc, cg, cd, _ptr(ct), _ptr(f), _ptr(d), _ptr(x), _ptr(nx), _ptr(ix), L,
        (ctypes.c_int32 * (L + 1))(*widths), ptrs(*[_ptr(t) for t in w]), ptrs(*[_ptr(t) for t in sc]),
        ptrs(*[_ptr(t) for t in sh]), (ctypes.c_float * L)(*[float(v) for v in slopes]), int(bool(full)),
        _ptr(out), _ptr(bad)), "grouped_mlp")
    _raise_if_bad(bad, check, "grouped_mlp")
    return out


def pair_attention(q, kw):
    """ssf_pn2_pair_attention (soflow.py:420-458): q, kw [B,C,S,K] -> (qm, kwm) of the same shape,
    with a[m][m'] = sum_ch q[ch][m] kw[ch][m'], W = softmax_m(a) * softmax_m'(a) per centroid,
    qm = q + W kw^T, kwm = kw + q W.  C <= 512, K <= 32."""
    a = _f32(q, "q", 4)
    b = _f32(kw, "kw", 4)
    if a.shape != b.shape:
        raise ValueError("q and kw must have the same [B, C, S, K] shape")
    B, Cc, S, K = a.shape
    qm, kwm = torch.empty_like(a), torch.empty_like(b)
    _check(_abi.lib().ssf_pn2_pair_attention(_stream(a.device), B, Cc, S, K, _ptr(a), _ptr(b), _ptr(qm),
                                             _ptr(kwm)), "pair_attention")
    return qm, kwm


def segment_softmax_sum(logit, val, n_segments, offsets=None, order=None, check=False):
    """ssf_pn2_segment_softmax_sum: logit [B,M], val [B,C,M] -> [B,C,n_segments], the
    softmax-weighted sum of val over each segment.  Without offsets / order the segments are the
    M / n_segments consecutive entries of each centroid; with them (see segments()) segment t is
    order[offsets[t]:offsets[t+1]].  An empty segment gives 0."""
    lg = _f32(logit, "logit", 2)
    v = _f32(val, "val", 3)
    B, M = lg.shape
    if v.shape[0] != B or v.shape[2] != M:
        raise ValueError("logit [B, M] and val [B, C, M] expected")
    T = int(n_segments)
    k = 0
    of = od = None
    if (offsets is None) != (order is None):
        raise ValueError("segment_softmax_sum: offsets and order go together")
    if offsets is not None:
        of, od = _i32(offsets, "offsets"), _i32(order, "order")
        if of.shape != (B, T + 1) or od.shape != (B, M):
            raise ValueError("offsets [B, n_segments + 1] and order [B, M] expected")
    else:
        if T <= 0 or M % T:
            raise ValueError("segment_softmax_sum: uniform segments need M = n_segments * K")
        k = M // T
    out = torch.empty((B, v.shape[1], T), dtype=torch.float32, device=lg.device)
    bad = _bad_flag(lg.device)
    _check(_abi.lib().ssf_pn2_segment_softmax_sum(_stream(lg.device), B, v.shape[1], M, T, k, _ptr(lg),
                                                  _ptr(v), _ptr(of), _ptr(od), _ptr(out), _ptr(bad)),
           "segment_softmax_sum")
    _raise_if_bad(bad, check, "segment_softmax_sum")
    return out


def segments(idx, n_targets):
    """CSR form of the scatter index knn_idxw [B, N1, K] over n_targets targets: (offsets
    [B, n_targets + 1], order [B, N1 * K]) int32 on idx's device, order[b, offsets[b, t] :
    offsets[b, t + 1]] being the flat entries e = j * K + m with idx[b, j, m] == t, ascending (a
    stable sort), so a sum over a segment has one fixed order.  Torch ops (index plumbing)."""
    if not isinstance(idx, torch.Tensor) or idx.dim() != 3:
        raise ValueError("idx must be a [B, N1, K] tensor")
    B = idx.shape[0]
    T = int(n_targets)
    flat = idx.reshape(B, -1).long()
    if bool(((flat < 0) | (flat >= T)).any()):
        raise ValueError("segments: index out of range")
    order = torch.sort(flat, dim=1, stable=True)[1]
    # one bincount for the whole batch: element b counts in [b T, (b + 1) T)
    base = torch.arange(B, device=idx.device)[:, None] * T
    counts = torch.bincount((flat + base).reshape(-1), minlength=B * T).reshape(B, T)
    offsets = torch.zeros((B, T + 1), dtype=torch.long, device=idx.device)
    offsets[:, 1:] = torch.cumsum(counts, dim=1)
    return offsets.to(torch.int32), order.to(torch.int32)


def _conv_rows(conv):
    """a 1x1 convolution's weight as [in, out] float32 (the kernels' input-major layout)"""
    return conv.weight.detach().float().reshape(conv.out_channels, conv.in_channels).t()


def _bias_layers(convs, first_rows=None):
    """(weights, scales, shifts, slopes) of a chain of (1x1 conv with bias, LeakyReLU): the bias
    is the shift under a scale of 1.  first_rows: row permutation of the first layer."""
    ws, scs, shs = [], [], []
    for l, conv in enumerate(convs):
        w = _conv_rows(conv)
        if l == 0 and first_rows is not None:
            w = w[first_rows]
        ws.append(w.contiguous())
        scs.append(torch.ones_like(conv.bias.detach().float()))
        shs.append(conv.bias.detach().float().contiguous())
    return ws, scs, shs, [LEAKY_RATE] * len(ws)


def cost_volume(params, xyz1, xyz2, points1, points2, knn_idx, knn_idxw, sf=None, sf_feat=None):
    """PointConvTransFlowV2.forward (soflow.py:354-525) with both index sets given.

    params: CostVolume.folded().  xyz1 [B,3,N1], xyz2 [B,3,N2], points1 [B,D,N1], points2 [B,D,N2],
    knn_idx / knn_idxw [B,N1,K] into cloud 2 (:384-391, :406), sf [B,3,N1] or None, sf_feat
    [B,F,N1] or None.  Returns (cost_fwd [B,C,N1], cost_bwd [B,C,N2], patch_to_patch_cost
    [B,flow_mlp[-1],N1], flow [B,3,N1]).

    cost_bwd always has N2 columns, zero where no point of cloud 1 chose that target; the
    reference's tensor is max(knn_idxw) + 1 long, because scatter_sum gets no dim_size."""
    x1, x2 = _f32(xyz1, "xyz1", 3), _f32(xyz2, "xyz2", 3)
    p1, p2 = _f32(points1, "points1", 3), _f32(points2, "points2", 3)
    ix, ixw = _i32(knn_idx, "knn_idx"), _i32(knn_idxw, "knn_idxw")
    sff = None if sf_feat is None else _f32(sf_feat, "sf_feat", 3)
    B, _, N1 = x1.shape
    N2 = x2.shape[2]
    # 1. mlp_convs / mlp_convs2 on cat(points1, points2[idx]) (:392-418)
    q = grouped_mlp(*params["mlp1"], idx=ix, ctr=p1, feat=p2, full=True)
    kw = grouped_mlp(*params["mlp2"], idx=ixw, ctr=p1, feat=p2, full=True)
    # 2. the mutual attention (:420-422, :453-458)
    qm, kwm = pair_attention(q, kw)
    # 3. weightnet1 on both mixed tensors (:460-461) -> [B, 1, N1, K]
    wf = grouped_mlp(*params["weightnet"], dense=qm, full=True)
    wfw = grouped_mlp(*params["weightnet"], dense=kwm, full=True)
    # 4. mlp_convs3 on cat(features, sf_feat, direction) of both branches (:424-451); the w branch
    #    takes xyz2, not the warped cloud, at knn_idxw (:407-408)
    cq = grouped_mlp(*params["mlp3"], idx=ix, ctr=sff, dense=q, xyz=x2, new_xyz=x1, full=True)
    ckw = grouped_mlp(*params["mlp3"], idx=ixw, ctr=sff, dense=kw, xyz=x2, new_xyz=x1, full=True)
    # 5. softmax over the samples and the weighted sum (:469, :486); scatter_softmax, product and
    #    scatter_sum over the targets of knn_idxw (:471-481)
    Cc = cq.shape[1]
    cost_fwd = segment_softmax_sum(wf.reshape(B, -1), cq.reshape(B, Cc, -1), N1)
    offsets, order = segments(ixw, N2)
    cost_bwd = segment_softmax_sum(wfw.reshape(B, -1), ckw.reshape(B, Cc, -1), N2, offsets, order)
    # 6. mlp_convs4 on cat(cost_fwd, cost_bwd[idx], sf_feat, direction) and the max (:489-509).
    #    The reference regroups cost_fwd with point_to_patch_cost_fwd.view(B, N1, 1, C) (:490) on the
    #    [B, C, N1] tensor, without a permute: centroid j, channel ch reads flat element j * C + ch of
    #    the [C, N1] plane.  Checkpoints are trained with that, so it is reproduced as written.
    fwd_as_viewed = cost_fwd.reshape(B, N1, Cc).permute(0, 2, 1)
    ctr = fwd_as_viewed.contiguous() if sff is None else torch.cat([fwd_as_viewed, sff], dim=1)
    cost = grouped_mlp(*params["mlp4"], idx=ix, ctr=ctr, feat=cost_bwd, xyz=x2, new_xyz=x1)
    # 7. the flow regressor (:511-525)
    for w, bias in params["flow_mlp"]:
        cost = torch.nn.functional.leaky_relu(torch.nn.functional.conv1d(cost, w, bias), LEAKY_RATE)
    flow = torch.nn.functional.conv1d(cost, *params["fc"]).clamp(-50.0, 50.0)
    if sf is not None:
        flow = flow + _f32(sf, "sf", 3)
    return cost_fwd, cost_bwd, cost, flow.clamp(-50.0, 50.0)


class _Inference(torch.nn.Module):
    """Inference-only module with a cache of folded operands, dropped when parameters are loaded
    or moved (as ssf.pointnet2._FusedMlp)."""

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
            raise NotImplementedError(f"{type(self).__name__} is inference-only (call .eval())")
        return super().train(False)


class _Conv1d(torch.nn.Module):
    """The reference's Conv1d block (soflow.py:1260-1276 with a bias; TFlowV3_Occlussion_addSeg.py
    :22-38 without): composed_module = (Conv1d, Identity, LeakyReLU(0.1))."""

    def __init__(self, in_channels, out_channels, bias):
        super().__init__()
        self.composed_module = torch.nn.Sequential(torch.nn.Conv1d(in_channels, out_channels, 1, bias=bias),
                                                   torch.nn.Identity(), torch.nn.LeakyReLU(LEAKY_RATE))

    def forward(self, x):
        return self.composed_module(x)


class CostVolume(_Inference):
    """PointConvTransFlowV2 (soflow.py:281-525, bn=False, use_leaky=True) for inference, with the
    reference's parameter names: mlp_convs.*, mlp_convs2.*, weightnet1.{0,1,3,4,6}.*,
    mlp_convs3.*, mlp_convs4.*, flow_mlp_convs.{i}.composed_module.0.*, fc.*.
    forward(xyz1 [B,3,N1], xyz2 [B,3,N2], xyz2w [B,3,N2] or None, points1, points2, sf=None,
    sf_feat=None) -> (cost_fwd, cost_bwd, patch_to_patch_cost, flow): see cost_volume()."""

    def __init__(self, nsample, in_channel, sf_channel, mlp, flow_mlp, use_flow=True):
        super().__init__()
        if not (1 <= len(mlp) <= _abi.PN2_MLP_MAX_LAYERS):
            raise NotImplementedError(f"CostVolume: mlp must have 1 to {_abi.PN2_MLP_MAX_LAYERS} layers")
        self.nsample, self.use_flow, self.sf_channel = nsample, use_flow, sf_channel
        nn = torch.nn

        def chain(last):
            convs = nn.ModuleList()
            for out_channel in mlp:
                convs.append(nn.Conv2d(last, out_channel, 1))
                last = out_channel
            return convs

        c = mlp[-1]
        self.mlp_convs = chain(in_channel * 2)
        self.mlp_convs2 = chain(in_channel * 2)
        self.weightnet1 = nn.Sequential(nn.Conv2d(c, c, 1, bias=False), nn.BatchNorm2d(c), nn.ReLU(),
                                        nn.Conv2d(c, c // 2, 1, bias=False), nn.BatchNorm2d(c // 2), nn.ReLU(),
                                        nn.Conv2d(c // 2, 1, 1))
        self.mlp_convs3 = chain(c + sf_channel + 3)
        self.mlp_convs4 = chain(c * 2 + sf_channel + 3)
        self.flow_mlp_convs = nn.ModuleList()
        last = c
        for ch_out in flow_mlp:
            self.flow_mlp_convs.append(_Conv1d(last, ch_out, bias=True))
            last = ch_out
        self.fc = nn.Conv1d(last, 3, 1)
        super().train(False)

    def folded(self):
        """The operands of cost_volume() on the parameters' device: per grouped MLP (weights,
        scales, shifts, slopes); the two row permutations put the reference's concatenation
        orders into the kernel's (ctr, feat, dense, direction) order."""
        if self._folded is None:
            c, f = self.mlp_convs[-1].out_channels, self.sf_channel
            dev = self.fc.weight.device
            r = lambda *spans: torch.cat([torch.arange(a, b, device=dev) for a, b in spans])  # noqa: E731
            # mlp_convs3: (features, sf_feat, direction) (:428-437) -> (sf_feat, features, direction)
            rows3 = r((c, c + f), (0, c), (c + f, c + f + 3))
            # mlp_convs4: (cost_fwd, cost_bwd, sf_feat, direction) (:494-499) -> (cost_fwd, sf_feat,
            # cost_bwd, direction)
            rows4 = r((0, c), (2 * c, 2 * c + f), (c, 2 * c), (2 * c + f, 2 * c + f + 3))
            wn = self.weightnet1
            ws, scs, shs = [], [], []
            for conv, bn in ((wn[0], wn[1]), (wn[3], wn[4])):
                sc, sh = fold_batchnorm(bn)
                ws.append(_conv_rows(conv).contiguous())
                scs.append(sc.contiguous())
                shs.append(sh.contiguous())
            ws.append(_conv_rows(wn[6]).contiguous())
            scs.append(torch.ones_like(wn[6].bias.detach().float()))
            shs.append(wn[6].bias.detach().float().contiguous())
            self._folded = dict(
                mlp1=_bias_layers(self.mlp_convs), mlp2=_bias_layers(self.mlp_convs2),
                weightnet=(ws, scs, shs, [0.0, 0.0, 1.0]),
                mlp3=_bias_layers(self.mlp_convs3, rows3), mlp4=_bias_layers(self.mlp_convs4, rows4),
                flow_mlp=[(m.composed_module[0].weight.detach(), m.composed_module[0].bias.detach())
                          for m in self.flow_mlp_convs],
                fc=(self.fc.weight.detach(), self.fc.bias.detach()))
        return self._folded

    def indices(self, xyz1, xyz2, xyz2w=None, sf=None):
        """(knn_idx, knn_idxw): knn(xyz1 + sf, xyz2) when sf is given and use_flow, else
        knn(xyz1, xyz2) (:384-391); knn(xyz1, xyz2w), xyz2w = xyz2 when None (:372-375, :406)."""
        x1 = _f32(xyz1, "xyz1", 3).permute(0, 2, 1).contiguous()
        x2 = _f32(xyz2, "xyz2", 3).permute(0, 2, 1).contiguous()
        x2w = x2 if xyz2w is None else _f32(xyz2w, "xyz2w", 3).permute(0, 2, 1).contiguous()
        query = x1 + _f32(sf, "sf", 3).permute(0, 2, 1) if (sf is not None and self.use_flow) else x1
        return knn(self.nsample, query.contiguous(), x2)[1], knn(self.nsample, x1, x2w)[1]

    def forward(self, xyz1, xyz2, xyz2w, points1, points2, sf=None, sf_feat=None):
        knn_idx, knn_idxw = self.indices(xyz1, xyz2, xyz2w, sf)
        return cost_volume(self.folded(), xyz1, xyz2, points1, points2, knn_idx, knn_idxw, sf, sf_feat)


class PointWarping(torch.nn.Module):
    """soflow.py:1222-1257 (no parameters): cloud 2 moved back by the flow of cloud 1, interpolated
    with inverse-distance weights over the nsample nearest warped points of cloud 1 (three_nn when
    nsample is None), clamped to [-10, 10].  The device k-NN and grouping_operation, then torch
    arithmetic (upsample_flow stages at most 4096 sparse points; here they are all of cloud 1)."""

    def forward(self, pos1, pos2, flow1=None, nsample=None):
        if flow1 is None:
            return pos2
        p1, p2, fl = _f32(pos1, "pos1", 3), _f32(pos2, "pos2", 3), _f32(flow1, "flow1", 3)
        B, Cc, N2 = p2.shape
        moved = p1 + fl                                                          # :1231
        moved_t = moved.permute(0, 2, 1).contiguous()
        p2_t = p2.permute(0, 2, 1).contiguous()
        if nsample is None:
            nsample = 3
            _, idx = three_nn(p2_t, moved_t)                                     # :1241
        else:
            _, idx = knn(nsample, p2_t, moved_t)                                 # :1243
        rel = grouping_operation(moved, idx) - p2.view(B, Cc, N2, 1)             # :1244
        dist = torch.norm(rel, dim=1).clamp(min=1e-10)
        norm = torch.sum(1.0 / dist, dim=2, keepdim=True)
        weight = (1.0 / dist) / norm
        flow2 = torch.sum(weight.view(B, 1, N2, nsample) * grouping_operation(fl, idx), dim=-1)
        return (p2 - flow2).clamp(-10.0, 10.0)                                   # :1255-1257


class RefineFlowRegressor(torch.nn.Module):
    """TFlowV3_Occlussion_addSeg.py:41-62: PointWarping, then the cost volume (keys under cost.)."""

    def __init__(self, nsample=8, in_channel=128, feat_channel=128, mlp=(128, 128, 128), flow_mlp=(128, 128),
                 use_flow=True):
        super().__init__()
        self.use_flow, self.nsample = use_flow, nsample
        self.cost = CostVolume(nsample, in_channel, feat_channel, list(mlp), list(flow_mlp), use_flow=use_flow)
        self.warping = PointWarping()
        super().train(False)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("RefineFlowRegressor is inference-only (call .eval())")
        return super().train(False)

    def forward(self, pc1, pc2, feats1, feats2, wraping_num=5, c_flow=None, flow_feats=None):
        pc2_warp = None if c_flow is None else self.warping(pc1, pc2, c_flow, wraping_num)
        if self.use_flow:
            return self.cost(pc1, pc2, pc2_warp, feats1, feats2, c_flow, flow_feats)
        return self.cost(pc1, pc2, pc2_warp, feats1, feats2)


class _WideSetUpConv(SetUpConv):
    """SetUpConv whose first mlp1 layer is wider than ssf_pn2_grouped_mlp_max takes (su3: 512
    features + 3 = 515 > 512 rows): the same layers through ssf_pn2_grouped_mlp (up to 766 rows),
    slope 0, max mode.  Its column order (features, direction) is the reference's (utils.py:303),
    so the first layer's rows stay as they are."""

    def _first_layer_rows(self, w):
        return w

    def forward(self, pos1, pos2, feature1, feature2, sf1=None, sf2=None):
        if sf1 is not None or sf2 is not None:
            raise NotImplementedError("SetUpConv: sf1 / sf2 are not implemented")
        p1, p2 = _f32(pos1, "pos1", 3), _f32(pos2, "pos2", 3)
        _, idx = knn(self.nsample, p1.permute(0, 2, 1).contiguous(), p2.permute(0, 2, 1).contiguous())
        w, sc, sh = self.folded()
        feat_new = grouped_mlp(w, sc, sh, [0.0] * len(w), idx=idx, feat=feature2, xyz=p2, new_xyz=p1)
        if feature1 is not None:
            feat_new = torch.cat([feat_new, _f32(feature1, "feature1", 3)], dim=1)
        for conv in self.mlp2_convs:
            feat_new = conv(feat_new)
        return feat_new


class TFlow(torch.nn.Module):
    """The network of TFlowV3_Occlussion_addSeg.py:65-199 for inference; its state-dict keys and
    shapes are the reference's.  forward(pc1 [B,3,N], pc2 [B,3,N], feats1=None, feats2=None) ->
    (flows [full, l1, l2, l3 resolution], fps_inds [l1, l2, l3])."""

    def __init__(self, npoint=8192):
        super().__init__()
        nn = torch.nn
        self.point_conv = nn.Sequential(_Conv1d(3, 32, bias=False), _Conv1d(32, 32, bias=False))
        self.sa1 = SetAbstraction(2048, 0.5, 16, 32, [32, 32, 64])
        self.sa2 = SetAbstraction(512, 2.0, 16, 64, [64, 64, 128])
        self.sa3 = SetAbstraction(256, 4.0, 16, 128, [128, 128, 256])
        self.sa4 = SetAbstraction(128, 8.0, 8, 256, [256, 256, 512])
        self.su3 = _WideSetUpConv(16, 2.4, 256, 512, [256, 256], [256, 256])
        self.flow3_r = RefineFlowRegressor(16, 256, 0, [256, 256], [128, 128], use_flow=False)
        self.su2 = SetUpConv(16, 2.4, 128, 256, [128, 128], [128, 128])
        self.flow2_r = RefineFlowRegressor(16, 128 + 64, 128, [128, 128], [128, 128], use_flow=True)
        self.su1 = SetUpConv(16, 2.4, 64, 128, [64, 64], [64, 64])
        self.flow1_r = RefineFlowRegressor(16, 64 + 32, 128, [64, 64], [64, 64], use_flow=True)
        self.su0 = SetUpConv(16, 2.4, 32, 64, [64, 64], [64, 64])
        self.flow0_r = RefineFlowRegressor(16, 64 + 32, 64, [64, 64], [64, 64], use_flow=True)
        self.flow_up_sample = UpsampleFlow()
        self.deconv3_2 = _Conv1d(256, 64, bias=False)
        self.deconv2_1 = _Conv1d(128, 32, bias=False)
        self.deconv1_0 = _Conv1d(64, 32, bias=False)
        super().train(False)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("TFlow is inference-only (call .eval())")
        return super().train(False)

    @torch.no_grad()
    def forward(self, pc1, pc2, feats1=None, feats2=None):
        pc1, pc2 = _f32(pc1, "pc1", 3), _f32(pc2, "pc2", 3)
        if feats1 is None or feats2 is None:                                     # :112-117
            feats1, feats2 = self.point_conv(pc1), self.point_conv(pc2)
        else:
            feats1, feats2 = self.point_conv(_f32(feats1, "feats1", 3)), self.point_conv(_f32(feats2, "feats2", 3))
        up = self.flow_up_sample
        l1_pc1, l1_feats1, l1_fps1 = self.sa1(pc1, feats1)
        l1_pc2, l1_feats2, _ = self.sa1(pc2, feats2)
        l2_pc1, l2_feats1, l2_fps1 = self.sa2(l1_pc1, l1_feats1)
        l2_pc2, l2_feats2, _ = self.sa2(l1_pc2, l1_feats2)
        l3_pc1, l3_feats1, l3_fps1 = self.sa3(l2_pc1, l2_feats1)
        l3_pc2, l3_feats2, _ = self.sa3(l2_pc2, l2_feats2)
        l4_pc1, l4_feats1, _ = self.sa4(l3_pc1, l3_feats1)
        l4_pc2, l4_feats2, _ = self.sa4(l3_pc2, l3_feats2)

        l3_4_feats1 = self.su3(l3_pc1, l4_pc1, l3_feats1, l4_feats1)
        l3_4_feats2 = self.su3(l3_pc2, l4_pc2, l3_feats2, l4_feats2)
        fwd_l3, bwd_l3, l3_feats, l3_flow = self.flow3_r(l3_pc1, l3_pc2, l3_4_feats1, l3_4_feats2, 3)

        l2_3_feats1 = self.su2(l2_pc1, l3_pc1, l2_feats1, l3_4_feats1)
        l2_3_feats2 = self.su2(l2_pc2, l3_pc2, l2_feats2, l3_4_feats2)
        l2_coarse_sf = up(l2_pc1, l3_pc1, l3_flow, k=5)
        l2_3_feats_sf = up(l2_pc1, l3_pc1, l3_feats, k=5)
        fwd = torch.cat([l2_3_feats1, self.deconv3_2(up(l2_pc1, l3_pc1, fwd_l3))], dim=1)
        bwd = torch.cat([l2_3_feats2, self.deconv3_2(up(l2_pc1, l3_pc1, bwd_l3))], dim=1)   # :146, as written
        fwd_l2, bwd_l2, l2_feats_sf, l2_flow = self.flow2_r(l2_pc1, l2_pc2, fwd, bwd, 5, l2_coarse_sf,
                                                            l2_3_feats_sf)

        l1_2_feats1 = self.su1(l1_pc1, l2_pc1, l1_feats1, l2_3_feats1)
        l1_2_feats2 = self.su1(l1_pc2, l2_pc2, l1_feats2, l2_3_feats2)
        l1_coarse_sf = up(l1_pc1, l2_pc1, l2_flow, k=5)
        l1_2_feats_sf = up(l1_pc1, l2_pc1, l2_feats_sf, k=5)
        fwd = torch.cat([l1_2_feats1, self.deconv2_1(up(l1_pc1, l2_pc1, fwd_l2))], dim=1)
        bwd = torch.cat([l1_2_feats2, self.deconv2_1(up(l1_pc1, l2_pc1, bwd_l2))], dim=1)
        fwd_l1, bwd_l1, l1_feats_sf, l1_flow = self.flow1_r(l1_pc1, l1_pc2, fwd, bwd, 7, l1_coarse_sf,
                                                            l1_2_feats_sf)

        l0_1_feats1 = self.su0(pc1, l1_pc1, feats1, l1_2_feats1)
        l0_1_feats2 = self.su0(pc2, l1_pc2, feats2, l1_2_feats2)
        l0_1_feats_sf = up(pc1, l1_pc1, l1_feats_sf, k=7)
        l0_coarse_sf = up(pc1, l1_pc1, l1_flow, k=7)
        fwd = torch.cat([l0_1_feats1, self.deconv1_0(up(pc1, l1_pc1, fwd_l1))], dim=1)
        bwd = torch.cat([l0_1_feats2, self.deconv1_0(up(pc1, l1_pc1, bwd_l1))], dim=1)
        _, _, _, flow = self.flow0_r(pc1, pc2, fwd, bwd, 7, l0_coarse_sf, l0_1_feats_sf)
        return [flow, l1_flow, l2_flow, l3_flow], [l1_fps1, l2_fps1, l3_fps1]

"""numpy float64 restatement of the three cost-volume kernels (ssf_pn2_grouped_mlp,
ssf_pn2_pair_attention, ssf_pn2_segment_softmax_sum, include/ssf_pointnet2.h), of
ssf.tflow.cost_volume and of PointWarping -- the yardstick of tests/test_cv_host.py and
tests/test_gpu_cv.py for the cases that have no fixture.  tests/test_cv_host.py ties it to the
reference: it reproduces the float64 outputs of the reference's own PointConvTransFlowV2 and
PointWarping in tests/golden/cv_ref.npz.

Everything is evaluated in float64 on the arrays it is given (float32 inputs are converted
exactly), in the order of PointConvTransFlowV2.forward, utils/soflow.py:354-525.  Layouts are the
package's: grouped tensors are [B, C, S, K].

seed_state() is the one weight generator of the fixtures and the tests.
"""
from __future__ import annotations

import numpy as np

LEAKY = 0.1


def _f(a):
    return None if a is None else np.asarray(a, np.float64)


def _gather(feat, idx):
    """feat [B, C, N], idx [B, S, K] -> [B, C, S, K]; an index outside [0, N) reads as index 0"""
    feat = _f(feat)
    idx = np.asarray(idx, np.int64)
    N = feat.shape[2]
    idx = np.where((idx < 0) | (idx >= N), 0, idx)
    return np.stack([feat[b][:, idx[b]] for b in range(feat.shape[0])])


def grouped_input(idx=None, ctr=None, feat=None, dense=None, xyz=None, new_xyz=None):
    """cat(ctr[:, j], feat[:, idx], dense, xyz[:, idx] - new_xyz[:, j]) -> [B, C0, S, K]"""
    K = (np.asarray(idx) if idx is not None else np.asarray(dense)).shape[-1]
    cols = []
    if ctr is not None:
        cols.append(np.repeat(_f(ctr)[:, :, :, None], K, axis=3))
    if feat is not None:
        cols.append(_gather(feat, idx))
    if dense is not None:
        cols.append(_f(dense))
    if xyz is not None:
        cols.append(_gather(xyz, idx) - _f(new_xyz)[:, :, :, None])
    return np.concatenate(cols, axis=1)


def layers(x, weights, scales, shifts, slopes):
    """x [B, C0, S, K]; per layer t = (W^T x) * scale + shift, y = t > 0 ? t : slope * t"""
    for w, sc, sh, sl in zip(weights, scales, shifts, slopes):
        t = np.einsum("io,bisk->bosk", _f(w), x)
        t = t * _f(sc)[None, :, None, None] + _f(sh)[None, :, None, None]
        x = np.where(t > 0, t, float(sl) * t)
    return x


def grouped_mlp(weights, scales, shifts, slopes, idx=None, ctr=None, feat=None, dense=None, xyz=None,
                new_xyz=None, full=False):
    y = layers(grouped_input(idx, ctr, feat, dense, xyz, new_xyz), weights, scales, shifts, slopes)
    return y if full else y.max(axis=-1)


def _softmax(a, axis):
    e = np.exp(a - a.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def pair_attention(q, kw):
    """q, kw [B, C, S, K] -> (qm, kwm): soflow.py:420-422, :453-458"""
    q, kw = _f(q), _f(kw)
    a = np.einsum("bcsm,bcsn->bsmn", q, kw)                       # a[m][m']
    w = _softmax(a, 2) * _softmax(a, 3)                           # over m, times over m'
    qm = q + np.einsum("bsmn,bcsn->bcsm", w, kw)
    kwm = kw + np.einsum("bcsm,bsmn->bcsn", q, w)
    return qm, kwm


def segments(idx, n_targets):
    """CSR of the scatter index [B, N1, K]: (offsets [B, T + 1], order [B, N1 * K]), entries of a
    segment ascending (numpy stable argsort)."""
    idx = np.asarray(idx, np.int64)
    B = idx.shape[0]
    flat = idx.reshape(B, -1)
    order = np.stack([np.argsort(flat[b], kind="stable") for b in range(B)])
    offsets = np.zeros((B, n_targets + 1), np.int64)
    for b in range(B):
        offsets[b, 1:] = np.cumsum(np.bincount(flat[b], minlength=n_targets))
    return offsets.astype(np.int32), order.astype(np.int32)


def segment_softmax_sum(logit, val, n_segments, offsets=None, order=None):
    """logit [B, M], val [B, C, M] -> [B, C, n_segments]; an order entry outside [0, M) reads as
    entry 0 (the header's convention); an empty segment gives 0."""
    logit, val = _f(logit), _f(val)
    B, M = logit.shape
    out = np.zeros((B, val.shape[1], n_segments))
    for b in range(B):
        for t in range(n_segments):
            if offsets is None:
                k = M // n_segments
                e = np.arange(t * k, (t + 1) * k)
            else:
                e = np.asarray(order[b, offsets[b, t]:offsets[b, t + 1]], np.int64)
                e = np.where((e < 0) | (e >= M), 0, e)
            if e.size:
                w = np.exp(logit[b, e] - logit[b, e].max())
                out[b, :, t] = val[b][:, e] @ (w / w.sum())
    return out


def fold_batchnorm(gamma, beta, mean, var, eps=1e-5):
    gamma, beta, mean, var = (_f(a) for a in (gamma, beta, mean, var))
    scale = gamma / np.sqrt(var + eps)
    return scale, beta - mean * scale


def _rows(state, key):
    w = _f(state[key])
    return w.reshape(w.shape[0], w.shape[1]).T                    # [in, out]


def _chain(state, prefix, n, rows=None):
    ws = [_rows(state, f"{prefix}.{i}.weight") for i in range(n)]
    if rows is not None:
        ws[0] = ws[0][rows]
    shs = [_f(state[f"{prefix}.{i}.bias"]) for i in range(n)]
    return ws, [np.ones_like(s) for s in shs], shs, [LEAKY] * n


def cost_volume(state, n_mlp, n_flow, xyz1, xyz2, points1, points2, knn_idx, knn_idxw, sf=None, sf_feat=None):
    """ssf.tflow.cost_volume from a PointConvTransFlowV2 state dict (numpy arrays), with the
    kernel's column orders -> (cost_fwd [B,C,N1], cost_bwd [B,C,N2], cost, flow)."""
    B, _, N1 = np.asarray(xyz1).shape
    N2 = np.asarray(xyz2).shape[2]
    c = state[f"mlp_convs.{n_mlp - 1}.weight"].shape[0]
    f = 0 if sf_feat is None else np.asarray(sf_feat).shape[1]
    q = grouped_mlp(*_chain(state, "mlp_convs", n_mlp), idx=knn_idx, ctr=points1, feat=points2, full=True)
    kw = grouped_mlp(*_chain(state, "mlp_convs2", n_mlp), idx=knn_idxw, ctr=points1, feat=points2, full=True)
    qm, kwm = pair_attention(q, kw)
    wn = "weightnet1"
    s0 = fold_batchnorm(*(state[f"{wn}.1.{n}"] for n in ("weight", "bias", "running_mean", "running_var")))
    s1 = fold_batchnorm(*(state[f"{wn}.4.{n}"] for n in ("weight", "bias", "running_mean", "running_var")))
    b6 = _f(state[f"{wn}.6.bias"])
    wnet = ([_rows(state, f"{wn}.0.weight"), _rows(state, f"{wn}.3.weight"), _rows(state, f"{wn}.6.weight")],
            [s0[0], s1[0], np.ones_like(b6)], [s0[1], s1[1], b6], [0.0, 0.0, 1.0])
    wf = grouped_mlp(*wnet, dense=qm, full=True)
    wfw = grouped_mlp(*wnet, dense=kwm, full=True)
    ar = np.arange
    rows3 = np.concatenate([ar(c, c + f), ar(0, c), ar(c + f, c + f + 3)])
    rows4 = np.concatenate([ar(0, c), ar(2 * c, 2 * c + f), ar(c, 2 * c), ar(2 * c + f, 2 * c + f + 3)])
    m3 = _chain(state, "mlp_convs3", n_mlp, rows3)
    cq = grouped_mlp(*m3, idx=knn_idx, ctr=sf_feat, dense=q, xyz=xyz2, new_xyz=xyz1, full=True)
    ckw = grouped_mlp(*m3, idx=knn_idxw, ctr=sf_feat, dense=kw, xyz=xyz2, new_xyz=xyz1, full=True)
    cost_fwd = segment_softmax_sum(wf.reshape(B, -1), cq.reshape(B, c, -1), N1)
    offsets, order = segments(knn_idxw, N2)
    cost_bwd = segment_softmax_sum(wfw.reshape(B, -1), ckw.reshape(B, c, -1), N2, offsets, order)
    # the reference's point_to_patch_cost_fwd.view(B, N1, 1, C) on a [B, C, N1] tensor (:490), as written
    viewed = cost_fwd.reshape(B, N1, c).transpose(0, 2, 1)
    ctr = viewed if sf_feat is None else np.concatenate([viewed, _f(sf_feat)], axis=1)
    cost = grouped_mlp(*_chain(state, "mlp_convs4", n_mlp, rows4), idx=knn_idx, ctr=ctr, feat=cost_bwd,
                       xyz=xyz2, new_xyz=xyz1)
    for i in range(n_flow):
        p = f"flow_mlp_convs.{i}.composed_module.0"
        t = np.einsum("oi,bin->bon", _f(state[p + ".weight"])[:, :, 0], cost) + _f(state[p + ".bias"])[None, :, None]
        cost = np.where(t > 0, t, LEAKY * t)
    flow = np.einsum("oi,bin->bon", _f(state["fc.weight"])[:, :, 0], cost) + _f(state["fc.bias"])[None, :, None]
    flow = np.clip(flow, -50.0, 50.0)
    if sf is not None:
        flow = flow + _f(sf)
    return cost_fwd, cost_bwd, cost, np.clip(flow, -50.0, 50.0)


def point_warping(pos1, pos2, flow1, idx):
    """PointWarping.forward (soflow.py:1222-1257) with the k-NN indices [B, N2, nsample] given"""
    pos1, pos2, flow1 = _f(pos1), _f(pos2), _f(flow1)
    rel = _gather(pos1 + flow1, idx) - pos2[:, :, :, None]
    dist = np.maximum(np.sqrt((rel * rel).sum(axis=1)), 1e-10)
    weight = (1.0 / dist) / (1.0 / dist).sum(axis=2, keepdims=True)
    flow2 = (weight[:, None] * _gather(flow1, idx)).sum(axis=-1)
    return np.clip(pos2 - flow2, -10.0, 10.0)


def seed_state(keys_and_shapes, seed):
    """{key: array} from numpy.random.default_rng(seed), drawn in sorted-key order: running_var ~
    U(0.5, 2); convolution weights (two or more dimensions) ~ N(0, 1) / sqrt(fan-in); BatchNorm
    weight (one dimension) ~ U(0.5, 1.5); num_batches_tracked = 0; every other tensor ~ N(0, 0.2).
    Floating-point tensors are float32."""
    rng = np.random.default_rng(int(seed))
    state = {}
    for key, shape in sorted((str(k), tuple(int(d) for d in s)) for k, s in keys_and_shapes):
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            state[key] = np.zeros(shape, np.int64)
        elif leaf == "running_var":
            state[key] = rng.uniform(0.5, 2.0, shape).astype(np.float32)
        elif leaf == "weight" and len(shape) >= 2:
            state[key] = (rng.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))).astype(np.float32)
        elif leaf == "weight":
            state[key] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        else:
            state[key] = (rng.standard_normal(shape) * 0.2).astype(np.float32)
    return state

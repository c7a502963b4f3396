"""numpy float64 restatement of ssf_pn2_grouped_mlp_max (include/ssf_pointnet2.h) and of the two
modules built on it -- the yardstick of tests/test_sa_host.py and tests/test_gpu_sa.py for the
cases that have no fixture.  tests/test_sa_host.py ties it to the reference: it reproduces the
float64 outputs of the reference's own modules in tests/golden/sa_ref.npz.

Everything is evaluated in float64 on the arrays it is given (float32 inputs are converted
exactly), in the order of PointNetSetAbstraction.forward, utils/utils.py:231-247: gather,
relative coordinates, per layer matmul, scale and shift, ReLU, then the max over the samples.
"""
from __future__ import annotations

import numpy as np


def group_relative(xyz, new_xyz, feat, idx):
    """cat(xyz[:, idx] - new_xyz[..., None], feat[:, idx]) -> [B, 3 + C, S, K]; an index outside
    [0, N) reads as index 0 (the header's convention)."""
    xyz = np.asarray(xyz, np.float64)
    new_xyz = np.asarray(new_xyz, np.float64)
    idx = np.asarray(idx, np.int64)
    B, _, N = xyz.shape
    idx = np.where((idx < 0) | (idx >= N), 0, idx)
    cols = []
    for b in range(B):
        g = xyz[b][:, idx[b]] - new_xyz[b][:, :, None]                 # [3, S, K]
        if feat is not None:
            g = np.concatenate([g, np.asarray(feat[b], np.float64)[:, idx[b]]], axis=0)
        cols.append(g)
    return np.stack(cols)


def mlp_max(x, weights, scales, shifts):
    """x [B, C0, S, K]; weights[l] [C_l, C_{l+1}] (input-major) -> [B, C_L, S]."""
    for w, sc, sh in zip(weights, scales, shifts):
        y = np.einsum("io,bisk->bosk", np.asarray(w, np.float64), x)
        y = y * np.asarray(sc, np.float64)[None, :, None, None] + np.asarray(sh, np.float64)[None, :, None, None]
        x = np.maximum(y, 0.0)
    return x.max(axis=-1)


def grouped_mlp_max(xyz, new_xyz, feat, idx, weights, scales, shifts):
    return mlp_max(group_relative(xyz, new_xyz, feat, idx), weights, scales, shifts)


def fold_batchnorm(gamma, beta, mean, var, eps=1e-5):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale, in float64."""
    gamma, beta, mean, var = (np.asarray(a, np.float64) for a in (gamma, beta, mean, var))
    scale = gamma / np.sqrt(var + eps)
    return scale, beta - mean * scale


def _folded(state, conv, bn):
    w = np.asarray(state[conv + ".weight"], np.float64)
    w = w.reshape(w.shape[0], w.shape[1]).T                              # [in, out]
    sc, sh = fold_batchnorm(state[bn + ".weight"], state[bn + ".bias"], state[bn + ".running_mean"],
                            state[bn + ".running_var"])
    return w, sc, sh


def set_abstraction(state, n_layers, xyz, points, fps_idx, knn_idx):
    """PointNetSetAbstraction.forward with given FPS and k-NN indices -> (new_xyz, new_points)."""
    xyz64 = np.asarray(xyz, np.float64)
    new_xyz = np.stack([xyz64[b][:, fps_idx[b]] for b in range(xyz64.shape[0])])
    ops = [_folded(state, f"mlp_convs.{i}", f"mlp_bns.{i}") for i in range(n_layers)]
    return new_xyz, grouped_mlp_max(xyz, new_xyz, points, knn_idx, *zip(*ops))


def set_upconv(state, n_mlp, n_mlp2, pos1, pos2, feature1, feature2, knn_idx):
    """PointNetSetUpConv.forward (knn=True, no sf1 / sf2) with given k-NN indices.  The reference
    concatenates [feat2_grouped, pos_diff] (utils.py:303): the first layer's input rows are
    moved to the (pos_diff, features) order of group_relative."""
    ops = [_folded(state, f"mlp1_convs.{i}.0", f"mlp1_convs.{i}.1") for i in range(n_mlp)]
    w0 = ops[0][0]
    ops[0] = (np.concatenate([w0[-3:], w0[:-3]], axis=0),) + ops[0][1:]
    y = grouped_mlp_max(pos2, pos1, feature2, knn_idx, *zip(*ops))       # [B, C, N1]
    if feature1 is not None:
        y = np.concatenate([y, np.asarray(feature1, np.float64)], axis=1)
    for i in range(n_mlp2):
        w, sc, sh = _folded(state, f"mlp2_convs.{i}.0", f"mlp2_convs.{i}.1")
        y = np.einsum("io,bin->bon", w, y) * sc[None, :, None] + sh[None, :, None]
        y = np.maximum(y, 0.0)
    return y

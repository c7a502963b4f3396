"""The accumulated map cloud of mapOptmization (src/mapOptmization.cpp: mapCloudPtr).

updateKeyPose (:296-312) transforms a keyframe's plane cloud by its key pose and appends it to
the map; correctPoses (:315-332) clears the map and rebuilds it from every keyframe when a loop
has closed; publishResult (:387-397) sends its 0.4 m VoxelGrid on /sum_map_cloud_res3.

``MapCloud`` keeps the keyframe clouds and the map on the device: two parallel float4 buffers
over one offset table, ``raw`` (the keyframe clouds as received) and ``mapped`` (the same points
in the map frame).  Appending a keyframe and rebuilding all of them are the same call,
``transform(first, last, Ts)``: one ssf_transform_clouds_batch launch (loop.hip) from ``raw``
into ``mapped`` at the same offsets.  Capacity grows geometrically with the contents kept;
between growths nothing is allocated.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _abi, loop
from .frontend import Frontend, _ptr, _stream

DEFAULT_CAPACITY_POINTS = 1 << 21        # 512 keyframes of 4096 plane points: 2 x 32 MiB
DEFAULT_CAPACITY_KEYFRAMES = 512


def pose_rows(Ts) -> np.ndarray:
    """Poses as [n, 4, 4], [n, 3, 4] or [n, 12] -> [n, 12] float64: the top three rows of each
    4x4, row-major (R[r][0], R[r][1], R[r][2], t[r]), as ssf_transform_clouds_batch reads them."""
    T = np.asarray(Ts, np.float64)
    if T.ndim == 3 and T.shape[1:] == (4, 4):
        T = T[:, :3, :]
    return np.ascontiguousarray(T.reshape(-1, 12))


class MapCloud:
    """Device-resident keyframe store plus the map built from it."""

    def __init__(self, fe: Frontend, capacity_points: int = DEFAULT_CAPACITY_POINTS,
                 capacity_keyframes: int = DEFAULT_CAPACITY_KEYFRAMES):
        self.fe = fe
        dev = fe.device
        cap, kcap = max(int(capacity_points), 1), max(int(capacity_keyframes), 1)
        self.raw = torch.empty((cap, 4), dtype=torch.float32, device=dev)
        self.mapped = torch.empty((cap, 4), dtype=torch.float32, device=dev)
        self.h_off = torch.zeros(kcap + 1, dtype=torch.int64)
        self.d_off = torch.zeros(kcap + 1, dtype=torch.int64, device=dev)
        self.d_T = torch.zeros((kcap, 12), dtype=torch.float64, device=dev)
        self.n_keyframes = 0
        self.n_points = 0
        self.generation = 0              # bumped when raw / mapped move to a larger buffer

    @property
    def capacity_points(self) -> int:
        return int(self.raw.shape[0])

    def _grow_points(self, need: int):
        cap = self.capacity_points
        while cap < need:
            cap *= 2
        n = self.n_points
        for name in ("raw", "mapped"):
            old = getattr(self, name)
            new = torch.empty((cap, 4), dtype=torch.float32, device=old.device)
            new[:n].copy_(old[:n])
            setattr(self, name, new)
        self.generation += 1

    def _grow_keyframes(self):
        kcap = 2 * int(self.d_T.shape[0])
        k = self.n_keyframes
        h = torch.zeros(kcap + 1, dtype=torch.int64)
        h[:k + 1].copy_(self.h_off[:k + 1])
        d = torch.zeros(kcap + 1, dtype=torch.int64, device=self.d_off.device)
        d[:k + 1].copy_(self.d_off[:k + 1])
        self.h_off, self.d_off = h, d
        self.d_T = torch.zeros((kcap, 12), dtype=torch.float64, device=self.d_T.device)

    def store(self, xyzi: torch.Tensor) -> torch.Tensor:
        """Copy one keyframe cloud ([m, 4] float32 on the device) into ``raw`` -> its view there.
        The keyframe joins ``points()`` once ``transform`` has covered it."""
        if not (xyzi.is_cuda and xyzi.dtype == torch.float32 and xyzi.dim() == 2 and xyzi.shape[1] == 4):
            raise _abi.SSFError("MapCloud.store: expected an [m, 4] float32 CUDA tensor")
        m, n, k = int(xyzi.shape[0]), self.n_points, self.n_keyframes
        if n + m > self.capacity_points:
            self._grow_points(n + m)
        if k + 1 > int(self.d_T.shape[0]):
            self._grow_keyframes()
        view = self.raw[n:n + m]
        view.copy_(xyzi)
        self.h_off[k + 1] = n + m
        self.d_off[k + 1:k + 2].copy_(self.h_off[k + 1:k + 2])
        self.n_keyframes, self.n_points = k + 1, n + m
        return view

    def keyframe(self, k: int) -> torch.Tensor:
        """The stored cloud of keyframe k (a view of ``raw``)."""
        if not 0 <= k < self.n_keyframes:
            raise IndexError(k)
        return self.raw[int(self.h_off[k]):int(self.h_off[k + 1])]

    def transform(self, first: int, last: int, Ts):
        """Keyframes [first, last) from ``raw`` into ``mapped`` by the poses Ts (last - first of
        them, see pose_rows): one launch."""
        n = last - first
        if not 0 <= first <= last <= self.n_keyframes:
            raise ValueError(f"MapCloud.transform: keyframes [{first}, {last}) of {self.n_keyframes}")
        if n == 0:
            return
        T = pose_rows(Ts)
        if T.shape[0] != n:
            raise ValueError(f"MapCloud.transform: {T.shape[0]} poses for {n} keyframes")
        self.d_T[first:last].copy_(torch.from_numpy(T))
        rc = _abi.lib().ssf_transform_clouds_batch(
            self.fe._h, _stream(self.fe.device), n, _ptr(self.raw),
            C.c_void_p(self.d_off.data_ptr() + 8 * first), C.c_void_p(self.h_off.data_ptr() + 8 * first),
            C.c_void_p(self.d_T.data_ptr() + 96 * first), _ptr(self.mapped))
        self.fe._check(rc, "ssf_transform_clouds_batch")

    def points(self) -> torch.Tensor:
        """The map (mapCloudPtr): keyframe order, input order within a keyframe."""
        return self.mapped[:self.n_points]

    def filtered(self, leaf: float = 0.4) -> torch.Tensor:
        """downSizeFilterMap (:390-391): the VoxelGrid of the map."""
        if self.n_points == 0:
            return torch.zeros((0, 4), dtype=torch.float32, device=self.fe.device)
        return loop.voxel_grid_one(self.fe, self.points(), leaf)

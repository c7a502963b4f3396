"""The ActiveSceneFlow chain on the device: a pair of scans -> the loader's
subsample (ssf_subsample_batch) -> TFlow -> the network's own flow -> the dynamic-point mask ->
the float32 Kabsch pose, as scripts/ActiveSceneFlow/main_sju_occ_ros.py:146-296 and
main_sju_occ_addSeg_ros.py run it per test pair.

    subsample(fe, ...)        ssf_subsample_batch: utils/datasets/carla.py:179-200, 236-250, 274-285
    load_checkpoint(net, p)   main_sju_occ_ros.py:698-711 (DataParallel `module.` keys accepted)
    flow_metrics(pred, gt)    error(), main_sju_occ_ros.py:112-143
    flow_mask_pose(net, ...)  net(pc1, pc2)[0][0] -> the ASF block (:257-284 / addSeg :277-290)
    ActiveSceneFlowNode       the data-source node of run_noSeg_ActiveSceneFlow.launch /
                              run_Seg_ActiveSceneFlow.launch

Inputs are CUDA tensors; there is no CPU path.  No trained weights ship with the project: a
checkpoint is the caller's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _abi
from . import io as sio
from ._abi import SSFError
from .frontend import Frontend, _ptr, _stream, frame_offsets
from .nodes import Float64MultiArray

RM_GROUND_Z = -3.3                      # carla.py:237, 242
HYBRID_QUOTA = 100                      # carla.py:249-250
STAGE_TWO_TAG = 1 << 63
SAMPLE_STATUS = {_abi.SAMPLE_EMPTY: "no point survives the cut",
                 _abi.SAMPLE_SHORT: "the background holds fewer points than the quota leaves to it "
                                    "(the reference's np.random.choice raises here)"}


def subsample(fe: Frontend, pts, off, h_off, nb, seed, tags=None, cls=None, z_min=None, quota=-1,
              key_bits=32, want_xyz=True):
    """ssf_subsample_batch for F frames packed in pts [total, stride] f32 at offsets off / h_off:
    per frame nb points by the seeded keys of (seed, tag) -- tags [F] (default: the frame's
    position) -- among the points with !(z < z_min) (z_min None: all), with the foreground quota
    when quota >= 0 (cls [total] uint8, 0 = background).
    -> (idx [F, nb] int32, xyz [F, 3, nb] f32 or None, n [F] int32 survivors, status [F] int32
    (_abi.SAMPLE_*)), all on the device; nothing synchronises."""
    pts = fe._dev(pts, torch.float32)
    if pts.dim() != 2:
        raise ValueError("pts must be [total, stride]")
    off = fe._dev(off, torch.int64)
    F = h_off.numel() - 1
    if off.numel() != F + 1:
        raise ValueError(f"off has {off.numel()} entries for {F} frames")
    total = int(h_off[-1])
    if pts.shape[0] < total:
        raise ValueError(f"pts has {pts.shape[0]} points, the offsets end at {total}")
    if cls is not None:
        cls = fe._dev(cls, torch.uint8)
        if cls.numel() < total:
            raise ValueError(f"cls has {cls.numel()} entries for {total} points")
    h_off64 = h_off.to(torch.int64).contiguous()
    h_tag = None
    if tags is not None:
        h_tag = np.ascontiguousarray(np.array([int(t) & (2 ** 64 - 1) for t in tags], dtype=np.uint64))
        if h_tag.size != F:
            raise ValueError(f"{h_tag.size} tags for {F} frames")
    nbc = max(int(nb), 0)
    dev = fe.device
    idx = torch.empty((F, nbc), dtype=torch.int32, device=dev)
    xyz = torch.empty((F, 3, nbc), dtype=torch.float32, device=dev) if want_xyz else None
    n = torch.empty(max(F, 1), dtype=torch.int32, device=dev)
    status = torch.empty(max(F, 1), dtype=torch.int32, device=dev)
    rc = _abi.lib().ssf_subsample_batch(
        fe._h, _stream(dev), F, _ptr(pts), int(pts.shape[1]), _ptr(off), C.c_void_p(h_off64.data_ptr()),
        _ptr(cls), int(nb), float(RM_GROUND_Z if z_min is None else z_min), 0 if z_min is None else 1,
        int(quota), int(seed) & (2 ** 64 - 1), None if h_tag is None else h_tag.ctypes.data_as(C.c_void_p),
        int(key_bits), _ptr(idx), _ptr(xyz), _ptr(n), _ptr(status))
    fe._check(rc, "ssf_subsample_batch")
    return idx, xyz, n[:F], status[:F]


def load_checkpoint(net, path):
    """Load a torch.load-able state dict with the reference's keys into `net`, strict=True.  The
    reference's checkpoints are saved from a DataParallel wrapper (main_sju_occ_ros.py:698-711):
    a leading `module.` on the keys is dropped."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or not all(isinstance(k, str) for k in sd):
        raise ValueError(f"{path}: not a state dict")
    if sd and all(k.startswith("module.") for k in sd):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    net.load_state_dict(sd, strict=True)
    return net


def flow_metrics(pred, gt, mask=None):
    """error() of main_sju_occ_ros.py:112-143 as device torch ops, in float64 on the float32
    inputs: pred / gt [B, 3, N], mask [B, N] (or [B, N, 1]) or None = ones.
    -> dict(epe3d, acc3d_strict, acc3d_relax, outlier) of python floats (one host copy)."""
    p = pred.permute(0, 2, 1).to(torch.float64)
    g = gt.permute(0, 2, 1).to(torch.float64)
    if mask is None:
        m = torch.ones(p.shape[:2], dtype=torch.float64, device=p.device)
    else:
        m = mask.reshape(p.shape[0], p.shape[1]).to(torch.float64)
    l2 = torch.linalg.vector_norm(g - p, dim=-1) * m                          # :120-124
    sf = torch.linalg.vector_norm(g, dim=-1) * m
    msum = m.sum(1)
    epe = (l2.sum(1) / (msum + 1e-10)).mean()                                  # :127-128
    rel = l2 / (sf + 1e-10)                                                    # :130
    on = m != 0

    def ratio(a, b):                                                           # :132-141
        cnt = ((a & on) | (b & on)).sum(1).to(torch.float64)
        keep = msum > 0
        return (cnt[keep] / msum[keep]).mean()

    vals = torch.stack([epe, ratio(l2 < 0.05, rel < 0.05), ratio(l2 < 0.1, rel < 0.1),
                        ratio(l2 >= 0.3, rel >= 0.1)]).cpu().tolist()
    return dict(zip(("epe3d", "acc3d_strict", "acc3d_relax", "outlier"), vals))


def flow_mask_pose(net, fe: Frontend, pc1, pc2, mode="gmm", fg1=None, seed=None, draws=None,
                   errors="status"):
    """The network and the ASF block for B pairs: flow = net(pc1, pc2)[0][0] (pc1 / pc2 [B, 3, N]
    f32), then on the points and the flow as [B N, 3] f32 the mask kernel and the float32 Kabsch
    on the same stream -- what ssf.mask_and_pose(..., kabsch_dtype="float32") runs.
    mode "gmm": main_sju_occ_ros.py:257-284 (draws [B, 3]: the k-means++ doubles; None: the
    context's RandomState, seeded here when seed is given); "gt": background = fg1 == 0 (fg1
    [B, N]), main_sju_occ_addSeg_ros.py:277-290.
    errors "status": nothing goes to the host, out[:, 16] holds every pair's status; "raise": the
    statuses are read and a failed pair raises as ssf.mask_and_pose does.
    -> (out [B, 32] f64 (_abi.POSE_OUT), bg_mask [B N] uint8, flow [B, 3, N] f32)."""
    if mode not in ("gmm", "gt"):
        raise ValueError(f"mode {mode!r}: 'gmm' or 'gt'")
    if errors not in ("raise", "status"):
        raise ValueError(f"errors must be 'raise' or 'status', not {errors!r}")
    # One forward per pair, as the reference's node runs it: every pair then goes through the same
    # shapes whatever the batch, so its pose cannot depend on what else is in the batch.  (A B = 2
    # forward was once seen 2e-7 away from the two single forwards -- the network's torch
    # convolutions may choose another algorithm for another shape -- and three later runs gave
    # identical bits)
    flow = torch.cat([net(pc1[b:b + 1], pc2[b:b + 1])[0][0] for b in range(pc1.shape[0])])
    B, _, N = flow.shape
    pts = pc1.permute(0, 2, 1).reshape(B * N, 3).to(torch.float32).contiguous()
    fl = flow.permute(0, 2, 1).reshape(B * N, 3).contiguous()
    off, h_off = frame_offsets([N] * B, fe.device)
    m = None
    if mode == "gt":
        if fg1 is None:
            raise ValueError("mode 'gt' needs fg1")
        m = (fg1.reshape(B * N) != 0).to(torch.uint8).contiguous()
    if seed is not None:
        fe.seed(seed)
    out, bg = fe.mask_pose(pts, fl, off, h_off, mode=mode, mask_in=m, draws=draws)
    fe.kabsch_f32(pts, off, h_off, flow=fl, mask=bg, out=out)
    if errors == "raise":
        from .pose import _raise_status
        for st in out[:, _abi.POSE_OUT["STATUS"]].cpu().tolist():
            if int(st) != 0:
                _raise_status(st)
    return out, bg, flow


class ActiveSceneFlowNode:
    """The data-source node of run_noSeg_ActiveSceneFlow.launch (mode 'gmm', main_sju_occ_ros.py)
    and run_Seg_ActiveSceneFlow.launch (mode 'gt', main_sju_occ_addSeg_ros.py), for one pair of
    scans: subsample both clouds to n_points, publish the sampled cloud 1 on /velodyne_points
    (xyz, point_step 12, frame livox_frame), run the network and the ASF block, publish
    /frame_odom1 = [t, q].

    reference_loader with both foreground masks: the reference's two stages -- the hybrid quota
    of 100 to n_points (carla.py:249-250), then the choice to n_points, which on exactly n_points
    survivors resamples with replacement (:276-277).  Otherwise the second stage alone.  Tags:
    2 pair_index + cloud for stage one, the same + 2^63 for stage two.  rm_ground: the
    !(z < -3.3) cut of carla.py:236-246, in the first stage that runs."""

    def __init__(self, publish, net, frontend: Frontend | None = None, mode: str = "gmm",
                 n_points: int = 8192, seed: int = 1234, reference_loader: bool = True,
                 rm_ground: bool = False, device=None):
        if mode not in ("gmm", "gt"):
            raise ValueError(f"mode {mode!r}")
        self.fe = frontend or Frontend(64, device=device)
        self.publish = publish
        self.net = net
        self.mode = mode
        self.n_points = int(n_points)
        self.seed = int(seed)
        self.reference_loader = bool(reference_loader)
        self.rm_ground = bool(rm_ground)
        self.pair_index = 0
        self.last = None                # the last pair's device tensors (indices, flow, mask)
        self.fe.seed(self.seed)         # the GMM's k-means++ RandomState

    def _f32(self, a):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32))
        return t.to(self.fe.device, torch.float32).contiguous()

    def _mask(self, a):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return (t.to(self.fe.device).reshape(-1) != 0).to(torch.uint8).contiguous()

    def sample(self, pos1, pos2, fg1=None, fg2=None):
        """-> (idx [2, n_points] int64 into the raw clouds, xyz [2, 3, n_points] f32, status [k, 2]
        int32 of the k stages run), on the device"""
        fe, nb = self.fe, self.n_points
        p1, p2 = self._f32(pos1)[:, :3], self._f32(pos2)[:, :3]
        pts = torch.cat([p1, p2]).contiguous()
        off, h_off = frame_offsets([p1.shape[0], p2.shape[0]], fe.device)
        tags = [2 * self.pair_index, 2 * self.pair_index + 1]
        z_min = RM_GROUND_Z if self.rm_ground else None
        stats = []
        base = None
        if self.reference_loader and fg1 is not None and fg2 is not None:
            cls = torch.cat([self._mask(fg1), self._mask(fg2)])
            idx1, _, _, st = subsample(fe, pts, off, h_off, nb, self.seed, tags=tags, cls=cls, z_min=z_min,
                                       quota=HYBRID_QUOTA, want_xyz=False)
            stats.append(st)
            base = idx1.long()
            pts = pts[(base + off[:2, None]).reshape(-1)].contiguous()      # the stage-one clouds
            off, h_off = frame_offsets([nb, nb], fe.device)
            z_min = None
        idx2, xyz, _, st = subsample(fe, pts, off, h_off, nb, self.seed,
                                     tags=[t + STAGE_TWO_TAG for t in tags], z_min=z_min)
        stats.append(st)
        idx = idx2.long() if base is None else torch.gather(base, 1, idx2.long())
        return idx, xyz, torch.stack(stats)

    def on_pair(self, pos1, pos2, stamp=(0, 0), fg1=None, fg2=None, gt_flow=None):
        """-> (pose row [32] f64 numpy (_abi.POSE_OUT), flow metrics against gt_flow[idx1] or None)"""
        if self.mode == "gt" and fg1 is None:
            raise SSFError("mode 'gt' needs the foreground mask of cloud 1 (s_fg_mask)")
        idx, xyz, st = self.sample(pos1, pos2, fg1, fg2)
        self.pair_index += 1
        cloud1 = xyz[0].t().contiguous().cpu().numpy()          # the published cloud; synchronises
        for row in st.cpu().tolist():
            for c, s in enumerate(row):
                if s != _abi.SAMPLE_OK:
                    raise SSFError(f"subsample of cloud {c + 1}: {SAMPLE_STATUS.get(s, s)}")
        self.publish("/velodyne_points", sio.xyz_to_cloud(cloud1, stamp, "livox_frame"))
        fg_s = None if fg1 is None else self._mask(fg1)[idx[0]][None]
        out, bg, flow = flow_mask_pose(self.net, self.fe, xyz[0:1], xyz[1:2], mode=self.mode,
                                       fg1=fg_s if self.mode == "gt" else None)
        o = out[0].cpu().numpy()
        self.publish("/frame_odom1", Float64MultiArray([float(v) for v in o[0:7]]))   # hstack((t, q)) :282-284
        self.last = dict(idx=idx, xyz=xyz, flow=flow, bg_mask=bg, fg1=fg_s)
        metrics = None
        if gt_flow is not None:
            gt = self._f32(gt_flow)[:, :3][idx[0]].t()[None]
            metrics = flow_metrics(flow, gt)
        return o, metrics

"""Loop-closure registration of mapOptmization (src/mapOptmization.cpp).

GPU work goes through the C ABI (loop.hip): ``voxel_grid`` <- pcl::VoxelGrid<PointXYZI>::filter
(downSizeFilterICP 0.1 m :214-217, downSizeFilterMap 0.4 m :406-409) and ``icp`` <-
pcl::IterativeClosestPoint<PointXYZI, PointXYZI> (:224-238).  ``LoopCloser`` mirrors the
keyframe / loop-detection / local-map logic around them (isKeyFrame :129-144,
addPose3D6D :78-107, detectLoopFrameID :167-197, getLoopLocalMap :200-218, addLoopFactor
:221-272, trans_loop_adjust :325, the T_map_0_curr chain :447-450) and emits the loop
constraint the reference adds to its GTSAM graph (BetweenFactor poseFrom.between(poseTo),
noise = the ICP fitness score).  By default the published pose is the loop-adjusted odometry;
``LoopCloser(optimize=True)`` also records the factors of addOdomFactor (:147-165), optimises
the pose graph on the GPU at every loop closure (``optimize_pose_graphs`` <- runOptimize
:280-293, batched Gauss-Newton in pose_graph.hip, not GTSAM's iSAM2) and rewrites every
keyframe pose (correctPoses :296-332); ``robust=pgo_robust("huber")`` puts
a robust loss on the loop edges of those solves and ``lm=pgo_lm()`` Levenberg-Marquardt step
control under them (``pgo=pgo_params(...)`` their iteration limit).  ``LoopCloser(map_cloud=True)`` also keeps the
accumulated map cloud (mapCloudPtr: updateKeyPose :309-311, the rebuild of
correctPoses :320-325) on the device in an ``ssf.MapCloud``; a new keyframe
goes into the map at its stored key pose (the reference places it at its iSAM2 estimate).
``LoopCloser(detector="scan_context")`` replaces the radius search of detectLoopFrameID, which
finds nothing once the odometry has drifted past its 15 m, by place recognition on Scan Context
descriptors of the raw scans (``ssf.scan_context``); the default stays the radius.
With ``sc_candidates=K`` > 1 the K best places are verified by ICP in one batch (``local_maps``,
``icp_batch``) and the one the geometry likes best closes the loop.

Pose helpers restate pcl/common/eigen.h: getTransformation (roll/pitch/yaw -> affine,
yaw * pitch * roll) and getTranslationAndEulerAngles.  Key poses are stored in float, as the
reference's PointXYZIRPYT cloud holds them.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _abi
from .frontend import Frontend, _ptr, _stream


# --------------------------------------------------------------------------- pose helpers
def get_transformation(x, y, z, roll, pitch, yaw):
    """pcl::getTransformation (pcl/common/impl/eigen.hpp) in double -> 4x4."""
    A, B = math.cos(yaw), math.sin(yaw)
    Cc, D = math.cos(pitch), math.sin(pitch)
    E, F = math.cos(roll), math.sin(roll)
    DE, DF = D * E, D * F
    return np.array([[A * Cc, A * DF - B * E, B * F + A * DE, x],
                     [B * Cc, A * E + B * DF, B * DE - A * F, y],
                     [-D, Cc * F, Cc * E, z],
                     [0.0, 0.0, 0.0, 1.0]], np.float64)


def get_translation_and_euler_angles(t):
    """pcl::getTranslationAndEulerAngles -> (x, y, z, roll, pitch, yaw)."""
    return (float(t[0, 3]), float(t[1, 3]), float(t[2, 3]), math.atan2(t[2, 1], t[2, 2]),
            math.asin(-t[2, 0]), math.atan2(t[1, 0], t[0, 0]))


def pose_from_quat(q_xyzw, t):
    """Eigen::Affine3d: rotate(q) then pretranslate(t) (mapOptmization.cpp:447-449)."""
    x, y, z, w = (float(v) for v in q_xyzw)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(t, np.float64)
    return T


def between(a, b):
    """gtsam Pose3 a.between(b) = a^-1 b (4x4)."""
    return np.linalg.inv(a) @ b


# --------------------------------------------------------------------------- GPU entry points
def voxel_grid(fe: Frontend, xyzi: torch.Tensor, off: torch.Tensor, h_off: torch.Tensor, leaf: float):
    """Batched pcl::VoxelGrid: float4 clouds at offsets -> (centroids at the same offsets,
    per-cloud counts (device int32))."""
    F = int(h_off.numel()) - 1
    out = torch.empty_like(xyzi)
    cnt = torch.zeros(max(F, 0), dtype=torch.int32, device=xyzi.device)
    ho = h_off.contiguous()
    fe._check(_abi.lib().ssf_voxel_grid_batch(fe._h, _stream(fe.device), F, _ptr(xyzi), _ptr(off),
                                              C.c_void_p(ho.data_ptr()), float(leaf), _ptr(out), _ptr(cnt)),
              "ssf_voxel_grid_batch")
    return out, cnt


def voxel_grid_one(fe: Frontend, xyzi: torch.Tensor, leaf: float) -> torch.Tensor:
    """One cloud through the batched filter (the mapOptmization call shape)."""
    n = int(xyzi.shape[0])
    h = torch.tensor([0, n], dtype=torch.int64)
    out, cnt = voxel_grid(fe, xyzi.contiguous(), h.to(xyzi.device), h, leaf)
    return out[: int(cnt[0])]


def icp_params(max_iter=100, max_corr_dist=50.0, trans_eps=1e-6, fit_eps=1e-6):
    p = _abi.IcpParams()
    _abi.lib().ssf_icp_params_default(C.byref(p))
    p.max_iter, p.max_corr_dist, p.trans_eps, p.fit_eps = int(max_iter), float(max_corr_dist), float(trans_eps), float(fit_eps)
    return p


def icp_batch(fe: Frontend, src, src_off, h_src_off, tgt, tgt_off, h_tgt_off, params=None, guess=None):
    """Batched ICP -> list of dicts (T 4x4 float32, fitness, converged, iterations, state, n_corr)."""
    P = int(h_src_off.numel()) - 1
    params = params or icp_params()
    out = np.zeros(P * _abi.ICP_OUT_STRIDE, np.float64)
    g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(-1)
    hs, ht = h_src_off.contiguous(), h_tgt_off.contiguous()
    fe._check(_abi.lib().ssf_icp_batch(fe._h, _stream(fe.device), P, _ptr(src), _ptr(src_off),
                                       C.c_void_p(hs.data_ptr()), _ptr(tgt), _ptr(tgt_off),
                                       C.c_void_p(ht.data_ptr()), C.byref(params),
                                       None if g is None else g.ctypes.data_as(C.c_void_p),
                                       out.ctypes.data_as(C.c_void_p)), "ssf_icp_batch")
    res = []
    for k in range(P):
        o = out[k * _abi.ICP_OUT_STRIDE:(k + 1) * _abi.ICP_OUT_STRIDE]
        res.append(dict(T=o[0:16].astype(np.float32).reshape(4, 4), fitness=float(o[16]),
                        converged=bool(o[17]), iterations=int(o[18]),
                        state=_abi.ICP_STATES[int(o[19])], n_corr=int(o[20])))
    return res


def icp(fe: Frontend, src: torch.Tensor, tgt: torch.Tensor, params=None, guess=None):
    """One problem: icp.setInputSource(src); setInputTarget(tgt); align()."""
    hs = torch.tensor([0, int(src.shape[0])], dtype=torch.int64)
    ht = torch.tensor([0, int(tgt.shape[0])], dtype=torch.int64)
    return icp_batch(fe, src.contiguous(), hs.to(src.device), hs, tgt.contiguous(), ht.to(tgt.device),
                     ht, params, None if guess is None else [guess])[0]


def pgo_params(max_iter=8, func_tol=1e-6):
    p = _abi.PgoParams()
    _abi.lib().ssf_pgo_params_default(C.byref(p))
    p.max_iter, p.func_tol = int(max_iter), float(func_tol)
    return p


def pgo_robust(kind, k=None):
    """The loss on the loop edges of a pose graph (ssf_pgo_robust; what GTSAM's
    noiseModel::Robust does to a loop factor): kind "none", "huber", "cauchy" or "geman_mcclure",
    k its threshold (default: GTSAM's, 1.345 / 0.1 / 1.0)."""
    if not isinstance(kind, str) or kind not in _abi.PGO_ROBUST_KINDS:
        raise ValueError(f"pgo_robust: kind is one of {', '.join(_abi.PGO_ROBUST_KINDS)}, not {kind!r}")
    r = _abi.PgoRobust()
    if _abi.lib().ssf_pgo_robust_default(_abi.PGO_ROBUST_KINDS[kind], C.byref(r)) != _abi.SSF_OK:
        raise ValueError(f"pgo_robust: kind {kind!r} rejected")
    if k is not None:
        try:
            k = float(k)
        except (TypeError, ValueError):
            raise ValueError(f"pgo_robust: k must be a number, not {k!r}") from None
        if kind != "none" and not (math.isfinite(k) and k > 0.0):
            raise ValueError(f"pgo_robust: k must be finite and positive, not {k!r}")
        r.k = k
    return r


def parse_robust(text):
    """"KIND[:K]" (the --map-robust / --robust command-line form) -> pgo_robust(KIND, K)."""
    kind, sep, k = str(text).partition(":")
    if sep and not k:
        raise ValueError(f"robust loss {text!r}: nothing after the colon")
    return pgo_robust(kind, k if sep else None)


def pgo_lm(radius0=1e4, min_relative_decrease=1e-3, max_radius=1e16, min_radius=1e-32):
    """Levenberg-Marquardt step control for the pose-graph solve (ssf_pgo_lm; Ceres'
    LevenbergMarquardtStrategy and its defaults): no step is taken that raises the cost."""
    p = _abi.PgoLm()
    _abi.lib().ssf_pgo_lm_default(C.byref(p))
    try:
        vals = [float(v) for v in (radius0, min_relative_decrease, max_radius, min_radius)]
    except (TypeError, ValueError):
        raise ValueError("pgo_lm: the parameters are numbers") from None
    p.radius0, p.min_relative_decrease, p.max_radius, p.min_radius = vals
    if not all(math.isfinite(v) and v > 0.0 for v in (p.radius0, p.max_radius, p.min_radius)):
        raise ValueError("pgo_lm: radius0, max_radius and min_radius must be finite and positive")
    if p.min_radius > p.max_radius:
        raise ValueError("pgo_lm: min_radius is above max_radius")
    if not 0.0 <= p.min_relative_decrease < 1.0:
        raise ValueError("pgo_lm: min_relative_decrease must lie in [0, 1)")
    return p


def parse_lm(text):
    """The value of --map-lm[=RADIUS0] (True: no value) -> pgo_lm(RADIUS0)."""
    if text is True:
        return pgo_lm()
    try:
        r0 = float(text)
    except (TypeError, ValueError):
        raise ValueError(f"step control {text!r}: RADIUS0 must be a number") from None
    return pgo_lm(radius0=r0)


def optimize_pose_graphs(fe: Frontend, graphs, params=None, robust=None, edge_out=False, lm=None,
                         lm_log=False):
    """Batched pose-graph optimisation, one launch for every graph of the list.  A graph is a
    dict(poses [K, 7] f64 (q xyzw, t), edge_ij [E, 2] graph-local, edge_meas [E, 7], edge_var
    [E, 6] (rotation then translation), prior_pose [7], prior_var [6] on node 0).
    -> list of dict(poses [K, 7], status (PGO_*), status_name, iterations, cost0, cost, dx, loops,
    cost_log).  A graph whose status is not ok / converged gets its poses back unchanged.
    robust (pgo_robust): a loss on the loop edges (|i - j| != 1); with it or with edge_out every
    result also carries edge_weight [E] and edge_chi2 [E] (the unweighted squared whitened
    residual) of the evaluation `cost` belongs to, NaN for a graph that failed.
    lm (pgo_lm): Levenberg-Marquardt step control; params.max_iter then bounds the attempts,
    iterations counts them, poses / cost / dx belong to the last accepted point, cost_log never
    rises, and every result also holds accepted (the accepted attempts) and radius (the final
    trust-region radius).  lm_log (needs lm): also lm_log [attempts, 4], per attempt the trial cost,
    the model's decrease, the radius after it and the outcome (PGO_LM_LOG / PGO_LM_*)."""
    if lm_log and lm is None:
        raise ValueError("lm_log is the log of the step control: it needs lm")
    G = len(graphs)
    if G == 0:
        return []
    params = params or pgo_params()
    with_edges = robust is not None or bool(edge_out)
    f64 = lambda key, w: [np.ascontiguousarray(g[key], np.float64).reshape(-1, w) for g in graphs]  # noqa: E731
    poses, meas, var = f64("poses", 7), f64("edge_meas", 7), f64("edge_var", 6)
    ij = [np.ascontiguousarray(g["edge_ij"], np.int32).reshape(-1, 2) for g in graphs]
    for k in range(G):
        if not (len(ij[k]) == len(meas[k]) == len(var[k])):
            raise ValueError(f"graph {k}: edge_ij, edge_meas and edge_var differ in length")
    prior = np.concatenate(f64("prior_pose", 7))
    pvar = np.concatenate(f64("prior_var", 6))
    if prior.shape != (G, 7) or pvar.shape != (G, 6):
        raise ValueError("prior_pose is 7 and prior_var 6 doubles per graph")
    h_noff = torch.tensor(np.concatenate([[0], np.cumsum([len(p) for p in poses])]), dtype=torch.int32)
    h_eoff = torch.tensor(np.concatenate([[0], np.cumsum([len(e) for e in ij])]), dtype=torch.int32)
    dev = fe.device

    def up(parts, dtype, width):                  # never a null pointer, even with nothing in it
        a = np.concatenate(parts + [np.zeros((1, width), dtype)])
        return torch.from_numpy(a).to(dev)

    d_pose, d_meas, d_var = up(poses, np.float64, 7), up(meas, np.float64, 7), up(var, np.float64, 6)
    d_ij = up(ij, np.int32, 2)
    d_prior, d_pvar = torch.from_numpy(prior).to(dev), torch.from_numpy(pvar).to(dev)
    d_noff, d_eoff = h_noff.to(dev), h_eoff.to(dev)
    stats = torch.zeros(G, _abi.PGO_OUT_STRIDE, dtype=torch.float64, device=dev)
    clog = torch.zeros(G, params.max_iter + 1, dtype=torch.float64, device=dev)
    args = (fe._h, _stream(dev), G, _ptr(d_pose), _ptr(d_noff), C.c_void_p(h_noff.data_ptr()), _ptr(d_ij),
            _ptr(d_meas), _ptr(d_var), _ptr(d_eoff), C.c_void_p(h_eoff.data_ptr()), _ptr(d_prior), _ptr(d_pvar),
            C.byref(params), _ptr(stats), _ptr(clog))
    if lm is not None:
        eout = (torch.zeros(int(h_eoff[-1]) + 1, _abi.PGO_EDGE_OUT_STRIDE, dtype=torch.float64, device=dev)
                if with_edges else None)
        llog = (torch.zeros(G, max(params.max_iter, 1), _abi.PGO_LM_LOG_STRIDE, dtype=torch.float64, device=dev)
                if lm_log else None)
        fe._check(_abi.lib().ssf_pose_graph_batch_lm(*args, None if robust is None else C.byref(robust),
                                                     None if eout is None else _ptr(eout), C.byref(lm),
                                                     None if llog is None else _ptr(llog)),
                  "ssf_pose_graph_batch_lm")
        eo = None if eout is None else eout.cpu().numpy()
        ll = None if llog is None else llog.cpu().numpy()
    elif with_edges:
        eout = torch.zeros(int(h_eoff[-1]) + 1, _abi.PGO_EDGE_OUT_STRIDE, dtype=torch.float64, device=dev)
        fe._check(_abi.lib().ssf_pose_graph_batch_robust(*args, None if robust is None else C.byref(robust),
                                                         _ptr(eout)), "ssf_pose_graph_batch_robust")
        eo = eout.cpu().numpy()
    else:
        fe._check(_abi.lib().ssf_pose_graph_batch(*args), "ssf_pose_graph_batch")
    out_pose, st, cl = d_pose.cpu().numpy(), stats.cpu().numpy(), clog.cpu().numpy()
    res = []
    for k in range(G):
        o = st[k]
        status = int(o[_abi.PGO_OUT["STATUS"]])
        res.append(dict(poses=out_pose[int(h_noff[k]):int(h_noff[k + 1])].copy(), status=status,
                        status_name=_abi.PGO_STATUS.get(status, "?"),
                        iterations=int(o[_abi.PGO_OUT["ITERATIONS"]]), cost0=float(o[_abi.PGO_OUT["COST0"]]),
                        cost=float(o[_abi.PGO_OUT["COST"]]), dx=float(o[_abi.PGO_OUT["DX"]]),
                        loops=int(o[_abi.PGO_OUT["LOOPS"]]),
                        cost_log=[float(v) for v in cl[k] if not math.isnan(v)]))
        if with_edges:
            rows = eo[int(h_eoff[k]):int(h_eoff[k + 1])]
            res[-1].update(edge_weight=rows[:, _abi.PGO_EDGE_OUT["WEIGHT"]].copy(),
                           edge_chi2=rows[:, _abi.PGO_EDGE_OUT["CHI2"]].copy())
        if lm is not None:
            res[-1].update(accepted=int(o[_abi.PGO_OUT["ACCEPTED"]]), radius=float(o[_abi.PGO_OUT["RADIUS"]]))
            if lm_log:
                res[-1]["lm_log"] = ll[k, :res[-1]["iterations"]].copy()
    return res


def pose7_from_matrix(T):
    """4x4 -> (q xyzw, t), 7 doubles (the largest-component branch of the usual conversion)."""
    R = np.asarray(T, np.float64)[:3, :3]
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.asarray(q, np.float64)
    return np.concatenate([q / np.linalg.norm(q), np.asarray(T, np.float64)[:3, 3]])


PRIOR_VARIANCES = (1e-2, 1e-2, math.pi * math.pi, 1e8, 1e8, 1e8)      # priorNoise (:151)
ODOM_VARIANCES = (1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4)                  # odometryNoise (:160)


def transform_cloud(xyzi: torch.Tensor, T) -> torch.Tensor:
    """pcl::transformPointCloud with an Affine3d: double arithmetic, float result, intensity
    kept."""
    Td = torch.as_tensor(np.asarray(T, np.float64), device=xyzi.device)
    p = xyzi[:, :3].double()
    out = xyzi.clone()
    out[:, :3] = (p @ Td[:3, :3].T + Td[:3, 3]).float()
    return out


# --------------------------------------------------------------------------- keyframe logic
@dataclass
class LoopConstraint:
    key_cur: int
    key_pre: int
    between: np.ndarray          # poseFrom.between(poseTo), 4x4
    noise: float                 # ICP fitness score (diagonal variances, :257-259)
    correction: np.ndarray       # correctionLidarFrame, 4x4
    shift: int | None = None     # detector="scan_context": the column shift of the match (yaw = shift * 6 deg)
    dist: float | None = None    # and its Scan Context distance
    # sc_candidates > 1: every candidate ICP verified, in rank order, as
    # (key_pre, dist, shift, fitness, converged); key_pre / dist / shift above are the chosen one's
    candidates: list | None = None


@dataclass
class LoopCloser:
    """The mapOptmization state machine for one sequence (keyframes, loop detection, ICP)."""
    fe: Frontend
    icp_leaf: float = 0.1
    radius: float = 15.0
    time_gap: float = 20.0
    search_num: int = 10
    key6d: list = field(default_factory=list)          # float32 [x, y, z, roll, pitch, yaw] + time
    key_frames: list = field(default_factory=list)     # device float4 plane clouds
    loop_index: dict = field(default_factory=dict)
    loop_record_index: int = 0
    trans_loop_adjust: np.ndarray = field(default_factory=lambda: np.eye(4))
    constraints: list = field(default_factory=list)
    # optimize=True: the pose graph the reference keeps in GTSAM (addOdomFactor :147-165, the loop
    # factor :274), solved on the GPU at every loop closure
    optimize: bool = False
    graph_init: list = field(default_factory=list)     # per keyframe: the estimate, 7 doubles
    graph_edges: list = field(default_factory=list)    # (i, j, measurement 7 doubles, 6 variances)
    graph_prior: np.ndarray | None = None
    last_optimization: dict | None = None
    # a loss on the loop edges of every solve (pgo_robust); the solves then also report the
    # weight of every edge (loop_weights).  Nothing is rejected: a down-weighted loop stays in
    # the graph and its correction stays in trans_loop_adjust
    robust: object | None = None
    # step control of every solve (pgo_lm), and the parameters of the solves (pgo_params; None:
    # the defaults, max_iter 8 -- few attempts for step control from a far start)
    lm: object | None = None
    pgo: object | None = None
    # map_cloud=True: the keyframe clouds live in a device store and the accumulated map
    # (mapCloudPtr, updateKeyPose :309-311) is kept equal to every keyframe under its current key
    # pose: appended per keyframe, rebuilt in one launch when the poses are rewritten
    map_cloud: bool = False
    map: object | None = None                          # ssf.MapCloud when map_cloud, else None
    # detector="radius": detectLoopFrameID's radius search over the estimated key positions (the
    # reference; it finds nothing once odometry has drifted past `radius`).  "scan_context": place
    # recognition by appearance (ssf.scan_context): every keyframe's descriptor is
    # computed from the frame's raw scan (process(scan=...)) and kept on the device, a new keyframe is
    # compared with every keyframe of the eligible prefix, and a candidate is accepted when its
    # distance is below sc.threshold (sc: ssf.scan_context.sc_params; None: the defaults)
    detector: str = "radius"
    sc: object | None = None
    sc_db: object | None = None                        # ssf.scan_context.ScanContextDB
    sc_match: tuple | None = None                      # (key_pre, dist, shift) of the last accepted match
    # detector="scan_context", sc_candidates = K > 1: the nearest descriptor is often not the best
    # place, so the K best places (ScanContextDB.query_topk; no two within
    # sc_exclusion keyframes of each other, None: search_num, closer ones share a local map) are
    # verified by ICP in one batch and the best fitness wins.  1: the single nearest, as before
    sc_candidates: int = 1
    sc_exclusion: int | None = None

    def __post_init__(self):
        if self.detector not in ("radius", "scan_context"):
            raise ValueError(f"LoopCloser: detector is radius or scan_context, not {self.detector!r}")
        k, e = self.sc_candidates, self.sc_exclusion
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _abi.SC_MAX_TOPK:
            raise ValueError(f"LoopCloser: sc_candidates is an integer in 1 .. {_abi.SC_MAX_TOPK}, not {k!r}")
        if e is not None and (isinstance(e, bool) or not isinstance(e, (int, np.integer)) or e < 0):
            raise ValueError(f"LoopCloser: sc_exclusion is a non-negative integer or None, not {e!r}")
        if self.detector != "scan_context" and (k != 1 or e is not None):
            raise ValueError("LoopCloser: sc_candidates and sc_exclusion belong to detector=\"scan_context\"")
        if self.detector == "scan_context":
            from .scan_context import ScanContextDB, sc_params
            if self.sc is None:
                self.sc = sc_params()
            if self.sc_db is None:
                self.sc_db = ScanContextDB(self.fe)
        elif self.sc is not None:
            raise ValueError("LoopCloser: sc belongs to detector=\"scan_context\"")
        if self.map_cloud and self.map is None:
            from .map_cloud import MapCloud
            self.map = MapCloud(self.fe)

    def _store_key_frame(self, plane_xyzi):
        """keyFrameVector.push_back (:406) into the map's store: key_frames[k] is its view there."""
        gen = self.map.generation
        self.key_frames.append(self.map.store(plane_xyzi))
        if self.map.generation != gen:                 # the store moved: drop the views of the old one
            self.key_frames[:] = [self.map.keyframe(k) for k in range(self.map.n_keyframes)]

    def rebuild_map(self):
        """mapCloudPtr->clear() and updateKeyPose for every keyframe (:320-325), one launch."""
        K = self.map.n_keyframes
        self.map.transform(0, K, [self._T6(i) for i in range(K)])

    def _T6(self, i):
        p = self.key6d[i]
        return get_transformation(*(float(v) for v in p[:6]))

    def is_key_frame(self, T_map_0_curr):
        """isKeyFrame (:129-144)."""
        if not self.key6d:
            return True
        tb = np.linalg.inv(self._T6(-1)) @ T_map_0_curr
        x, y, z, r, p, yw = get_translation_and_euler_angles(tb)
        return not (abs(r) < 0.01 and abs(p) < 0.01 and abs(yw) < 0.01 and math.sqrt(x * x + y * y + z * z) < 1)

    def detect_loop(self):
        """detectLoopFrameID (:167-197): radius search over key positions (nearest first).
        detector="scan_context": the nearest descriptor of the eligible prefix instead."""
        cur = len(self.key6d) - 1
        if cur in self.loop_index:
            return None
        if self.detector == "scan_context":
            return self._detect_loop_scan_context(cur)
        pos = np.array([k[:3] for k in self.key6d], np.float32)
        d2 = ((pos - pos[cur]) ** 2).sum(1)
        cand = np.nonzero(d2 < np.float32(self.radius * self.radius))[0]   # FLANN: dist < r^2
        cand = cand[np.lexsort((cand, d2[cand]))]
        pre = -1
        for i in cand:
            if abs(self.key6d[i][6] - self.key6d[cur][6]) > self.time_gap:
                pre = int(i)
                break
        if pre == -1 or pre == cur:
            return None
        self.loop_record_index = cur + 2
        return cur, pre

    def _detect_loop_scan_context(self, cur):
        """The new keyframe's descriptor against the leading keyframes whose stamp is more than
        time_gap older than its own (the prefix stops at the first keyframe that is not); the
        smallest (dist, index) is accepted when dist < sc.threshold."""
        from .scan_context import eligible_prefix
        n_el = eligible_prefix([k[6] for k in self.key6d[:cur]], self.key6d[cur][6], self.time_gap)
        if n_el == 0:
            return None
        pre, dist, shift = self.sc_db.query(self.sc_db.descriptors()[cur], n_el)
        if pre < 0 or not dist < self.sc.threshold:
            return None
        self.sc_match = (pre, dist, shift)
        self.loop_record_index = cur + 2
        return cur, pre

    def _detect_loop_candidates(self):
        """sc_candidates > 1: detect_loop's gates, then the sc_candidates best places of the
        eligible prefix (ScanContextDB.query_topk) whose distance is below sc.threshold
        -> (cur, [(key_pre, dist, shift)] in rank order) or None."""
        from .scan_context import eligible_prefix
        cur = len(self.key6d) - 1
        if cur in self.loop_index:
            return None
        n_el = eligible_prefix([k[6] for k in self.key6d[:cur]], self.key6d[cur][6], self.time_gap)
        if n_el == 0:
            return None
        excl = self.search_num if self.sc_exclusion is None else self.sc_exclusion
        found = self.sc_db.query_topk(self.sc_db.descriptors()[cur], self.sc_candidates, excl, n_el)
        kept = [c for c in found if c[1] < self.sc.threshold]
        if not kept:
            return None
        self.loop_record_index = cur + 2
        return cur, kept

    def local_maps(self, items):
        """local_map for every (key, n) of items in two launches: every keyframe of every map
        through its own pose in one ssf_transform_clouds_batch, then the concatenated maps through
        one ssf_voxel_grid_batch (icp_leaf).  -> (maps [total, 4], h_off int64 [len(items) + 1]):
        map m is maps[h_off[m]:h_off[m + 1]]."""
        from .map_cloud import pose_rows
        dev = self.fe.device
        parts, poses, map_off = [], [], [0]
        for key, n in items:
            for k in range(key - n, key + n + 1):
                if 0 <= k < len(self.key6d):
                    parts.append(self.key_frames[k])
                    poses.append(self._T6(k))
            map_off.append(len(parts))
        sizes = np.array([int(p.shape[0]) for p in parts], np.int64)
        part_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        h_off = torch.from_numpy(part_off[map_off])
        if part_off[-1] == 0:
            return torch.zeros(0, 4, device=dev), torch.zeros(len(items) + 1, dtype=torch.int64)
        raw = torch.cat(parts)
        moved = torch.empty_like(raw)
        h_part = torch.from_numpy(part_off)
        d_part = h_part.to(dev)
        d_T = torch.from_numpy(pose_rows(poses)).to(dev)
        self.fe._check(_abi.lib().ssf_transform_clouds_batch(
            self.fe._h, _stream(dev), len(parts), _ptr(raw), _ptr(d_part), C.c_void_p(h_part.data_ptr()),
            _ptr(d_T), _ptr(moved)), "ssf_transform_clouds_batch")
        out, cnt = voxel_grid(self.fe, moved, h_off.to(dev), h_off, self.icp_leaf)
        cnt = cnt.cpu().numpy().astype(np.int64)
        maps = torch.cat([out[int(h_off[m]):int(h_off[m]) + int(cnt[m])] for m in range(len(items))])
        return maps, torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64))

    def local_map(self, key, n):
        """getLoopLocalMap (:200-218): keyframes key-n..key+n in the map frame, 0.1 m voxels."""
        parts = [transform_cloud(self.key_frames[k], self._T6(k))
                 for k in range(key - n, key + n + 1) if 0 <= k < len(self.key6d)]
        cloud = torch.cat(parts) if parts else torch.zeros(0, 4, device=self.fe.device)
        if cloud.shape[0] == 0:
            return cloud
        return voxel_grid_one(self.fe, cloud, self.icp_leaf)

    def add_loop_factor(self):
        """addLoopFactor (:221-272) up to the graph insertion."""
        n = len(self.key6d)
        if n < 5 or n - 1 <= self.loop_record_index:
            return None
        if self.sc_candidates > 1:
            return self._add_loop_factor_candidates()
        ids = self.detect_loop()
        if ids is None:
            return None
        cur, pre = ids
        cur_cloud = self.local_map(cur, 0)
        pre_cloud = self.local_map(pre, self.search_num)
        if cur_cloud.shape[0] < 300 or pre_cloud.shape[0] < 1000:
            return None
        if self.detector == "scan_context":
            # the keyframes may lie far apart in the drifted map frame: start ICP with the current
            # cloud placed at the candidate's pose under the yaw the match recovered
            yaw = self.sc_match[2] * (2.0 * math.pi / 60.0)
            guess = self._T6(pre) @ get_transformation(0.0, 0.0, 0.0, 0.0, 0.0, yaw) @ np.linalg.inv(self._T6(cur))
            r = icp(self.fe, cur_cloud, pre_cloud, guess=guess)
        else:
            r = icp(self.fe, cur_cloud, pre_cloud)
        if not r["converged"] or r["fitness"] > 0.2:
            return None
        return self._accept_loop(cur, pre, r)

    def _add_loop_factor_candidates(self):
        """add_loop_factor with sc_candidates > 1: every candidate verified in one batch
        (verify_candidates), and among the problems that pass the gates of the single-candidate
        path the smallest (fitness, rank)."""
        found = self._detect_loop_candidates()
        if found is None:
            return None
        cur, cands = found
        tried = self.verify_candidates(cur, cands)
        ok = [(r["fitness"], j, r) for j, r in tried if r["converged"] and r["fitness"] <= 0.2]
        if not ok:
            return None
        _, j, r = min(ok, key=lambda o: o[:2])
        self.sc_match = cands[j]
        c = self._accept_loop(cur, cands[j][0], r)
        c.candidates = [(*cands[k], q["fitness"], q["converged"]) for k, q in tried]
        return c

    def verify_candidates(self, cur, cands):
        """ICP of keyframe cur against every candidate (key_pre, dist, shift) of cands: the local
        maps of the candidates and the current cloud in one local_maps call, then one icp_batch
        with one problem per candidate -- the current cloud as every source, the candidate's map
        as its target, guess = T_pre . Rz(shift . 2 pi / 60) . T_cur^-1 as on the single-candidate
        path.  -> [(rank, icp result)] for the candidates whose map has at least 1000 points; []
        when the current cloud has fewer than 300."""
        maps, h_off = self.local_maps([(c[0], self.search_num) for c in cands] + [(cur, 0)])
        size = (h_off[1:] - h_off[:-1]).tolist()
        rank = [j for j in range(len(cands)) if size[j] >= 1000]
        if size[-1] < 300 or not rank:
            return []
        dev = self.fe.device
        cur_cloud = maps[int(h_off[-2]):int(h_off[-1])]
        src = cur_cloud.repeat(len(rank), 1)               # ICP moves its source: one copy per problem
        h_src = torch.arange(len(rank) + 1, dtype=torch.int64) * size[-1]
        tgt = torch.cat([maps[int(h_off[j]):int(h_off[j + 1])] for j in rank])
        h_tgt = torch.tensor(np.concatenate([[0], np.cumsum([size[j] for j in rank])]), dtype=torch.int64)
        inv_cur = np.linalg.inv(self._T6(cur))
        guess = [self._T6(cands[j][0]) @ get_transformation(0.0, 0.0, 0.0, 0.0, 0.0, cands[j][2] * (2.0 * math.pi / 60.0))
                 @ inv_cur for j in rank]
        res = icp_batch(self.fe, src, h_src.to(dev), h_src, tgt, h_tgt.to(dev), h_tgt, guess=guess)
        return list(zip(rank, res))

    def _accept_loop(self, cur, pre, r):
        """The rest of addLoopFactor for an ICP result r that passed its gates."""
        corr = r["T"].astype(np.float64)
        self.loop_record_index += 30
        t_correct = corr @ self._T6(cur)
        pose_from = get_transformation(*get_translation_and_euler_angles(t_correct))
        c = LoopConstraint(cur, pre, between(pose_from, self._T6(pre)), float(np.float32(r["fitness"])), corr)
        if self.detector == "scan_context":
            c.dist, c.shift = self.sc_match[1], self.sc_match[2]
        self.loop_index[cur] = pre
        self.constraints.append(c)
        return c

    # ---- pose graph (optimize=True)
    def _add_odom_factor(self, arr6d):
        """addOdomFactor (:147-165): currPose from the double arr6d, lastPose from the stored
        float key pose."""
        curr = get_transformation(*arr6d)
        n = len(self.key6d)
        if n == 1:
            self.graph_prior = pose7_from_matrix(curr)
        else:
            self.graph_edges.append((n - 2, n - 1, pose7_from_matrix(between(self._T6(n - 2), curr)),
                                     ODOM_VARIANCES))
        self.graph_init.append(pose7_from_matrix(curr))

    def pose_graph(self):
        """The recorded graph in the form optimize_pose_graphs takes."""
        return dict(poses=np.array(self.graph_init, np.float64).reshape(-1, 7),
                    edge_ij=np.array([(e[0], e[1]) for e in self.graph_edges], np.int32).reshape(-1, 2),
                    edge_meas=np.array([e[2] for e in self.graph_edges], np.float64).reshape(-1, 7),
                    edge_var=np.array([e[3] for e in self.graph_edges], np.float64).reshape(-1, 6),
                    prior_pose=np.asarray(self.graph_prior, np.float64), prior_var=np.array(PRIOR_VARIANCES))

    def apply_optimization(self, res):
        """correctPoses (:315-332) with a solution of pose_graph(): every key pose rewritten,
        rounded to float as PointXYZIRPYT stores it.  -> T_map_0_curr rebuilt from the last one."""
        if res["status"] not in (_abi.PGO_OK, _abi.PGO_CONVERGED):
            raise _abi.SSFError(f"pose-graph optimisation failed: {res['status_name']}")
        self.last_optimization = res
        for i, p in enumerate(res["poses"]):
            six = get_translation_and_euler_angles(pose_from_quat(p[:4], p[4:]))
            self.key6d[i][:6] = np.array(six, np.float32).tolist()
            self.graph_init[i] = np.array(p, np.float64)
        if self.map is not None:                            # the aLoopIsClosed branch (:318-326)
            self.rebuild_map()
        return self._T6(-1)

    def process(self, plane_xyzi: torch.Tensor, q_xyzw, t, stamp: float, scan: torch.Tensor | None = None):
        """One synchronised (/plane_frame_cloud2, /frame_odom2) pair (cloudThread :429-451 +
        mapOptimization :455-467).  Returns (T_map_0_curr, constraint or None, is_key).
        scan: the frame's raw points in the sensor frame, device [n, 3] or [n, 4] float32; needed by
        detector="scan_context" (ValueError without it) and not read otherwise.  The descriptor
        is never built from plane_xyzi: with a few hundred planar points most columns hold one
        occupied ring, two such columns have cosine 1, and every candidate comes out at distance 0."""
        if self.detector == "scan_context" and scan is None:
            raise ValueError("LoopCloser(detector=\"scan_context\"): process needs scan=, the frame's raw points")
        T = self.trans_loop_adjust @ pose_from_quat(q_xyzw, t)
        if not self.is_key_frame(T):
            return T, None, False
        x, y, z, r, p, yw = get_translation_and_euler_angles(T)
        self.key6d.append(np.array([x, y, z, r, p, yw], np.float32).tolist() + [float(stamp)])
        if self.map is not None:
            self._store_key_frame(plane_xyzi)
        else:
            self.key_frames.append(plane_xyzi.contiguous())
        if self.optimize:
            self._add_odom_factor((x, y, z, r, p, yw))
        if self.detector == "scan_context":
            from .scan_context import describe_one
            self.sc_db.append(describe_one(self.fe, scan, self.sc))
        c = self.add_loop_factor()
        rebuilt = False
        if c is not None:                                   # correctPoses (:321-326)
            if self.optimize:
                T = self.close_loop(c)                      # rebuilds the map, this keyframe included
                rebuilt = True
            self.trans_loop_adjust = self.trans_loop_adjust @ c.correction
        if self.map is not None and not rebuilt:            # updateKeyPose(numPoses - 1) (:329)
            k = len(self.key6d) - 1
            self.map.transform(k, k + 1, [self._T6(k)])
        return T, c, True

    def add_loop_edge(self, c: LoopConstraint):
        """The loop factor of :263-274: cur -> pre, poseFrom.between(poseTo), the fitness as all
        six variances."""
        self.graph_edges.append((c.key_cur, c.key_pre, pose7_from_matrix(c.between), (float(c.noise),) * 6))

    def close_loop(self, c: LoopConstraint):
        """runOptimize + correctPoses for one closed loop -> the corrected T_map_0_curr."""
        self.add_loop_edge(c)
        kw = {} if self.robust is None else dict(robust=self.robust, edge_out=True)
        if self.lm is not None:
            kw["lm"] = self.lm
        return self.apply_optimization(optimize_pose_graphs(self.fe, [self.pose_graph()], self.pgo, **kw)[0])

    def loop_weights(self):
        """[(key_cur, key_pre, weight)] of the loop edges in the last solve, in graph order (a
        solve with `robust`; [] before the first one)."""
        res = self.last_optimization
        if res is None or "edge_weight" not in res:
            return []
        return [(int(e[0]), int(e[1]), float(w)) for e, w in zip(self.graph_edges, res["edge_weight"])
                if abs(int(e[0]) - int(e[1])) != 1]


def optimize_loop_closers(fe: Frontend, closers, constraints, params=None, robust=None, lm=None):
    """Several sequences that closed a loop in the same step, solved in one launch: adds each
    constraint to its closer's graph, optimises all graphs together and applies correctPoses to
    each.  -> the corrected T_map_0_curr of every closer.  robust (pgo_robust): the loss on the
    loop edges of every graph of the launch; the closers then hold the edge weights.  lm (pgo_lm):
    step control for every graph of the launch."""
    for lc, c in zip(closers, constraints):
        lc.add_loop_edge(c)
    kw = {} if robust is None else dict(robust=robust, edge_out=True)
    if lm is not None:
        kw["lm"] = lm
    res = optimize_pose_graphs(fe, [lc.pose_graph() for lc in closers], params, **kw)
    return [lc.apply_optimization(r) for lc, r in zip(closers, res)]

"""Node shims around the device front-end that keep the reference's topics and message layouts
(SURVEY.md §8(f) row 1), plus an in-process runner that replays an npz dataset directory the
way `launch/*.launch` wires the nodes and writes the odometry as a TUM trajectory (row 2).

  PointCloudOdometryNode   scripts/PointCloudOdometry_noSeg.py:62-127
      per npz frame -> /velodyne_points (PointCloud2, xyz @ 0/4/8, step 12)
                    -> /frame_odom1    (Float64MultiArray data = [tx, ty, tz, qx, qy, qz, qw])
  FrameFeatureNode         src/frameFeature.cpp:35-139
      /velodyne_points -> /plane_frame_cloud1 (PointXYZI layout, stamp copied, frame "map")
                       -> /org_frame_cloud1   (the input, frame "map")
  LidarOdometryNode        src/lidarOdometry_onlyPC.cpp:85-124, 147-311  (run_onlyPC.launch)
      /plane_frame_cloud1 -> /frame_odom2 (Odometry, frame "map", child "map_child")
                          -> /frame_odom_path2 (Path of every pose so far)
                          -> /plane_frame_cloud2 (the current plane cloud, frame "map")
  LidarOdometryIngestNode  src/lidarOdometry.cpp:78-205  (run_noSeg / run_Seg launch graphs)
      /frame_odom1 -> odometryQueue;  /plane_frame_cloud1 -> pops the queue front from the
      second plane cloud on and accumulates it -> /frame_odom2, /frame_odom_path2,
      /plane_frame_cloud2 (no registration: the pose is the SSF Kabsch pose)

The data-source node of the two ActiveSceneFlow launches (pairs of scans through the sampler,
TFlow, the mask and the float32 Kabsch) is ssf.asf.ActiveSceneFlowNode; run_sequence builds it
for launch "noSeg_ActiveSceneFlow" / "Seg_ActiveSceneFlow".

rospy, sensor_msgs and nav_msgs are not in this image: messages are the plain stand-ins of
`ssf.io` / below, and a `Bus` delivers them in-process.  Subscribed callbacks are duck-typed
(any object with the sensor_msgs/PointCloud2 attributes works), so wiring a node to rospy is
`rospy.Subscriber(topic, PointCloud2, node.on_cloud)` plus a publish callable that converts
the stand-in to the real message class.
"""
from __future__ import annotations

import copy
from collections import defaultdict, deque
from dataclasses import dataclass, field

import numpy as np
import torch

from . import io as sio
from ._abi import SSFError
from .frontend import Frontend, PlaneBatch, frame_offsets, identity_poses


@dataclass
class Float64MultiArray:
    data: list = field(default_factory=list)


@dataclass
class Pose:
    position: tuple = (0.0, 0.0, 0.0)
    orientation: tuple = (0.0, 0.0, 0.0, 1.0)      # x, y, z, w


@dataclass
class Odometry:
    header: sio.Header = field(default_factory=sio.Header)
    child_frame_id: str = ""
    pose: Pose = field(default_factory=Pose)


@dataclass
class Path:
    header: sio.Header = field(default_factory=sio.Header)
    poses: list = field(default_factory=list)      # (Header, Pose) pairs (geometry_msgs/PoseStamped)


class Bus:
    """In-process topic bus: publish(topic, msg) calls every subscriber in subscription order
    and keeps the last `keep` messages per topic."""

    def __init__(self, keep: int = 0):
        self.subs = defaultdict(list)
        self.keep = keep
        self.log = defaultdict(list)

    def subscribe(self, topic, cb):
        self.subs[topic].append(cb)

    def publish(self, topic, msg):
        if self.keep:
            lg = self.log[topic]
            lg.append(msg)
            del lg[:-self.keep]
        for cb in self.subs[topic]:
            cb(msg)


def _single_batch(xyzi: torch.Tensor, device) -> PlaneBatch:
    m = int(xyzi.shape[0])
    off, h_off = frame_offsets([m], device)
    return PlaneBatch(xyzi, torch.tensor([m], dtype=torch.int32, device=device), off, h_off, max(m, 1))


class FrameFeatureNode:
    """src/frameFeature.cpp cloudHandler on the device: the single-read stage (k_feat_wave_reg /
    k_feat_wave_run / k_feat_chunk_flagged, then k_feat_select); frames above 262144 points take
    the binned stage (k_bin_count / k_bin_scan / k_bin_curv / k_select)."""

    def __init__(self, publish, n_rows: int = 64, device=None, frontend: Frontend | None = None):
        self.fe = frontend or Frontend(n_rows, device=device)
        self.publish = publish

    def on_cloud(self, msg):
        view, ox = sio.cloud_points(msg)
        pts = torch.from_numpy(np.array(view, dtype=np.float32)).to(self.fe.device)  # msg bytes are read-only
        planes = self.fe.extract_planes(pts, xyz_offset=ox)                 # :45-123
        stamp = sio.stamp_of(msg.header)
        self.publish("/plane_frame_cloud1", sio.xyzi_to_cloud(planes, stamp, "map"))   # :129-133
        org = copy.copy(msg)                                                  # :135-138
        org.header = sio.Header(stamp[0], stamp[1], "map")
        self.publish("/org_frame_cloud1", org)
        return planes


class LidarOdometryNode:
    """src/lidarOdometry_onlyPC.cpp: the first plane cloud only becomes the last frame; every
    later one is registered against it (association, plane table, Ceres-style LM or GN) and the
    accumulated pose is published.  para_q/para_t (the warm start) and q_0_curr/t_0_curr stay on
    the device between frames."""

    def __init__(self, publish, n_rows: int = 64, device=None, solver: str = "ceres_lm",
                 max_iter: int | None = None, frontend: Frontend | None = None):
        self.fe = frontend or Frontend(n_rows, device=device, solver=solver, max_iter=max_iter)
        self.publish = publish
        dev = self.fe.device
        self.pose_rel = identity_poses(1, dev)      # para_q, para_t (:49-50)
        self.pose_abs = identity_poses(1, dev)      # q_0_last / t_0_last (:87-90)
        self.last = None
        self.last_table = None
        self.path = Path(sio.Header(0, 0, "map"))
        self.num_frame = 0

    def on_plane_cloud(self, msg):
        self.num_frame += 1
        xyzi = torch.from_numpy(sio.cloud_xyzi(msg)).to(self.fe.device)
        curr = _single_batch(xyzi, self.fe.device)
        table = self.fe.plane_table(curr)            # this frame's 30-NN planes, used next frame
        stamp = sio.stamp_of(msg.header)
        result = None
        if self.last is not None:                    # flagStart (:301-306)
            self.fe.register(self.last, self.last_table, curr, self.pose_rel, self.pose_abs)
            result = self._publish_result(stamp, xyzi)
        self.last, self.last_table = curr, table     # *lastFramePlanePtr = *currFramePlanePtr (:307)
        return result

    def _publish_result(self, stamp, xyzi):
        p = self.pose_abs[0].cpu().numpy()
        hdr = sio.Header(stamp[0], stamp[1], "map")
        pose = Pose(tuple(float(v) for v in p[4:7]), tuple(float(v) for v in p[0:4]))
        odom = Odometry(hdr, "map_child", pose)
        self.publish("/frame_odom2", odom)                                    # :98-109
        self.path.poses.append((hdr, pose))                                   # :111-118
        self.path.header = sio.Header(stamp[0], stamp[1], "map")
        self.publish("/frame_odom_path2", self.path)
        self.publish("/plane_frame_cloud2", sio.xyzi_to_cloud(xyzi, stamp, "map"))   # :120-124
        return odom


class LidarOdometryIngestNode:
    """src/lidarOdometry.cpp, the odometry node of the SSF launch graphs (run_noSeg.launch:8,
    run_Seg.launch:8): no registration -- the relative pose comes from /frame_odom1.

    odomHandler (:169-173) queues every /frame_odom1 message; cloudThread (:176-205) takes plane
    clouds in order, the first one only sets flagStart, and every later one pops the FRONT of the
    odometry queue (frameRegistration, :145-159: data[0:3] -> para_t, data[3:7] -> para_q x,y,z,w)
    and accumulates it (publishResult :80-83) on the device.  With the publisher's order (cloud
    first, then its pose) plane cloud k therefore consumes the pose published with frame k - 1.
    The reference reads front() of an EMPTY queue when a plane cloud overtakes the poses (UB,
    :148); here that raises SSFError."""

    def __init__(self, publish, device=None, frontend: Frontend | None = None):
        self.fe = frontend or Frontend(64, device=device)
        self.publish = publish
        self.queue = deque()                        # odometryQueue
        self.flag_start = False
        self.q_0_last = [0.0, 0.0, 0.0, 1.0]        # q_0_last / t_0_last (:68-71)
        self.t_0_last = [0.0, 0.0, 0.0]
        self.path = Path(sio.Header(0, 0, "map"))
        self.num_frame = 0

    def on_odom(self, msg):
        data = [float(v) for v in msg.data]
        if len(data) < 7:
            raise SSFError(f"/frame_odom1 carries {len(data)} values, expected [t(3), q(4)]")
        self.queue.append(data)

    def on_plane_cloud(self, msg):
        self.num_frame += 1
        stamp = sio.stamp_of(msg.header)
        if not self.flag_start:                     # :196-197
            self.flag_start = True
            return None
        if not self.queue:
            raise SSFError("plane cloud before its /frame_odom1 pose: the reference reads "
                           "odometryQueue.front() of an empty queue here (lidarOdometry.cpp:148)")
        d = self.queue.popleft()                    # frameRegistration (:147-155)
        rel = torch.tensor([[d[3], d[4], d[5], d[6], d[0], d[1], d[2]]], dtype=torch.float64,
                           device=self.fe.device)
        start = self.q_0_last + self.t_0_last
        ab = self.fe.accumulate_sequence(rel, start=start)[0].cpu().numpy()   # :80-83
        self.q_0_last = [float(v) for v in ab[0:4]]
        self.t_0_last = [float(v) for v in ab[4:7]]
        hdr = sio.Header(stamp[0], stamp[1], "map")
        pose = Pose(tuple(self.t_0_last), tuple(self.q_0_last))
        odom = Odometry(hdr, "map_child", pose)
        self.publish("/frame_odom2", odom)                                    # :96-107
        self.path.poses.append((hdr, pose))                                   # :109-116
        self.path.header = sio.Header(stamp[0], stamp[1], "map")
        self.publish("/frame_odom_path2", self.path)
        xyzi = sio.cloud_xyzi(msg)                                            # :118-122
        self.publish("/plane_frame_cloud2", sio.xyzi_to_cloud(xyzi, stamp, "map"))
        return odom


class PointCloudOdometryNode:
    """The data-source node of the launch graphs, for one npz frame: publish the cloud, then
      mode 'gmm'  -- PointCloudOdometry_noSeg.py:62-127: GMM mask + Kabsch pose as [t, q];
      mode 'gt'   -- PointCloudOdometry.py:60-105: background = s_fg_mask == 0, Kabsch, [t, q];
      mode 'none' -- PointCloudOdometry_onlyPC.py:37-65: the cloud only (no /frame_odom1)."""

    def __init__(self, publish, device=None, frontend: Frontend | None = None, mode: str = "gmm",
                 seed: int | None = None):
        if mode not in ("gmm", "gt", "none"):
            raise ValueError(f"mode {mode!r}")
        self.fe = frontend or Frontend(64, device=device)
        self.publish = publish
        self.mode = mode
        if seed is not None:
            self.fe.seed(seed)

    def on_frame(self, pos1, flow=None, stamp=(0, 0), gt_mask=None):
        dev = self.fe.device
        pos = pos1 if isinstance(pos1, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pos1, np.float32))
        pos = pos.to(dev, torch.float32).contiguous()
        self.publish("/velodyne_points", sio.xyz_to_cloud(pos.cpu().numpy(), stamp, "livox_frame"))   # :73-94
        if self.mode == "none":
            return None
        fl = flow if isinstance(flow, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(flow, np.float32))
        fl = fl.to(dev, torch.float32).contiguous()
        off, h_off = frame_offsets([pos.shape[0]], dev)
        m = None
        if self.mode != "gmm":
            m = torch.as_tensor(np.asarray(gt_mask) if not isinstance(gt_mask, torch.Tensor) else gt_mask)
            m = m.to(dev, torch.uint8).contiguous()
        out, _ = self.fe.mask_pose(pos, fl, off, h_off, mode=self.mode, mask_in=m, want_mask=False)
        o = out[0].cpu().numpy()
        msg = Float64MultiArray([float(v) for v in o[0:7]])                   # hstack((t, q)) :123-125
        self.publish("/frame_odom1", msg)
        return o


class MapOptimizationNode:
    """src/mapOptmization.cpp cloudThread/mapOptimization (:429-467) for one sequence: pairs
    /plane_frame_cloud2 with /frame_odom2 (stamps within 5 ms, :434-439), keeps keyframes,
    detects loops and registers them on the GPU (ssf.loop.LoopCloser), publishes
    /map_odom_res3 (Odometry "map" / "map_child"), /map_frame_res3 (the frame in the map) and
    /map_laser_path_res3, and appends TUM lines to RESULT_PATH (:355-374).  GTSAM iSAM2 is not
    part of this path: the published pose is the loop-adjusted odometry trans_loop_adjust *
    T_fodom_0_curr (:450) at every frame (the reference publishes its iSAM2 estimate for
    keyframes only), and the loop constraints are kept in ``closer.constraints``.
    optimize=True: a loop closure also optimises the pose graph on the GPU and rewrites every
    keyframe pose (runOptimize / correctPoses, :280-332; ``closer.key6d``,
    ``closer.last_optimization``); the keyframe that closed the loop is published at its
    corrected pose.  map_robust (ssf.loop.pgo_robust, with optimize): a robust loss on the loop
    edges of those solves; ``closer.loop_weights()`` then gives every loop's weight.  map_lm
    (ssf.loop.pgo_lm, with optimize): Levenberg-Marquardt step control for those solves; map_iters
    (with optimize): their max_iter (default 8), the attempts under step control.
    map_cloud=True: the accumulated map (mapCloudPtr) is kept on the device (``closer.map``)
    and its 0.4 m VoxelGrid is published on /sum_map_cloud_res3 for every keyframe whose pair
    count numFrame (first pair = 1) is a multiple of 5 (publishResult :387-397).
    map_detector="scan_context" (default "radius", the reference's search over key positions):
    loops are found by Scan Context descriptors of the raw scans (ssf.scan_context, DESIGN.md
    §6.12); the node then also takes /velodyne_points (on_scan), pairs each scan with its plane
    cloud by stamp and hands it to the closer; map_sc_threshold: the acceptance distance
    (default: ssf_sc_params'); map_sc_candidates = K > 1: the K best places are verified by ICP in
    one batch and the best fitness closes the loop (LoopCloser(sc_candidates=)), map_sc_exclusion:
    no two of them within that many keyframes of each other (default: the closer's search_num)."""

    def __init__(self, publish, device=None, frontend: Frontend | None = None,
                 tum_path: str | None = None, optimize: bool = False, map_cloud: bool = False,
                 map_robust=None, map_lm=None, map_iters: int | None = None,
                 map_detector: str = "radius", map_sc_threshold: float | None = None,
                 map_sc_candidates: int = 1, map_sc_exclusion: int | None = None):
        from .loop import LoopCloser, get_translation_and_euler_angles, pgo_params  # noqa: F401
        self.publish = publish
        self.fe = frontend or Frontend(64, device=device)
        if map_robust is not None and not optimize:
            raise ValueError("map_robust is a loss of the pose-graph solve: it needs optimize=True")
        if map_lm is not None and not optimize:
            raise ValueError("map_lm is the step control of the pose-graph solve: it needs optimize=True")
        if map_iters is not None and not optimize:
            raise ValueError("map_iters is the iteration limit of the pose-graph solve: it needs optimize=True")
        if map_iters is not None and int(map_iters) <= 0:
            raise ValueError("map_iters must be positive")
        kw = dict(optimize=True) if optimize else {}
        if map_lm is not None:
            kw["lm"] = map_lm
        if map_iters is not None:
            kw["pgo"] = pgo_params(max_iter=int(map_iters))
        if map_cloud:
            kw["map_cloud"] = True
        if map_robust is not None:
            kw["robust"] = map_robust
        if map_detector not in ("radius", "scan_context"):
            raise ValueError(f"map_detector is radius or scan_context, not {map_detector!r}")
        if map_sc_threshold is not None and map_detector != "scan_context":
            raise ValueError("map_sc_threshold is the acceptance distance of map_detector=\"scan_context\"")
        if (map_sc_candidates != 1 or map_sc_exclusion is not None) and map_detector != "scan_context":
            raise ValueError("map_sc_candidates and map_sc_exclusion belong to map_detector=\"scan_context\"")
        if map_detector == "scan_context":
            from .scan_context import sc_params
            kw.update(detector="scan_context", sc=sc_params(threshold=map_sc_threshold))
            if map_sc_candidates != 1 or map_sc_exclusion is not None:
                kw.update(sc_candidates=map_sc_candidates, sc_exclusion=map_sc_exclusion)
        self.closer = LoopCloser(self.fe, **kw)
        self.scans = []                           # recent /velodyne_points (map_detector="scan_context")
        self.map_cloud = bool(map_cloud)
        self.num_frame = 0                        # numFrame (:433): synchronised pairs
        self.map_published = 0
        self.planes, self.odoms = [], []          # planeQueue / odometryQueue (:65-75)
        self.path = Path()
        self.writer = sio.TumWriter(tum_path) if tum_path else None

    def on_plane_cloud(self, msg):
        self.planes.append(msg)
        self._drain()

    def on_odom(self, msg):
        self.odoms.append(msg)
        self._drain()

    def on_scan(self, msg):
        """/velodyne_points: the raw scan the Scan Context descriptor is built from; not kept
        under the radius detector."""
        if self.closer.detector != "scan_context":
            return
        self.scans.append(msg)
        del self.scans[:-16]
        self._drain()

    def _scan_for(self, tp):
        """The kept scan stamped within 5 ms of tp -> (found, msg).  Without one: not found while
        no later scan has come either (it may still arrive); else the nearest in stamp (its own
        was lost)."""
        if not self.scans:
            return False, None
        dt = [(s[0] - tp[0]) + (s[1] - tp[1]) * 1e-9 for s in (sio.stamp_of(m.header) for m in self.scans)]
        k = min(range(len(dt)), key=lambda i: abs(dt[i]))
        if abs(dt[k]) > 0.005 and max(dt) < 0.0:
            return False, None
        return True, self.scans[k]

    def _drain(self):
        import numpy as np
        from .loop import transform_cloud
        from scipy.spatial.transform import Rotation
        while self.planes and self.odoms:
            pm, om = self.planes[0], self.odoms[0]
            tp, to = sio.stamp_of(pm.header), sio.stamp_of(om.header)
            if abs((tp[0] - to[0]) + (tp[1] - to[1]) * 1e-9) > 0.005:    # time sync (:436-439)
                return
            kw = {}
            if self.closer.detector == "scan_context":
                found, sm = self._scan_for(tp)
                if not found:                      # the pair's scan has not come yet: on_scan drains again
                    return
                kw["scan"] = torch.from_numpy(np.array(sio.cloud_xyz(sm))).to(self.fe.device)  # msg bytes are read-only
            self.planes.pop(0)
            self.odoms.pop(0)
            xyzi = torch.from_numpy(sio.cloud_xyzi(pm)).to(self.fe.device)
            stamp = tp[0] + tp[1] * 1e-9
            self.num_frame += 1
            T, _, is_key = self.closer.process(xyzi, om.pose.orientation, om.pose.position, stamp, **kw)
            q = Rotation.from_matrix(T[:3, :3]).as_quat()                  # x, y, z, w
            hdr = sio.Header(tp[0], tp[1], "map")
            pose = Pose(tuple(float(v) for v in T[:3, 3]), tuple(float(v) for v in q))
            self.publish("/map_odom_res3", Odometry(hdr, "map_child", pose))
            if self.writer:
                self.writer.write(tp, pose.position, pose.orientation)
            self.path.poses.append((hdr, pose))
            self.path.header = hdr
            self.publish("/map_laser_path_res3", self.path)
            self.publish("/map_frame_res3", sio.xyzi_to_cloud(transform_cloud(xyzi, T), tp, "map"))
            if self.map_cloud and is_key and self.num_frame % 5 == 0:      # :388-397
                self.publish("/sum_map_cloud_res3", sio.xyzi_to_cloud(self.closer.map.filtered(0.4), tp, "map"))
                self.map_published += 1


LAUNCH_GRAPHS = {
    # launch file: (data-source mode, odometry node, npz keys)
    "onlyPC": ("none", "registration", ("pos1",)),             # run_onlyPC.launch:7-15
    "noSeg": ("gmm", "ingest", ("pos1", "gt")),                 # run_noSeg.launch:7-16
    "Seg": ("gt", "ingest", ("pos1", "gt", "s_fg_mask")),       # run_Seg.launch:7-16
    # the ActiveSceneFlow launches (data source: ssf.asf.ActiveSceneFlowNode on pairs of scans); a
    # fourth entry: the npz keys that are read when the files carry them
    "noSeg_ActiveSceneFlow": ("gmm", "ingest", ("pos1", "pos2"),            # run_noSeg_ActiveSceneFlow.launch
                              ("gt", "s_fg_mask", "t_fg_mask")),
    "Seg_ActiveSceneFlow": ("gt", "ingest", ("pos1", "pos2", "s_fg_mask"),  # run_Seg_ActiveSceneFlow.launch
                            ("gt", "t_fg_mask")),
}
ASF_LAUNCHES = ("noSeg_ActiveSceneFlow", "Seg_ActiveSceneFlow")


def _npz_keys(root, keys, optional):
    """keys plus the optional ones the first file of the sequence carries"""
    files = sio.sequence_files(root)
    if not files:
        return tuple(keys)
    with np.load(files[0], allow_pickle=False) as z:
        return tuple(keys) + tuple(k for k in optional if k in z.files)


def _asf_net(weights, n_points, device):
    """the TFlow of an ASF launch: a ready module, or a checkpoint path loaded into a new one"""
    from .asf import load_checkpoint
    from .tflow import TFlow
    if weights is None:
        raise ValueError("an ActiveSceneFlow launch needs the network's weights: pass weights= (a "
                         "checkpoint path or a TFlow); no trained weights ship with the project")
    if isinstance(weights, torch.nn.Module):
        return weights
    return load_checkpoint(TFlow(npoint=n_points), weights).to(device)


def run_sequence(root: str, tum_path: str | None = None, n_rows: int = 64, device=None,
                 solver: str = "ceres_lm", max_iter: int | None = None, seed: int | None = None,
                 rate_hz: float = 10.0, launch: str = "onlyPC", map_tum_path: str | None = None,
                 truncate_results: bool = False, map_optimize: bool = False, map_cloud: bool = False,
                 weights=None, n_points: int = 8192, map_robust=None, map_lm=None,
                 map_iters: int | None = None, map_detector: str = "radius",
                 map_sc_threshold: float | None = None, map_sc_candidates: int = 1,
                 map_sc_exclusion: int | None = None):
    """Replay a DATASET_PATH directory through the node graph of launch/run_<launch>.launch:
      onlyPC: PointCloudOdometry_onlyPC -> frameFeature -> lidarOdometry_onlyPC (registration)
      noSeg:  PointCloudOdometry_noSeg (GMM mask + Kabsch -> /frame_odom1) -> frameFeature ->
              lidarOdometry (pose ingest + accumulation)
      Seg:    PointCloudOdometry (ground-truth mask s_fg_mask == 0) -> same as noSeg
      noSeg_ActiveSceneFlow / Seg_ActiveSceneFlow: ssf.asf.ActiveSceneFlowNode (subsample to
              n_points, TFlow with `weights` -- a checkpoint path or a ready TFlow --, GMM /
              ground-truth mask on the network's flow, float32 Kabsch -> /frame_odom1) -> same
              as noSeg; npz keys pos1, pos2 (+ gt, s_fg_mask, t_fg_mask when present); the sampler
              and the GMM take `seed` (default 1234)
    plus mapOptmization when `map_tum_path` is given (map_optimize: with the GPU pose-graph
    optimisation of its loop closures; map_robust: an ssf.loop.pgo_robust loss on their loop
    edges, map_lm: an ssf.loop.pgo_lm step control for those solves, map_iters: their max_iter;
    all three need map_optimize; map_detector="scan_context": its loops are found by Scan Context
    descriptors of the /velodyne_points scans instead of the radius search, map_sc_threshold the
    acceptance distance, map_sc_candidates / map_sc_exclusion the places it verifies by ICP per
    keyframe and how many keyframes apart they lie at least).  Stamps are synthetic and monotone (frame k
    at k / rate_hz; the reference uses wall-clock ros::Time::now()).  The /frame_odom2 poses are
    appended to `tum_path` as TUM lines (like the reference, an existing file is extended unless
    truncate_results=True).
    -> dict(odom1 [F, 7] f64 [t, q] (empty for onlyPC), odom2 [F-1, 7] f64 [t, q], stamps, loops;
    an ASF launch on files with gt also flow_metrics, one dict per pair;
    with map_optimize also optimization (the last solve) and key_poses; with map_cloud (needs
    map_tum_path) also map_cloud, the final 0.4 m map as float32 [M, 4], map_cloud_published,
    the number of /sum_map_cloud_res3 messages, and map_cloud_keyframes)"""
    if launch not in LAUNCH_GRAPHS:
        raise ValueError(f"launch {launch!r}: one of {sorted(LAUNCH_GRAPHS)}")
    if map_cloud and map_tum_path is None:
        raise ValueError("map_cloud needs mapOptmization in the graph: pass map_tum_path")
    if map_robust is not None and not map_optimize:
        raise ValueError("map_robust is a loss of the pose-graph solve: it needs map_optimize")
    if map_lm is not None and not map_optimize:
        raise ValueError("map_lm is the step control of the pose-graph solve: it needs map_optimize")
    if map_iters is not None and not map_optimize:
        raise ValueError("map_iters is the iteration limit of the pose-graph solve: it needs map_optimize")
    if map_iters is not None and int(map_iters) <= 0:
        raise ValueError("map_iters must be positive")
    if map_detector not in ("radius", "scan_context"):
        raise ValueError(f"map_detector is radius or scan_context, not {map_detector!r}")
    if map_detector != "radius" and map_tum_path is None:
        raise ValueError("map_detector chooses mapOptmization's loop detector: pass map_tum_path")
    if map_sc_threshold is not None and map_detector != "scan_context":
        raise ValueError("map_sc_threshold is the acceptance distance of map_detector=\"scan_context\"")
    if (map_sc_candidates != 1 or map_sc_exclusion is not None) and map_detector != "scan_context":
        raise ValueError("map_sc_candidates and map_sc_exclusion belong to map_detector=\"scan_context\"")
    src_mode, odo_kind, keys = LAUNCH_GRAPHS[launch][:3]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    bus = Bus()
    asf = launch in ASF_LAUNCHES
    if asf:
        from .asf import ActiveSceneFlowNode
        net = _asf_net(weights, n_points, dev)
        keys = _npz_keys(root, keys, LAUNCH_GRAPHS[launch][3])
        pco = ActiveSceneFlowNode(bus.publish, net, mode=src_mode, n_points=n_points, device=dev,
                                  **({} if seed is None else dict(seed=seed)))
    else:
        pco = PointCloudOdometryNode(bus.publish, device=dev, seed=seed, mode=src_mode)
    ff = FrameFeatureNode(bus.publish, n_rows=n_rows, device=dev)
    if odo_kind == "registration":
        lo = LidarOdometryNode(bus.publish, n_rows=n_rows, device=dev, solver=solver, max_iter=max_iter)
    else:
        lo = LidarOdometryIngestNode(bus.publish, device=dev)
        bus.subscribe("/frame_odom1", lo.on_odom)
    bus.subscribe("/velodyne_points", ff.on_cloud)
    bus.subscribe("/plane_frame_cloud1", lo.on_plane_cloud)
    odom1, odom2, stamps = [], [], []
    if tum_path and truncate_results:
        open(tum_path, "w").close()
    writer = sio.TumWriter(tum_path) if tum_path else None

    def on_odom1(msg):
        odom1.append(list(msg.data))

    def on_odom2(msg):
        odom2.append(list(msg.pose.position) + list(msg.pose.orientation))
        if writer:
            writer.write((msg.header.stamp_sec, msg.header.stamp_nsec), msg.pose.position,
                         msg.pose.orientation)

    bus.subscribe("/frame_odom1", on_odom1)
    bus.subscribe("/frame_odom2", on_odom2)
    mo = None
    if map_tum_path is not None:                     # mapOptmization on /plane_frame_cloud2 + /frame_odom2
        if map_tum_path and truncate_results:
            open(map_tum_path, "w").close()
        mkw = dict(optimize=True) if map_optimize else {}
        if map_cloud:
            mkw["map_cloud"] = True
        if map_robust is not None:
            mkw["map_robust"] = map_robust
        if map_lm is not None:
            mkw["map_lm"] = map_lm
        if map_iters is not None:
            mkw["map_iters"] = map_iters
        if map_detector != "radius":
            mkw.update(map_detector=map_detector, map_sc_threshold=map_sc_threshold)
        if map_sc_candidates != 1 or map_sc_exclusion is not None:
            mkw.update(map_sc_candidates=map_sc_candidates, map_sc_exclusion=map_sc_exclusion)
        mo = MapOptimizationNode(bus.publish, device=dev, tum_path=map_tum_path or None, **mkw)
        bus.subscribe("/plane_frame_cloud2", mo.on_plane_cloud)
        bus.subscribe("/frame_odom2", mo.on_odom)
        if map_detector == "scan_context":           # after frameFeature: the pair waits for its scan
            bus.subscribe("/velodyne_points", mo.on_scan)
    period_ns = int(round(1e9 / rate_hz))
    metrics = []
    for fr in sio.NpzSequence(root, keys=keys, device=dev):
        t_ns = fr["index"] * period_ns
        stamp = (t_ns // 1_000_000_000, t_ns % 1_000_000_000)
        stamps.append(stamp)
        if asf:
            _, fm = pco.on_pair(fr["pos1"], fr["pos2"], stamp, fg1=fr.get("s_fg_mask"),
                                fg2=fr.get("t_fg_mask"), gt_flow=fr.get("gt"))
            if fm is not None:
                metrics.append(fm)
            continue
        pco.on_frame(fr["pos1"], fr.get("gt"), stamp,
                     gt_mask=fr.get("s_fg_mask") if src_mode == "gt" else None)
    res = dict(odom1=np.asarray(odom1, np.float64).reshape(-1, 7),
               odom2=np.asarray(odom2, np.float64).reshape(-1, 7), stamps=stamps,
               loops=mo.closer.constraints if mo else [])
    if metrics:
        res["flow_metrics"] = metrics
    if map_optimize:                                 # the last solve (None: no loop was closed)
        res["optimization"] = mo.closer.last_optimization if mo else None
        res["key_poses"] = [list(k) for k in mo.closer.key6d] if mo else []
    if map_cloud:                                    # the map as it stands, filtered once
        res["map_cloud"] = mo.closer.map.filtered(0.4).cpu().numpy()
        res["map_cloud_published"] = mo.map_published
        res["map_cloud_keyframes"] = mo.closer.map.n_keyframes
    return res

"""ssf -- MI355X (gfx950) SSF-SLAM LiDAR front-end.

Host-side mirror of the reference's hot-path interfaces over the C ABI in
include/ssf_frontend.h (libssf_frontend.so, hand-written HIP kernels).  There is no CPU
fallback anywhere in this package.
"""
from ._abi import SSFError  # noqa: F401
from .frontend import Frontend, PlaneBatch, frame_offsets, identity_poses, register_plan  # noqa: F401
from .pose import mask_and_pose, slove_RT_by_SVD  # noqa: F401
from . import loop  # noqa: F401  (mapOptmization loop closure: voxel grid, ICP, LoopCloser)
from .map_cloud import MapCloud  # noqa: F401  (mapOptmization's accumulated map cloud)
from . import pointnet2  # noqa: F401  (TFlow point-set operators: pointutils surface)
from . import tflow  # noqa: F401  (the TFlow network: cost volume, warping, flow regressor)
from .tflow import CostVolume, PointWarping, RefineFlowRegressor, TFlow  # noqa: F401
from . import asf  # noqa: F401  (the ActiveSceneFlow chain: subsample, TFlow, mask, pose)
from . import scan_context  # noqa: F401  (loop detection by appearance: Scan Context descriptors)
from .scan_context import ScanContextDB  # noqa: F401

__all__ = ["Frontend", "PlaneBatch", "frame_offsets", "identity_poses", "register_plan", "SSFError",
           "mask_and_pose", "slove_RT_by_SVD", "loop", "MapCloud", "pointnet2"]
__all__ += ["tflow", "CostVolume", "PointWarping", "RefineFlowRegressor", "TFlow", "asf"]
__all__ += ["scan_context", "ScanContextDB"]

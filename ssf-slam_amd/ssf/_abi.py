"""ctypes binding of libssf_frontend.so (include/ssf_frontend.h).

The library is loaded AFTER torch so that its libamdhip64.so.7 dependency resolves to the HIP
runtime torch already mapped (one runtime per process).  There is no fallback: if the library
is missing or fails to load, every entry point raises -- the product path never silently runs
on a CPU substitute.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the dlopen below, see module docstring)

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib")
LIB_PATH = os.environ.get("SSF_LIB", os.path.join(LIB_DIR, "libssf_frontend.so"))

SSF_OK, SSF_E_ARG, SSF_E_HIP, SSF_E_NOMEM, SSF_E_CAPACITY, SSF_E_NODEV = 0, -1, -2, -3, -4, -5
SOLVER_CERES_LM, SOLVER_GN = 0, 1
MASK_GMM, MASK_GT, MASK_GIVEN = 0, 1, 2
# the evaluation of frameFeature.cpp:57 (ssf_config.ring_chain, include/ssf_frontend.h)
RING_CHAIN_FLOAT, RING_CHAIN_DOUBLE = 0, 1
RING_CHAINS = {"float": RING_CHAIN_FLOAT, "double": RING_CHAIN_DOUBLE}
# frames of plane points the association can stage from the plane table's strip image
# (reg_strips.hpp: kStripHeadWords, kAssocStripF4Max)
STRIP_IMAGE_MIN, STRIP_IMAGE_MAX = (256 + 1) + 2 * 256 + 4, 6144
POSE_OUT_STRIDE = 32
POSE_OUT = dict(T=0, Q=3, R=7, STATUS=16, NBG=17, BGLABEL=18, KM_ITER=19, EM_ITER=20,
                CONVERGED=21, CENTER0=22, CENTER1=23, LOWER_BOUND=24, PASSES=25)
POSE_EMPTY, POSE_REFLECTION, POSE_NOT_ORTHOGONAL, POSE_GMM_FAILED, POSE_SYNC_FAILED = -1, -2, -3, -4, -5

# Every symbol include/ssf_frontend.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "ssf_abi_version", "ssf_config_default", "ssf_create", "ssf_destroy", "ssf_last_error",
    "ssf_reserve", "ssf_extract_planes_batch", "ssf_extract_planes", "ssf_plane_table_batch",
    "ssf_register_batch", "ssf_register_chain", "ssf_mask_pose_batch", "ssf_rng_seed", "ssf_accumulate_sequence",
    "ssf_voxel_grid_batch", "ssf_icp_params_default", "ssf_icp_batch",
    "ssf_extract_planes_batch_masked", "ssf_register_pair", "ssf_profile_enable",
    "ssf_profile_read", "ssf_set_mask_split", "ssf_mask_pose_batch_f64",
    "ssf_edge_config_default", "ssf_set_edge_config", "ssf_extract_features_batch",
    "ssf_edge_table_batch", "ssf_register_batch_edges", "ssf_kabsch_f32_batch",
    "ssf_set_mask_schedule", "ssf_register_plan", "ssf_pgo_params_default", "ssf_pose_graph_batch",
    "ssf_transform_clouds_batch", "ssf_subsample_batch",
    "ssf_pgo_robust_default", "ssf_pose_graph_batch_robust",
    "ssf_pgo_lm_default", "ssf_pose_graph_batch_lm",
    "ssf_sc_params_default", "ssf_scan_context_batch", "ssf_scan_context_match",
    "ssf_scan_context_match_topk",
]
# ssf_scan_context_*: descriptor shape; ssf_sc_best as four 32-bit words per query (and per slot
# of ssf_scan_context_match_topk, at most SC_MAX_TOPK of them)
SC_RINGS, SC_SECTORS = 20, 60
SC_MAX_TOPK = 8
SC_BEST_STRIDE = 4
SC_BEST = dict(INDEX=0, DIST=1, SHIFT=2)
# ssf_subsample_batch: limits and per-frame status codes
SAMPLE_MAX_NB, SAMPLE_MAX_POINTS = 8192, 1 << 24
SAMPLE_OK, SAMPLE_EMPTY, SAMPLE_SHORT = 0, -1, -2
# Every symbol include/ssf_pointnet2.h declares (TFlow point-set operators).
PN2_EXPORTS = [
    "ssf_pn2_last_error", "ssf_pn2_furthest_point_sample", "ssf_pn2_knn", "ssf_pn2_three_nn",
    "ssf_pn2_gather", "ssf_pn2_three_interpolate", "ssf_pn2_upsample_flow",
    "ssf_pn2_group_relative", "ssf_pn2_grouped_mlp_max", "ssf_pn2_grouped_mlp",
    "ssf_pn2_pair_attention", "ssf_pn2_segment_softmax_sum",
]
PN2_KNN_MAX, PN2_UPSAMPLE_MAX_SPARSE = 32, 4096
PN2_MLP_MAX_LAYERS, PN2_MLP_MAX_WIDTH = 3, 512
PN2_GMLP_MAX_IN, PN2_ATTN_MAX_C = 766, 512

ICP_OUT_STRIDE = 24
ICP_OUT = dict(T=0, FITNESS=16, CONVERGED=17, ITERATIONS=18, STATE=19, NCORR=20)
ICP_STATES = {0: "not_converged", 1: "iterations", 2: "transform", 3: "abs_mse", 4: "rel_mse",
              5: "no_correspondences"}


PGO_MAX_LOOPS, PGO_MAX_ITER, PGO_OUT_STRIDE = 256, 1024, 8
PGO_OUT = dict(STATUS=0, ITERATIONS=1, COST0=2, COST=3, DX=4, LOOPS=5, ACCEPTED=6, RADIUS=7)
PGO_OK, PGO_CONVERGED, PGO_EMPTY, PGO_BAD_INPUT, PGO_TOO_MANY_LOOPS, PGO_NOT_PD = range(6)
PGO_STATUS = {0: "ok", 1: "converged", 2: "empty", 3: "bad_input", 4: "too_many_loops", 5: "not_pd"}


# ssf_pgo_robust: the loss on the loop edges (ssf_pose_graph_batch_robust) and its per-edge output
PGO_ROBUST_NONE, PGO_ROBUST_HUBER, PGO_ROBUST_CAUCHY, PGO_ROBUST_GEMAN_MCCLURE = range(4)
PGO_ROBUST_KINDS = dict(none=0, huber=1, cauchy=2, geman_mcclure=3)
PGO_EDGE_OUT_STRIDE = 2
PGO_EDGE_OUT = dict(WEIGHT=0, CHI2=1)
# ssf_pgo_lm: step control (ssf_pose_graph_batch_lm) and its per-attempt log
PGO_LM_LOG_STRIDE = 4
PGO_LM_LOG = dict(COST=0, MCC=1, RADIUS=2, OUTCOME=3)
PGO_LM_REJECTED, PGO_LM_ACCEPTED, PGO_LM_INVALID = range(3)


class PgoParams(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("func_tol", C.c_double)]


class PgoRobust(C.Structure):
    _fields_ = [("kind", C.c_int32), ("k", C.c_double)]


class PgoLm(C.Structure):
    _fields_ = [("radius0", C.c_double), ("min_relative_decrease", C.c_double), ("max_radius", C.c_double),
                ("min_radius", C.c_double)]


class ScParams(C.Structure):
    _fields_ = [("max_range", C.c_float), ("lidar_height", C.c_float), ("threshold", C.c_float)]


class IcpParams(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("max_corr_dist", C.c_float), ("trans_eps", C.c_double),
                ("fit_eps", C.c_double)]


STEP_STATUS = {0: "rejected", 1: "accepted", 2: "invalid", 3: "param_tol", 4: "func_tol",
               5: "grad_tol", 6: "gn"}


class Step(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("cost", C.c_double),
                ("status", C.c_int32), ("pad", C.c_int32), ("radius", C.c_double)]


class StepLog(C.Structure):
    _fields_ = [("cap", C.c_int32), ("n_steps", C.c_int32), ("n_corr", C.c_int32),
                ("pad", C.c_int32), ("steps", C.POINTER(Step))]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int32), ("total_ms", C.c_double)]


class Config(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("plane_min", C.c_float), ("plane_span", C.c_int32),
                ("row_start", C.c_int32), ("row_end", C.c_int32), ("plane_max", C.c_float),
                ("solver", C.c_int32), ("max_iter", C.c_int32), ("ring_chain", C.c_int32)]


class EdgeConfig(C.Structure):
    """ssf_edge_config (beyond the reference: edge features + point-to-line residuals)."""
    _fields_ = [("edge_min", C.c_float), ("edge_span", C.c_int32), ("line_ratio", C.c_float),
                ("max_nn_d2", C.c_float)]


class LaunchPlan(C.Structure):
    """ssf_launch_plan: the association launch of a register call (ssf_register_plan)."""
    _fields_ = [("strip_path", C.c_int32), ("group_mode", C.c_int32), ("soa", C.c_int32),
                ("qsplit", C.c_int32), ("lds_cap", C.c_int32), ("compacted", C.c_int32)]


_lib = None


class SSFError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SSFError(f"{LIB_PATH} is missing: build it first (python -c 'import __graft_entry__ "
                       f"as g; g.build()')")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.ssf_abi_version.restype = i32
    L.ssf_config_default.argtypes = [i32, C.POINTER(Config)]
    L.ssf_config_default.restype = i32
    L.ssf_create.argtypes = [i32, C.POINTER(Config), C.POINTER(vp)]
    L.ssf_create.restype = i32
    L.ssf_destroy.argtypes = [vp]
    L.ssf_destroy.restype = None
    L.ssf_last_error.argtypes = [vp]
    L.ssf_last_error.restype = C.c_char_p
    L.ssf_reserve.argtypes = [vp, i32, i64]
    L.ssf_reserve.restype = i32
    L.ssf_rng_seed.argtypes = [vp, C.c_uint32]
    L.ssf_rng_seed.restype = i32
    L.ssf_extract_planes_batch.argtypes = [vp, vp, i32, vp, i32, vp, i64, i64, vp, vp, vp, vp, vp]
    L.ssf_extract_planes_batch.restype = i32
    L.ssf_extract_planes_batch_masked.argtypes = [vp, vp, i32, vp, i32, vp, i64, i64, vp, vp, vp, vp, vp, vp]
    L.ssf_extract_planes_batch_masked.restype = i32
    L.ssf_extract_planes.argtypes = [vp, vp, vp, i64, i32, i32, vp, C.POINTER(i64), i64]
    L.ssf_extract_planes.restype = i32
    L.ssf_plane_table_batch.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.ssf_plane_table_batch.restype = i32
    L.ssf_register_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64,
                                     vp, vp, vp, vp, vp, vp, vp, vp]
    L.ssf_register_batch.restype = i32
    L.ssf_register_chain.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, i64,
                                     vp, vp, vp, vp, vp, vp, vp]
    L.ssf_register_chain.restype = i32
    L.ssf_register_pair.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, C.POINTER(StepLog)]
    L.ssf_register_pair.restype = i32
    L.ssf_register_plan.argtypes = [i32, i64, i32, C.POINTER(LaunchPlan)]
    L.ssf_register_plan.restype = i32
    L.ssf_set_mask_split.argtypes = [vp, i32]
    L.ssf_set_mask_split.restype = i32
    L.ssf_set_mask_schedule.argtypes = [vp, vp, i32, i32]
    L.ssf_set_mask_schedule.restype = i32
    L.ssf_profile_enable.argtypes = [vp, i32]
    L.ssf_profile_enable.restype = i32
    L.ssf_profile_read.argtypes = [vp, C.POINTER(KernelTime), i32, C.POINTER(i32)]
    L.ssf_profile_read.restype = i32
    L.ssf_mask_pose_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp]
    L.ssf_mask_pose_batch.restype = i32
    L.ssf_mask_pose_batch_f64.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp]
    L.ssf_mask_pose_batch_f64.restype = i32
    L.ssf_kabsch_f32_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp]
    L.ssf_kabsch_f32_batch.restype = i32
    L.ssf_subsample_batch.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, i32, C.c_float, i32, i32,
                                      C.c_uint64, vp, i32, vp, vp, vp, vp]
    L.ssf_subsample_batch.restype = i32
    L.ssf_edge_config_default.argtypes = [i32, C.POINTER(EdgeConfig)]
    L.ssf_edge_config_default.restype = i32
    L.ssf_set_edge_config.argtypes = [vp, C.POINTER(EdgeConfig)]
    L.ssf_set_edge_config.restype = i32
    L.ssf_extract_features_batch.argtypes = [vp, vp, i32, vp, i32, vp, i64, i64, vp, vp, vp, vp, vp]
    L.ssf_extract_features_batch.restype = i32
    L.ssf_edge_table_batch.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, vp]
    L.ssf_edge_table_batch.restype = i32
    L.ssf_register_batch_edges.argtypes = ([vp, vp, i32] + [vp] * 10 + [i64, i64] + [vp] * 8 +
                                           [i64, i64] + [vp] * 8)
    L.ssf_register_batch_edges.restype = i32
    L.ssf_accumulate_sequence.argtypes = [vp, vp, i32, vp, vp, vp]
    L.ssf_accumulate_sequence.restype = i32
    L.ssf_voxel_grid_batch.argtypes = [vp, vp, i32, vp, vp, vp, C.c_float, vp, vp]
    L.ssf_voxel_grid_batch.restype = i32
    L.ssf_transform_clouds_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.ssf_transform_clouds_batch.restype = i32
    L.ssf_icp_params_default.argtypes = [C.POINTER(IcpParams)]
    L.ssf_icp_params_default.restype = i32
    L.ssf_icp_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, C.POINTER(IcpParams), vp, vp]
    L.ssf_icp_batch.restype = i32
    L.ssf_pgo_params_default.argtypes = [C.POINTER(PgoParams)]
    L.ssf_pgo_params_default.restype = i32
    L.ssf_pose_graph_batch.argtypes = [vp, vp, i32] + [vp] * 10 + [C.POINTER(PgoParams), vp, vp]
    L.ssf_pose_graph_batch.restype = i32
    L.ssf_pgo_robust_default.argtypes = [i32, C.POINTER(PgoRobust)]
    L.ssf_pgo_robust_default.restype = i32
    L.ssf_pose_graph_batch_robust.argtypes = [vp, vp, i32] + [vp] * 10 + [C.POINTER(PgoParams), vp, vp,
                                                                          C.POINTER(PgoRobust), vp]
    L.ssf_pose_graph_batch_robust.restype = i32
    L.ssf_pgo_lm_default.argtypes = [C.POINTER(PgoLm)]
    L.ssf_pgo_lm_default.restype = i32
    L.ssf_pose_graph_batch_lm.argtypes = [vp, vp, i32] + [vp] * 10 + [C.POINTER(PgoParams), vp, vp,
                                                                      C.POINTER(PgoRobust), vp,
                                                                      C.POINTER(PgoLm), vp]
    L.ssf_pose_graph_batch_lm.restype = i32
    L.ssf_sc_params_default.argtypes = [C.POINTER(ScParams)]
    L.ssf_sc_params_default.restype = i32
    L.ssf_scan_context_batch.argtypes = [vp, vp, i32, vp, i32, vp, vp, C.POINTER(ScParams), vp]
    L.ssf_scan_context_batch.restype = i32
    L.ssf_scan_context_match.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.ssf_scan_context_match.restype = i32
    L.ssf_scan_context_match_topk.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32]
    L.ssf_scan_context_match_topk.restype = i32
    L.ssf_pn2_last_error.argtypes = []
    L.ssf_pn2_last_error.restype = C.c_char_p
    L.ssf_pn2_furthest_point_sample.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.ssf_pn2_knn.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.ssf_pn2_three_nn.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.ssf_pn2_gather.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.ssf_pn2_three_interpolate.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.ssf_pn2_upsample_flow.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.ssf_pn2_group_relative.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.ssf_pn2_grouped_mlp_max.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp,
                                          vp, vp]
    L.ssf_pn2_grouped_mlp.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32,
                                      vp, vp, vp, vp, vp, i32, vp, vp]
    L.ssf_pn2_pair_attention.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.ssf_pn2_segment_softmax_sum.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    for name in PN2_EXPORTS[1:]:
        getattr(L, name).restype = i32
    _lib = L
    return L


def config_default(n_rows: int) -> Config:
    cfg = Config()
    if lib().ssf_config_default(n_rows, C.byref(cfg)) != SSF_OK:
        raise ValueError(f"unsupported N_SCAN_ROW {n_rows} (16 or 64)")
    return cfg

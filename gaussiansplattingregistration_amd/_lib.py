"""Loader of the C-ABI HIP library (csrc/libgsr_hip.so, declared in include/gsr_hip.h).

The product path has NO CPU fallback: if the library is missing, fails to load, or no HIP device
is visible, every entry point raises ``RuntimeError``.  Build it with ``__graft_entry__.build()``
(hipcc cross-compiles for gfx950 without a GPU).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_HIP_LIB") or os.path.join(_HERE, "csrc", "libgsr_hip.so")   # GSR_HIP_LIB: A/B builds

GSR_OK = 0
GSR_E_INVALID = -1
GSR_E_HIP = -2
GSR_E_NO_DEVICE = -3
GSR_E_PRECONDITION = -4

GSR_RNG_GLIBC = 0
GSR_RNG_HASH = 1

GSR_ICP_ACC_LEN = 32

GSR_COMM_ID_BYTES = 128

GSR_DECOMP_REFERENCE = 0
GSR_DECOMP_EXACT = 1

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_void_p)
ALLREDUCE_DEV_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int64, C.c_void_p)
ALLGATHER_DEV_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)

COMM_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p)
COMM_ALLGATHER_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
COMM_EXCHANGE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64),
                               C.POINTER(C.c_int64), C.c_void_p)


class CommCallbacks(C.Structure):          # struct gsr_comm_callbacks
    _fields_ = [("allreduce", COMM_ALLREDUCE_FN), ("allgather", COMM_ALLGATHER_FN), ("exchange", COMM_EXCHANGE_FN), ("user", C.c_void_p)]


# name -> (restype, argtypes); mirrors include/gsr_hip.h one to one (tests/test_abi.py checks it)
_vp, _i32, _i64, _u32, _u64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double
SIGNATURES = {
    "gsr_last_error": (C.c_char_p, []),
    "gsr_version": (C.c_char_p, []),
    "gsr_device_count": (_i32, []),
    "gsr_comm_get_unique_id": (_i32, [_vp]),
    "gsr_comm_create": (_i32, [C.POINTER(_vp), _vp, _i32, _i32, _i32]),
    "gsr_comm_create_callbacks": (_i32, [C.POINTER(_vp), _i32, _i32, _i32, C.POINTER(CommCallbacks)]),
    "gsr_comm_destroy": (_i32, [_vp]),
    "gsr_comm_rank": (_i32, [_vp]),
    "gsr_comm_world": (_i32, [_vp]),
    "gsr_comm_allreduce": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "gsr_comm_allgather": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "gsr_comm_exchange": (_i32, [_vp, _vp, C.POINTER(_i64), C.POINTER(_i64), _vp, C.POINTER(_i64), C.POINTER(_i64), _vp]),
    "gsr_hem_create": (_i32, [C.POINTER(_vp), _i32, _vp]),
    "gsr_hem_destroy": (_i32, [_vp]),
    "gsr_hem_set_params": (_i32, [_vp, _f32, _f32, _f32, _f32]),
    "gsr_hem_set_rng": (_i32, [_vp, _i32, _u32, _u64]),
    "gsr_hem_get_rng_position": (_i32, [_vp, C.POINTER(_u64)]),
    "gsr_hem_set_shard": (_i32, [_vp, _i32, _i32, ALLREDUCE_DEV_FN, ALLGATHER_DEV_FN, _vp]),
    "gsr_hem_set_level0": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "gsr_hem_set_state": (_i32, [_vp, _vp, _vp]),
    "gsr_hem_set_comm": (_i32, [_vp, _vp]),
    "gsr_hem_set_level0_part": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32]),
    "gsr_hem_get_gids": (_i32, [_vp, _vp, _i32]),
    "gsr_hem_set_output": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64]),
    "gsr_hem_get_part_stats": (_i32, [_vp, C.POINTER(_i64)]),
    "gsr_hem_get_part_ms": (_i32, [_vp, C.POINTER(C.c_float)]),
    "gsr_hem_run_level": (_i32, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "gsr_hem_run_levels": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "gsr_hem_level_size": (_i32, [_vp, C.POINTER(_i64), C.POINTER(_i32)]),
    "gsr_hem_get_level": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "gsr_hem_get_stats": (_i32, [_vp, C.POINTER(_i64)]),
    "gsr_hem_get_stats_ex": (_i32, [_vp, C.POINTER(_i64)]),
    "gsr_hem_get_phase_ms": (_i32, [_vp, C.POINTER(_f32)]),
    "gsr_hem_get_kernel_ms": (_i32, [_vp, C.POINTER(_f32)]),
    "gsr_hem_set_timing": (_i32, [_vp, _i32]),
    "gsr_icp_create": (_i32, [C.POINTER(_vp), _i32, _vp]),
    "gsr_icp_destroy": (_i32, [_vp]),
    "gsr_icp_set_target": (_i32, [_vp, _vp, _vp, _i64, _f64, _i32]),
    "gsr_icp_set_source": (_i32, [_vp, _vp, _i64, _i32]),
    "gsr_icp_set_target_cov": (_i32, [_vp, _vp, _i32]),
    "gsr_voxel_down_sample": (_i32, [_i32, _vp, _vp, _vp, _vp, _i64, _f64, _i32, C.POINTER(_vp), C.POINTER(_i64)]),
    "gsr_voxel_fetch": (_i32, [_vp, _vp, _vp, _vp, _i32]),
    "gsr_voxel_free": (_i32, [_vp]),
    "gsr_icp_set_source_cov": (_i32, [_vp, _vp, _i32]),
    "gsr_icp_set_target_color": (_i32, [_vp, _vp, _i32]),
    "gsr_icp_set_source_color": (_i32, [_vp, _vp, _i32]),
    "gsr_icp_set_lambda_geometric": (_i32, [_vp, _f64]),
    "gsr_icp_get_color_gradient": (_i32, [_vp, _vp]),
    "gsr_icp_set_allreduce": (_i32, [_vp, ALLREDUCE_FN, _vp, _i64]),
    "gsr_icp_set_allreduce_dev": (_i32, [_vp, ALLREDUCE_DEV_FN, _vp, _i64]),
    "gsr_icp_set_comm": (_i32, [_vp, _vp, _i64]),
    "gsr_icp_accumulate": (_i32, [_vp, _vp, _i32, _i32, _f64, _vp]),
    "gsr_icp_register_clouds": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _vp, _i32, _i32, _f64, _f64, _f64, _i32, _vp, C.POINTER(_f64),
                                       C.POINTER(_f64), C.POINTER(_i32)]),
    "gsr_icp_register_multiscale": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _f64, _f64, _f64, _vp, _vp]),
    "gsr_icp_register": (_i32, [_vp, _vp, _i32, _i32, _f64, _f64, _f64, _i32, _vp, C.POINTER(_f64), C.POINTER(_f64),
                                C.POINTER(_i32)]),
    "gsr_icp_correspondences": (_i32, [_vp, _vp, _vp, _vp]),
    "gsr_icp_information": (_i32, [_vp, _vp, _vp, C.POINTER(_i64)]),
    "gsr_icp_get_timing": (_i32, [_vp, C.POINTER(_f32)]),
    "gsr_normals_from_cov": (_i32, [_vp, _i64, _vp, _i32, _i32, _vp]),
    "gsr_normals_knn": (_i32, [_vp, _i64, _i32, _vp, _i32, _i32, _vp]),
    "gsr_cov_from_normals": (_i32, [_vp, _i64, _f64, _vp, _i32, _i32, _vp]),
    "gsr_decompose_cov": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_cov_build": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32, _vp]),
    "gsr_cov_build_backward": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _vp]),
    "gsr_ply_unpack": (_i32, [_vp, _i64, _i32, C.POINTER(_i32), _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "gsr_ply_pack": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp]),
    "gsr_sh_rotation": (_i32, [_vp, _i32, _vp]),
    "gsr_model_transform": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_model_similarity": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_model_fuse": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_model_match": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_color_sums": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _f64, _vp, C.POINTER(_i64), C.POINTER(_i64), _i32, _i32, _vp]),
    "gsr_color_solve": (_i32, [_i32, _vp, _i32, _vp, _i32, _f64, _i64, _i32, _vp, _vp]),
    "gsr_model_color_apply": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_fuse_multi": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_outlier_mask": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_model_select": (_i32, [_vp, _i32, _vp, _vp, _vp, C.POINTER(_i64), _i32, _i32, _vp]),
    "gsr_orient_normals_graph": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_orient_normals": (_i32, [_vp, _vp, _i64, _f64, _i32, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_plane_score": (_i32, [_vp, _vp, _i64, _vp, _i32, _f32, _f32, _vp, _vp, C.POINTER(_i32), _i32, _i32, _vp]),
    "gsr_icp_solve": (_i32, [_vp, _i32, _vp, _vp]),
    "gsr_icp_get_centre": (_i32, [_vp, _vp]),
    "gsr_hybrid_search": (_i32, [_vp, _i64, _f64, _i32, _vp, _vp, _i32, _i32, _vp]),
    "gsr_fpfh": (_i32, [_vp, _vp, _i64, _f64, _i32, _vp, _i32, _i32, _vp]),
    "gsr_feature_match": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, C.POINTER(_i64), C.POINTER(_i32), _vp, _vp, _i32, _i32, _vp]),
    "gsr_ransac_correspondence": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _vp]),
    "gsr_fgr_tuple_test": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), _i32, _i32, _vp]),
    "gsr_fgr_optimize": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _i32, _vp]),
    "gsr_sc2_correspondence": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _i32, _vp]),
    "gsr_posegraph_optimize": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "gsr_raster_create": (_i32, [C.POINTER(_vp), _i32, _vp]),
    "gsr_raster_destroy": (_i32, [_vp]),
    "gsr_raster_render": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), _f32, _f32, _f32, _f32, _i32, _i32, C.POINTER(_f32), _f32,
                                 _vp, _vp, _vp]),
    "gsr_raster_render_aux": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), _f32, _f32, _f32, _f32, _i32, _i32, C.POINTER(_f32), _f32,
                                     _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_raster_get_timing": (_i32, [_vp, C.POINTER(_f32)]),
    "gsr_raster_backward": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), _f32, _f32, _f32, _f32, _i32, _i32, C.POINTER(_f32), _f32,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gsr_raster_get_backward_timing": (_i32, [_vp, C.POINTER(_f32)]),
    "gsr_image_metrics": (_i32, [_vp, _vp, _i32, _i32, _i32, C.POINTER(_f64), _i32, _vp]),
    "gsr_photo_accumulate": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.POINTER(_f64), _f64, _f64, _f64, _f64, _f64, _f64, _f64, _i32,
                                    C.POINTER(_f64), _i32, _vp]),
    "gsr_warp_create": (_i32, [C.POINTER(_vp), _i32, _vp]),
    "gsr_warp_destroy": (_i32, [_vp]),
    "gsr_warp_set_target": (_i32, [_vp, _vp, _vp, _i64, _f64, _i32]),
    "gsr_warp_set_source": (_i32, [_vp, _vp, _i64, _i32]),
    "gsr_warp_accumulate": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_f64)]),
    "gsr_warp_points": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _vp]),
    "gsr_model_warp": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, C.POINTER(_i64), _i32, _i32, _vp]),
    "gsr_warp_solve": (_i32, [_vp, _vp, _f64, _f64, _vp, _vp]),
    "gsr_d2d_create": (_i32, [C.POINTER(_vp), _i32, _vp]),
    "gsr_d2d_destroy": (_i32, [_vp]),
    "gsr_d2d_set_target": (_i32, [_vp, _vp, _vp, _vp, _i64, _f64, _i32]),
    "gsr_d2d_set_source": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "gsr_d2d_accumulate": (_i32, [_vp, _vp, _f64, _f64, _vp]),
    "gsr_d2d_register": (_i32, [_vp, _vp, _f64, _f64, _f64, _i32, _vp, _vp]),
    "gsr_loss_create": (_i32, [_i32, C.POINTER(_vp)]),
    "gsr_loss_destroy": (_i32, [_vp]),
    "gsr_loss_l1_dssim": (_i32, [_vp, _vp, _vp, _i32, _i32, _f64, _vp, _vp, _vp]),
}
# private test hooks (csrc/gsr_test_hooks.h): exported by the library, not part of the public header
TEST_HOOKS = {
    "gsr_debug_logf": (_i32, [_vp, _i64, _vp, _i32]),
    "gsr_debug_kld": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i32]),
    "gsr_debug_kl_gate": (_i32, [_vp, _vp, _vp, _i64, _f32, _vp, _vp, _vp, _i32]),
    "gsr_debug_stage1": (_i32, [_vp, _vp, _vp, _vp, _i64, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "gsr_debug_ransac_sample": (_i32, [_u64, _i64, _i64, _i64, _i32, _vp]),
    "gsr_debug_fold": (_i32, [_vp, _i64, _i32, _i32, _vp, _i32]),
    "gsr_test_i8_gemm_nt": (_i32, [_vp, _i64, _vp, _i64, _i64, _vp, _i32]),
    "gsr_test_sc2_timed": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp]),
    "gsr_test_sc2_stages": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
}

_lib = None


class HemLevelReport(C.Structure):
    """gsr_hem_level_report (include/gsr_hip.h): what gsr_hem_run_levels reports per level."""
    _fields_ = [("offset_rows", C.c_int64), ("rows", C.c_int64), ("dropped", C.c_int64), ("rng_position", C.c_uint64),
                ("stats", C.c_int64 * 8), ("stats_ex", C.c_int64 * 8), ("phase_ms", C.c_float * 8), ("kernel_ms", C.c_float * 8)]


class IcpEntry(C.Structure):
    """gsr_icp_entry (include/gsr_hip.h): one entry of a coarse-to-fine schedule."""
    _fields_ = [("src_xyz", C.c_void_p), ("ns", C.c_int64), ("tgt_xyz", C.c_void_p), ("tgt_normals", C.c_void_p), ("nt", C.c_int64),
                ("max_corr", C.c_double), ("max_iter", C.c_int32), ("reserved", C.c_int32)]


class IcpEntryResult(C.Structure):
    """gsr_icp_entry_result (include/gsr_hip.h)."""
    _fields_ = [("init_T", C.c_double * 16), ("T", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("iterations", C.c_int32), ("evaluations", C.c_int32), ("ms_build", C.c_float), ("ms_iters", C.c_float)]


class RansacParams(C.Structure):
    """gsr_ransac_params (include/gsr_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("ransac_n", C.c_int32), ("max_corr", C.c_double), ("max_iteration", C.c_int64),
                ("confidence", C.c_double), ("seed", C.c_uint64), ("batch", C.c_int32), ("n_checkers", C.c_int32),
                ("checker_kind", C.c_int32 * 4), ("checker_param", C.c_double * 4)]


class RansacResult(C.Structure):
    """gsr_ransac_result (include/gsr_hip.h)."""
    _fields_ = [("T", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double), ("best_index", C.c_int64),
                ("n_evaluated", C.c_int64), ("n_valid", C.c_int64), ("exit_index", C.c_int64)]


class FgrOptions(C.Structure):
    """gsr_fgr_options (include/gsr_hip.h)."""
    _fields_ = [("division_factor", C.c_double), ("use_absolute_scale", C.c_int32), ("decrease_mu", C.c_int32),
                ("maximum_correspondence_distance", C.c_double), ("iteration_number", C.c_int32), ("maximum_tuple_count", C.c_int32),
                ("tuple_scale", C.c_double), ("tuple_test", C.c_int32), ("batch", C.c_int32), ("seed", C.c_uint64)]


class FgrResult(C.Structure):
    """gsr_fgr_result (include/gsr_hip.h)."""
    _fields_ = [("T", C.c_double * 16), ("n_corres", C.c_int64), ("n_reciprocal", C.c_int64), ("n_trials", C.c_int64),
                ("n_tuples", C.c_int64), ("iterations", C.c_int32), ("host_waits", C.c_int32), ("scale_global", C.c_double)]


class Sc2Params(C.Structure):
    """gsr_sc2_params (include/gsr_hip.h)."""
    _fields_ = [("d_thr", C.c_double), ("seed_ratio", C.c_double), ("max_seeds", C.c_int32), ("k1", C.c_int32), ("k2", C.c_int32),
                ("refine_iters", C.c_int32)]


class Sc2Result(C.Structure):
    """gsr_sc2_result (include/gsr_hip.h)."""
    _fields_ = [("T", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double), ("best_seed", C.c_int64), ("best_index", C.c_int64),
                ("n_seeds", C.c_int64), ("n_valid", C.c_int64), ("n_edges", C.c_int64), ("refine_steps", C.c_int32), ("host_waits", C.c_int32)]


class ModelView(C.Structure):
    """gsr_model_view (include/gsr_hip.h): the arrays of one splat model."""
    _fields_ = [("n", C.c_int64), ("xyz", C.c_void_p), ("cov6", C.c_void_p), ("dc", C.c_void_p), ("sh", C.c_void_p), ("opacity", C.c_void_p),
                ("scaling", C.c_void_p), ("rot", C.c_void_p)]


class FuseParams(C.Structure):
    """gsr_fuse_params (include/gsr_hip.h)."""
    _fields_ = [("max_distance", C.c_double), ("kld_max", C.c_double), ("color_delta", C.c_double)]


class FuseReport(C.Structure):
    """gsr_fuse_report (include/gsr_hip.h)."""
    _fields_ = [("n_out", C.c_int64), ("n_pairs", C.c_int64), ("n_a_only", C.c_int64), ("n_b_only", C.c_int64), ("n_invalid_a", C.c_int64),
                ("n_invalid_b", C.c_int64), ("gated_pairs", C.c_int64), ("workspace_bytes", C.c_int64), ("phase_ms", C.c_float * 4)]


GSR_FUSE_MAX_MODELS = 16


class FuseMultiReport(C.Structure):
    """gsr_fuse_multi_report (include/gsr_hip.h)."""
    _fields_ = [("n_out", C.c_int64), ("n_groups", C.c_int64), ("n_grouped_rows", C.c_int64), ("n_invalid", C.c_int64), ("gated_pairs", C.c_int64),
                ("mutual_edges", C.c_int64), ("rejected_edges", C.c_int64), ("rounds", C.c_int64), ("workspace_bytes", C.c_int64),
                ("groups_of_size", C.c_int64 * (GSR_FUSE_MAX_MODELS + 1)), ("phase_ms", C.c_float * 6)]


class CleanParams(C.Structure):
    """gsr_clean_params (include/gsr_hip.h)."""
    _fields_ = [("min_raw_opacity", C.c_double), ("max_log_scale", C.c_double), ("nb_neighbors", C.c_int32), ("reserved0", C.c_int32),
                ("std_ratio", C.c_double), ("radius", C.c_double), ("nb_points", C.c_int32), ("reserved1", C.c_int32)]


class CleanReport(C.Structure):
    """gsr_clean_report (include/gsr_hip.h)."""
    _fields_ = [("n", C.c_int64), ("n_nonfinite", C.c_int64), ("n_gate_opacity", C.c_int64), ("n_gate_scale", C.c_int64), ("n_statistical", C.c_int64),
                ("n_radius", C.c_int64), ("n_kept", C.c_int64), ("cloud_mean", C.c_double), ("std_dev", C.c_double), ("threshold", C.c_double),
                ("deferred_queries", C.c_int64), ("workspace_bytes", C.c_int64), ("phase_ms", C.c_float * 4)]


class OrientReport(C.Structure):
    """gsr_orient_report (include/gsr_hip.h)."""
    _fields_ = [("n", C.c_int64), ("n_components", C.c_int64), ("n_flipped", C.c_int64), ("n_not_live", C.c_int64), ("rounds", C.c_int32),
                ("reserved", C.c_int32), ("workspace_bytes", C.c_int64), ("phase_ms", C.c_float * 4)]


class PoseEdge(C.Structure):
    """gsr_pose_edge (include/gsr_hip.h)."""
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("uncertain", C.c_int32), ("reserved", C.c_int32), ("T", C.c_double * 16),
                ("information", C.c_double * 36)]


class PoseGraphOption(C.Structure):
    """gsr_posegraph_option (include/gsr_hip.h)."""
    _fields_ = [("max_correspondence_distance", C.c_double), ("edge_prune_threshold", C.c_double), ("preference_loop_closure", C.c_double),
                ("reference_node", C.c_int32), ("max_iteration", C.c_int32), ("max_iteration_lm", C.c_int32), ("reserved", C.c_int32),
                ("min_relative_increment", C.c_double), ("min_relative_residual_increment", C.c_double), ("min_right_term", C.c_double),
                ("min_residual", C.c_double)]


class PoseGraphResult(C.Structure):
    """gsr_posegraph_result (include/gsr_hip.h)."""
    _fields_ = [("iterations", C.c_int32 * 2), ("n_pruned", C.c_int32), ("reserved", C.c_int32), ("E_initial", C.c_double), ("E_final", C.c_double),
                ("mu", C.c_double), ("mu_first", C.c_double)]


GSR_COLOR_SUMS_LEN = 40
GSR_PHOTO_SUMS_LEN = 30
GSR_COLOR_MODES = {"gain": 0, "channel_gain": 1, "affine": 2}


class ColorEdge(C.Structure):
    """gsr_color_edge (include/gsr_hip.h)."""
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("sums", C.c_double * GSR_COLOR_SUMS_LEN)]


class ColorSolveResult(C.Structure):
    """gsr_color_solve_result (include/gsr_hip.h)."""
    _fields_ = [("E_initial", C.c_double), ("E_final", C.c_double), ("pivot_min", C.c_double), ("pivot_max", C.c_double), ("n_free", C.c_int32),
                ("n_unknowns", C.c_int32)]


GSR_WARP_CELL_LEN = 326


class WarpReport(C.Structure):
    """gsr_warp_report (include/gsr_hip.h)."""
    _fields_ = [("E_before", C.c_double), ("E_after", C.c_double), ("E_data_before", C.c_double), ("E_data_after", C.c_double), ("n_corr", C.c_int64),
                ("n_unknowns", C.c_int32), ("half_band", C.c_int32), ("pivot_min", C.c_double), ("pivot_max", C.c_double)]


GSR_D2D_SUMS_LEN = 32
GSR_D2D_STATUS = {0: "converged", 1: "max_iteration", 2: "no_pairs", 3: "degenerate"}


class D2DReport(C.Structure):
    """gsr_d2d_report (include/gsr_hip.h)."""
    _fields_ = [("score", C.c_double), ("fitness", C.c_double), ("mahalanobis_rmse", C.c_double), ("n_pairs", C.c_int64), ("n_singular", C.c_int64),
                ("iterations", C.c_int32), ("status", C.c_int32)]


GSR_CHECK_EDGE_LENGTH = 0
GSR_CHECK_DISTANCE = 1
GSR_CHECK_NORMAL = 2
GSR_RANSAC_MAX_N = 16
GSR_HYBRID_MAX_NN = 512
GSR_SC2_MAX_CORRES = 32768
GSR_SC2_MAX_K = 64


def load(require_device: bool = False):
    """Return the ctypes handle of libgsr_hip.so; raise RuntimeError if it cannot serve the hot path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"HIP extension missing: {LIB_PATH} not built.  Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(needs hipcc).  This backend has no CPU fallback.")
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the machine
            raise RuntimeError(f"HIP extension failed to load ({LIB_PATH}): {e}.  This backend has no CPU fallback.") from e
        for name, (res, args) in list(SIGNATURES.items()) + list(TEST_HOOKS.items()):
            fn = getattr(lib, name)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    if require_device and _lib.gsr_device_count() <= 0:
        raise RuntimeError("no HIP device visible: the MI355X backend has no CPU fallback")
    return _lib


def check(code: int, what: str = ""):
    if code != GSR_OK:
        msg = load().gsr_last_error()
        msg = msg.decode("utf-8", "replace") if msg else ""
        raise RuntimeError(f"{what or 'gsr'} failed ({code}): {msg}")

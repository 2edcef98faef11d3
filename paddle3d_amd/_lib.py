"""ctypes loader for libpaddle3d_amd.so (the C ABI declared in include/paddle3d_amd.h).

There is NO fallback: if the shared object is missing, was built for another ABI, or lacks a symbol,
importing an op raises.  A GPU box must never silently run a PyTorch/CPU substitute.
"""
from __future__ import annotations

import ctypes as C
import os
from functools import lru_cache

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpaddle3d_amd.so")

c_f32p = C.c_void_p
c_i32p = C.c_void_p

# ONE table: symbol -> (restype, argtypes, scenarios).  restype / argtypes mirror include/paddle3d_amd.h one to one
# (tests/test_abi.py holds every row to the header); `scenarios` is the bare name of the test module whose guarded
# scenarios (tests/guarded.py: Protocol) have to reach the entry point -- that module's last test fails until one does.
# A new entry point is one row in the block of the module that holds its scenarios.
ENTRY_POINTS = {}


def _block(scenarios, rows):
    for name, (res, args) in rows.items():
        if name in ENTRY_POINTS:
            raise ValueError(f"{name} has a row in the block of {ENTRY_POINTS[name][2]} "
                             f"and another in that of {scenarios}")
        ENTRY_POINTS[name] = (res, args, scenarios)


def symbols(module=None):
    """Every name of ENTRY_POINTS in table order, or those (of any table: _tables(), then LATER_TABLES, then LAST_TABLES)
    whose guarded scenarios live in tests/<module>.py."""
    if module is None:
        return tuple(ENTRY_POINTS)
    return tuple(name for table in (*_tables(), *LATER_TABLES, *LAST_TABLES) for name, row in table.items()
                 if row[2] == module)


def _tables():
    """ENTRY_POINTS and every side table, in the order they are bound."""
    return (ENTRY_POINTS, *SIDE_TABLES)


# the first models' ops: voxelization, pillar encoders, NMS, post-processing, point ops, sparse and dense convolutions
_block("test_memory_safety_gpu", {
    "pd3_version": (C.c_int, []),
    "pd3_target_arch": (C.c_char_p, []),
    "pd3_hard_voxelize_workspace": (C.c_size_t, [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_int]),
    "pd3_hard_voxelize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_hard_voxelize_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_hard_voxelize_path": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    "pd3_hard_voxelize_index_list_entries": (C.c_int64, [C.c_int, C.c_int64]),
    "pd3_hard_voxelize_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_pillar_feature_net_indexed": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                                 C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p]),
    "pd3_pointpillars_scatter_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pd3_pointpillars_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_pillar_feature_net": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                         C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_pillar_feature_net_path": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                              C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                              C.c_float, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "pd3_voxel_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p]),
    "pd3_nms_workspace": (C.c_size_t, [C.c_int]),
    "pd3_nms_bev": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_size_t, C.c_void_p]),
    "pd3_nms_normal": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    "pd3_boxes_iou_bev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_boxes_overlap_bev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    "pd3_libm_eval": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "pd3_centerpoint_postprocess_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "pd3_centerpoint_postprocess": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_centerpoint_postprocess_strided": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    "pd3_centerpoint_postprocess_records": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_ms_deform_attn_forward": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 7 + [C.c_void_p] * 2),
    "pd3_ms_deform_attn_backward": (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 7 + [C.c_void_p] * 4),
    "pd3_farthest_point_sample_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pd3_farthest_point_sample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p]),
    "pd3_gather_points": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]),
    "pd3_gather_points_grad": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]),
    "pd3_ball_query_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "pd3_group_points_batch": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "pd3_group_points_batch_grad": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "pd3_points_in_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                      C.c_void_p, C.c_void_p]),
    "pd3_ball_query_stack": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_float, C.c_int, C.c_void_p,
                                                                            C.c_void_p]),
    "pd3_voxel_query": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_float] + [C.c_int] * 4 + [C.c_void_p] * 2),
    "pd3_group_points_stack": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 2),
    "pd3_group_points_stack_grad": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 2),
    "pd3_assign_score_withk_forward": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 2),
    "pd3_assign_score_withk_backward_workspace": (C.c_size_t, [C.c_int] * 4),
    "pd3_assign_score_withk_backward": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p] * 4 +
                                        [C.c_size_t, C.c_void_p]),
    "pd3_bev_pool_v2": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                                     C.c_void_p]),
    "pd3_bev_pool_v2_bkwd": (C.c_int, [C.c_void_p] * 8 + [C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "pd3_frustum_to_lidar": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 7),
    "pd3_voxel_pooling_prepare_workspace": (C.c_size_t, [C.c_int64]),
    "pd3_voxel_pooling_prepare": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]),
    "pd3_sparse_conv3d_workspace": (C.c_size_t, [C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "pd3_sparse_conv3d_indices": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_sparse_conv3d_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_sparse_conv3d_features_ordered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pd3_sparse_pack_weight_bf16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_sparse_conv3d_features_bf16x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pd3_sparse_pack_weight_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_sparse_conv3d_features_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pd3_gather_gemm_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pd3_sparse_tile_order_entries": (C.c_int64, [C.c_int]),
    "pd3_sparse_tile_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_sparse_plan_workspace": (C.c_size_t, [C.c_int]),
    "pd3_sparse_conv_outputs_workspace": (C.c_size_t, [C.c_int] + [C.c_void_p] * 4),
    "pd3_sparse_sort_coords": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_sparse_conv_outputs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_size_t, C.c_void_p]),
    "pd3_sparse_rulebook_workspace": (C.c_size_t, [C.c_int, C.c_void_p]),
    "pd3_sparse_rulebook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_sparse_to_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "pd3_selfcheck_lds_atomic_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p]),
    "pd3_selfcheck_block_topk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pd3_conv3x3_f16_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pd3_f32_nchw_to_f16_nhwc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_conv3x3_f16_bias_relu_dual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pd3_conv3x3_s2_f16_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_scatter_conv3x3_s2_f16_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                       C.c_void_p]),
    "pd3_grouped_conv3x3_small_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pd3_grouped_conv3x3_small_f16_gm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pd3_stable_argsort_workspace": (C.c_size_t, [C.c_int64, C.c_uint32]),
    "pd3_stable_argsort": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "pd3_conv3x3_winograd43_pp_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_conv3x3_winograd43_pp_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pd3_merge_sweeps_workspace": (C.c_size_t, [C.c_int64]),
    "pd3_merge_sweeps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "pd3_dynamic_voxelize": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pd3_conv3x3_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "pd3_conv3x3_winograd_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_conv3x3_winograd43_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                   C.c_void_p]),
    "pd3_patch_conv_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p]),
    "pd3_patch_conv_x3_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p]),
    "pd3_conv3x3_s2_x3_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "pd3_winograd43_input_transform_floats": (C.c_size_t, [C.c_int] * 4),
    "pd3_winograd43_input_transform": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p]),
    "pd3_conv3x3_winograd43_ppv_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_ssd_postprocess_workspace": (C.c_size_t, [C.c_int] * 7),
    "pd3_ssd_postprocess": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_int]),
    "pd3_pointpillars_inverse_map": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p]),
    "pd3_scatter_conv3x3_bias_relu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                C.c_void_p]),
    "pd3_pillar_conv_rulebook_workspace": (C.c_size_t, [C.c_int] * 4),
    "pd3_pillar_conv_rulebook": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p]),
    "pd3_rows_to_dense_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "pd3_bevdet_postprocess_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pd3_bevdet_postprocess": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_circle_nms_workspace": (C.c_size_t, [C.c_int]),
    "pd3_circle_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "pd3_bevdet4d_align": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 12),
    "pd3_grouped_conv3x3_small": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pd3_grouped_conv3x3_small_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_void_p]),
})

# Voxel R-CNN's RoI head (csrc/roi_head.hip)
_block("test_memory_safety_roi_gpu", {
    "pd3_voxel_pool": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 7 + [C.c_float] + [C.c_int] * 5 + [C.c_void_p] * 2),
    "pd3_roi_grid_points": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] +
                            [C.c_void_p] * 3),
    "pd3_rcnn_decode_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "pd3_class_agnostic_nms_workspace": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "pd3_class_agnostic_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_float,
                                         C.c_void_p, C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 5 +
                               [C.c_size_t, C.c_void_p]),
})

# the final SeparateHead convolutions with per-group channel counts (csrc/conv3x3.hip)
_block("test_grouped_counts_gpu", {
    "pd3_grouped_conv3x3_small_counts_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                         C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                         C.c_int, C.c_void_p]),
})

# PV-RCNN's keypoint branch and RoI head (csrc/pvrcnn.hip)
_block("test_memory_safety_pvrcnn_gpu", {
    "pd3_stack_sa_pool": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 5 + [C.c_float, C.c_int] + [C.c_void_p] * 2),
    "pd3_bev_interpolate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int] * 4 + [C.c_float] * 5 +
                            [C.c_void_p] * 2),
})

# CaDDN's frustum-to-voxel and map-to-BEV stage (csrc/caddn.hip)
_CADDN_GRID = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int, C.c_double, C.c_double]  # grid, pc_min, voxel_size, mode, depths
_CADDN_IN = [C.c_void_p] * 5 + [C.c_int] * 5 + _CADDN_GRID  # features, logits, calibration, image_shape, B, C, D, h, w
_block("test_memory_safety_caddn_gpu", {
    "pd3_frustum_grid": (C.c_int, [C.c_void_p] * 3 + [C.c_int] + _CADDN_GRID + [C.c_int] + [C.c_void_p] * 2),
    "pd3_frustum_to_voxel_workspace": (C.c_size_t, [C.c_int] * 5),
    "pd3_frustum_to_voxel": (C.c_int, _CADDN_IN + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pd3_frustum_to_bev_workspace": (C.c_size_t, [C.c_int] * 7),
    "pd3_frustum_to_bev": (C.c_int, _CADDN_IN + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                                    C.c_void_p]),
})

# BEVFormer's encoder attention (csrc/bevformer.hip)
_block("test_memory_safety_bevformer_gpu", {
    "pd3_bevformer_point_sampling": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p] * 5),
    "pd3_bevformer_sca": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 9 + [C.c_void_p] * 2),
    "pd3_bevformer_tsa": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 7 + [C.c_void_p] * 2),
})

# BEVFormer's decoder, head and NMS-free decode (csrc/bevformer_decoder.hip)
_block("test_memory_safety_bevformer_dec_gpu", {
    "pd3_mha_forward": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_float] + [C.c_void_p] * 2),
    "pd3_bevformer_dec_ca": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 8 + [C.c_void_p] * 2),
    "pd3_nms_free_decode": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_double, C.c_int] + [C.c_void_p] * 5),
})

# PETR / PETRv2's head (csrc/petr.hip)
_block("test_memory_safety_petr_gpu", {
    "pd3_mha_stream_forward": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_float] + [C.c_void_p] * 2),
    "pd3_petr_coords3d": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 4),
})

# SqueezeSegV3's SAC block and range projection (csrc/squeezeseg.hip)
_block("test_memory_safety_squeezeseg_gpu", {
    "pd3_sac_isk_forward": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_void_p] * 2),
    "pd3_range_project": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int] * 3 + [C.c_double] * 2 +
                          [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p]),
})

# BEVFusion's Anchor3DHead (csrc/anchor3d_head.hip)
_A3D_CFG = [C.c_int] * 2 + [C.c_float] * 4 + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]  # nms_pre .. stream
_block("test_memory_safety_anchor3d_gpu", {
    "pd3_anchor3d_head_workspace": (C.c_size_t, [C.c_int] * 7),
    "pd3_anchor3d_head_forward": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 7 + _A3D_CFG),
    "pd3_anchor3d_get_bboxes": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + _A3D_CFG),
})

# the sparse first backbone layer as one launch (csrc/pillar_conv_span.hip)
_block("test_pillar_conv_span_gpu", {
    "pd3_pillar_conv_span_x3": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3 +
                                [C.c_int] + [C.c_void_p] * 2),
})

# IA-SSD's fused set abstraction and box decode (csrc/iassd.hip)
_block("test_memory_safety_iassd_gpu", {
    "pd3_sa_msg_pool": (C.c_int, [C.c_void_p] * 12 + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_void_p, C.c_int64,
                                                                     C.c_void_p]),
    "pd3_iassd_decode": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int] +
                         [C.c_void_p] * 2),
})

# SMOKE's head and post-processing (csrc/smoke.hip)
_SMOKE_CFG = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]
_block("test_memory_safety_smoke_gpu", {
    "pd3_smoke_head_workspace": (C.c_size_t, [C.c_int] * 5),
    "pd3_smoke_head_forward": (C.c_int, [C.c_void_p] * 2 + [C.c_int64, C.c_int] + [C.c_void_p] * 15 + [C.c_int] * 6 +
                               _SMOKE_CFG),
    "pd3_smoke_post_process": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 4 + _SMOKE_CFG),
})

# DD3D's FCOS heads and post-processing (csrc/dd3d.hip)
_DD3D_CFG = [C.c_int] * 4 + [C.c_float] * 5 + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]  # pre_nms_topk .. stream
_block("test_memory_safety_dd3d_gpu", {
    "pd3_dd3d_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "pd3_dd3d_head_forward": (C.c_int, [C.c_void_p] * 12 + [C.c_int] * 6 + _DD3D_CFG),
    "pd3_dd3d_post_process": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 4 + _DD3D_CFG),
})

# BEV-LaneDet's lane head tail and lane post-processing (csrc/lanedet.hip), declared in include/paddle3d_amd_lanedet.h.
# A table of its own beside ENTRY_POINTS (whose size and blocks tests/test_abi.py pins), in the same row format;
# tests/test_abi_lanedet.py holds it to its header, and symbols("test_memory_safety_lanedet_gpu") names its rows.
_LANEDET_CFG = ([C.c_int] * 4 + [C.c_float] * 2 + [C.c_int] + [C.c_double] * 3 + [C.c_void_p] * 10 +
                [C.c_size_t, C.c_void_p])  # batch .. stream
LANEDET_ENTRY_POINTS = {name: row + ("test_memory_safety_lanedet_gpu",) for name, row in {
    "pd3_lanedet_workspace": (C.c_size_t, [C.c_int] * 4),
    "pd3_lanedet_post_process": (C.c_int, [C.c_void_p] * 4 + [C.c_int] + _LANEDET_CFG),
    "pd3_lanedet_head_forward": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 8 +
                                 _LANEDET_CFG),
}.items()}

# CAPE / CAPE-T's cross-view attention core and 3D position embedding (csrc/cape.hip), declared in
# include/paddle3d_amd_cape.h; tests/test_abi_cape.py holds the table to its header.
CAPE_ENTRY_POINTS = {name: row + ("test_memory_safety_cape_gpu",) for name, row in {
    "pd3_cape_cva_forward": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 6 + [C.c_void_p] * 2),
    "pd3_cape_posemb3d": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p] * 2),
}.items()}

# the tables beside ENTRY_POINTS, each with a header of its own: symbols(module) and lib() walk this tuple
SIDE_TABLES = (LANEDET_ENTRY_POINTS, CAPE_ENTRY_POINTS)

# The modulated deformable convolution (csrc/deform_conv.hip), declared in include/paddle3d_amd_dcn.h;
# tests/test_abi_dcn.py holds the table to its header.
DCN_ENTRY_POINTS = {name: row + ("test_memory_safety_dcn_gpu",) for name, row in {
    "pd3_deform_conv2d_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                            C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 9 + [C.c_void_p] * 2),
}.items()}

# the tables added after SIDE_TABLES (which tests/test_abi_cape.py pins, as it pins _tables()): symbols(module) and lib()
# walk this tuple after _tables()
LATER_TABLES = (DCN_ENTRY_POINTS,)

# BEVDepth's DepthNet: the ASPP and the softmax / channels-last tail (csrc/depthnet.hip), declared in
# include/paddle3d_amd_depthnet.h; tests/test_abi_depthnet.py holds the table to its header.
DEPTHNET_ENTRY_POINTS = {name: row + ("test_memory_safety_depthnet_gpu",) for name, row in {
    "pd3_aspp_workspace": (C.c_size_t, [C.c_int] * 5),
    "pd3_aspp_forward": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 8 + [C.c_void_p] * 2 + [C.c_size_t, C.c_void_p]),
    "pd3_depth_softmax_split": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3),
}.items()}

# the tables added after LATER_TABLES (which tests/test_abi_dcn.py pins): symbols(module) and lib() walk this tuple last
LAST_TABLES = (DEPTHNET_ENTRY_POINTS,)


class Paddle3DAmdError(RuntimeError):
    pass


@lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise Paddle3DAmdError(
            f"{LIB_PATH} not found: build it with `python -m paddle3d_amd.build` "
            "(there is no CPU / PyTorch fallback for the HIP ops)")
    handle = C.CDLL(LIB_PATH)
    for name, (res, args, _) in [row for table in (*_tables(), *LATER_TABLES, *LAST_TABLES) for row in table.items()]:
        try:
            fn = getattr(handle, name)
        except AttributeError as e:  # pragma: no cover
            raise Paddle3DAmdError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    return handle


def check(status: int, what: str) -> None:
    if status == 0:
        return
    if status < 0:
        msg = {-1: "invalid argument", -2: "workspace too small", -3: "unsupported configuration"}.get(
            status, "error")
        raise Paddle3DAmdError(f"{what}: {msg} (status {status})")
    raise Paddle3DAmdError(f"{what}: HIP error {status}")

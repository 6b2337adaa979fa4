"""ctypes binding of libpn2_hip.so (the C ABI declared in include/pn2.h).

The HIP library is the only compute path of this package: if it is missing or a symbol
cannot be resolved this module raises -- there is no CPU or eager-PyTorch fallback.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PN2_LIB_PATH") or os.path.join(_HERE, "libpn2_hip.so")   # override: A/B runs of two builds
CSRC = os.path.join(_HERE, "csrc")

_vp, _i, _i64, _f, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double

# name -> (restype, argtypes); mirrors include/pn2.h one to one (tests check the header against this table)
SIGNATURES = {
    "pn2_version": (_i, []),
    "pn2_error_string": (ctypes.c_char_p, [_i]),
    "pn2_last_kernel": (ctypes.c_char_p, []),
    "pn2_clear_last_kernel": (None, []),
    "pn2_set_option": (_i, [ctypes.c_char_p, _i]),
    "pn2_get_option": (_i, [ctypes.c_char_p, _vp]),
    "pn2_option_name": (ctypes.c_char_p, [_i]),
    "pn2_fps_workspace_bytes": (_i64, [_i, _i, _i]),
    "pn2_fps": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "pn2_ball_query": (_i, [_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp]),
    "pn2_ball_query_workspace_bytes": (_i64, [_i, _i, _i]),
    "pn2_ball_query_ws": (_i, [_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp, _vp]),
    "pn2_square_distance": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pn2_three_nn": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pn2_gather_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pn2_gather_rows_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pn2_group": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pn2_group_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "pn2_group_affine_fwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "pn2_group_affine_bwd": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "pn2_three_interp": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp]),
    "pn2_three_interp_bwd": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pn2_copy_cols": (_i, [_vp, _i, _i, _vp, _i, _i, _i64, _i, _vp]),
    "pn2_conv1x1_fwd": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i64, _i, _i, _vp, _vp, _vp]),
    "pn2_group_conv_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "pn2_conv1x1_fwd_pool": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i64, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "pn2_bn_pool_select": (_i, [_vp, _vp, _i64, _i, _vp, _i, _vp, _vp, _vp]),
    "pn2_bn_finalize": (_i, [_vp, _i64, _i, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_bn_relu_max": (_i, [_vp, _i, _vp, _i64, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "pn2_pool_bwd_reduce": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "pn2_pool_bwd_reduce_ld": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "pn2_pool_bwd_reduce_rec": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp]),
    "pn2_relu_bwd_reduce": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i64, _i, _vp, _i, _vp, _vp]),
    "pn2_bn_bwd_coef": (_i, [_vp, _i64, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "pn2_conv1x1_dgrad": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp,
                               _i64, _i, _i, _vp, _vp]),
    "pn2_conv1x1_wgrad": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp,
                               _i64, _i, _i, _vp, _vp]),
    "pn2_conv1x1_wgrad_workspace_bytes": (_i64, [_i64, _i, _i, _i]),
    "pn2_conv1x1_wgrad_ws": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp,
                                  _i64, _i, _i, _vp, _vp, _vp]),
    "pn2_conv1x1_wgrad_cf_scratch_bytes": (_i64, []),
    "pn2_conv1x1_wgrad_cf": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _vp]),
    "pn2_conv1x1_bwd_pair": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i,
                                  _i64, _i, _i, _vp, _vp]),
    "pn2_res_supported": (_i, [_i64, _i, _i]),
    "pn2_bwd_res_supported": (_i, [_i64, _i, _i, _i, _i]),
    "pn2_conv1x1_bwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i,
                             _i64, _i, _i, _vp, _vp]),
    "pn2_conv1x1_bwd_cf_supported": (_i, [_i64, _i, _i, _i]),
    "pn2_conv1x1_bwd_cf_scratch_bytes": (_i64, [_i, _i]),
    "pn2_conv1x1_bwd_cf": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i64, _i, _i, _vp, _vp, _vp]),
    "pn2_conv1x1_bwd_first_supported": (_i, [_i64, _i, _i, _i]),
    "pn2_conv1x1_bwd_first": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _i64, _i, _i, _vp, _vp]),
    "pn2_fused_eval": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp]),
    "pn2_invert_index": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pn2_three_interp_bwd_seg": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pn2_group_affine_bwd_seg": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i,
                                         _vp, _vp, _vp]),
    "pn2_nll_loss_workspace_bytes": (_i64, [_i64]),
    "pn2_nll_loss_fwd": (_i, [_vp, _i, _vp, _vp, _i64, _i, _i64, _vp, _vp, _vp, _vp]),
    "pn2_nll_loss_bwd": (_i, [_vp, _vp, _i64, _i, _i64, _vp, _vp, _vp, _i, _vp]),
    "pn2_cross_entropy_workspace_bytes": (_i64, [_i64]),
    "pn2_cross_entropy_fwd": (_i, [_vp, _i, _i64, _vp, _vp, _i64, _i, _i64, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_cross_entropy_bwd": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _i64, _i, _i64, _d, _i, _vp, _vp, _vp, _vp]),
    "pn2_log_softmax_fwd": (_i, [_vp, _i, _i64, _i, _vp, _i, _vp]),
    "pn2_log_softmax_bwd": (_i, [_vp, _i, _vp, _i, _i64, _i, _vp, _i, _vp]),
    "pn2_adam_step": (_i, [_vp, _vp, _vp, _vp, _i64, _d, _d, _d, _d, _d, _i64, _vp, _vp, _i, _vp]),
    "pn2_sgd_step": (_i, [_vp, _vp, _vp, _i64, _d, _d, _d, _d, _i, _i, _i64, _vp, _vp, _i, _vp]),
    "pn2_prepare_clouds": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "pn2_prepare_shapes": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "pn2_point_transform": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _i, _vp]),
    "pn2_point_transform_workspace_bytes": (_i64, [_i, _i, _i]),
    "pn2_point_transform_bwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "pn2_bn_max": (_i, [_vp, _i, _vp, _i64, _i, _i, _vp, _i, _vp, _vp]),
    "pn2_pool_bwd_reduce_noact": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "pn2_conv1x1_fwd_gbias": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i64, _vp, _i, _i64, _i, _i, _vp, _vp]),
    "pn2_group_colsum_workspace_bytes": (_i64, [_i64, _i64, _i]),
    "pn2_group_colsum": (_i, [_vp, _i, _vp, _i, _vp, _i64, _i64, _i, _vp, _i, _vp, _vp]),
    "pn2_conv1x1_fwd_multi": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i64, _vp, _i, _i64, _i, _vp, _vp]),
    "pn2_conv1x1_wgrad_multi": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i64, _i, _vp]),
    "pn2_conv1x1_dgrad_multi": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i64, _i, _vp]),
    "pn2_bn_bwd_reduce_noact_dense": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i64, _i, _i, _vp, _i, _vp, _vp]),
    "pn2_chamfer_nn_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "pn2_chamfer_nn": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_chamfer_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pn2_seg_confusion": (_i, [_vp, _i, _vp, _i, _i64, _i, _i64, _vp, _i64, _vp, _vp]),
    "pn2_seg_predict": (_i, [_vp, _i, _i64, _i, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "pn2_project_points": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp]),
    "pn2_splat_discs": (_i, [_vp, _i64, _vp, _i, _i, _i, _vp, _vp]),
    "pn2_splat_resolve": (_i, [_vp, _i, _i, _vp, _i64, _vp, _i, _vp, _vp, _vp, _vp]),
    "pn2_depth_splat": (_i, [_vp, _i, _i64, _vp, _vp, _d, _d, _i, _i, _i, _vp, _vp]),
    "pn2_depth_resolve": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "pn2_sample_image": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i64, _i64, _vp, _i, _vp, _vp, _vp]),
    "pn2_hsv_to_rgb": (_i, [_vp, _i, _i64, _i, _vp, _vp]),
    "pn2_scan_filter_workspace_bytes": (_i64, [_i, _i64]),
    "pn2_scan_filter": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_knn": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_knn_vote": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _vp, _i, _vp, _i64, _vp, _vp, _vp]),
    "pn2_local_pca": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_grid_workspace_bytes": (_i64, [_i, _i64]),
    "pn2_grid_build": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_grid_knn": (_i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_icp_workspace_bytes": (_i64, [_i, _i]),
    "pn2_icp_step": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _f, _i, _i, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                          _vp, _vp]),
    "pn2_plane_workspace_bytes": (_i64, [_i, _i, _i]),
    "pn2_plane_ransac": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, ctypes.c_uint64, _vp, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_plane_refit": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_plane_classify": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _i64, _d, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_spfh": (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "pn2_fpfh": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "pn2_feature_nn2": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_match_pairs_workspace_bytes": (_i64, [_i, _i]),
    "pn2_match_pairs": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_corr_workspace_bytes": (_i64, [_i, _i, _i]),
    "pn2_corr_ransac": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, ctypes.c_uint64, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_corr_refit": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _d, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_voxel_grid_workspace_bytes": (_i64, [_i, _i64]),
    "pn2_voxel_grid": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_segment_reduce_workspace_bytes": (_i64, [_i, _i64, _i]),
    "pn2_segment_mean": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "pn2_segment_mean_bwd": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "pn2_segment_mode": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_segment_boxes_workspace_bytes": (_i64, [_i, _i64]),
    "pn2_segment_boxes": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp]),
    "pn2_voxel_components_workspace_bytes": (_i64, [_i, _i64]),
    "pn2_voxel_components": (_i, [_vp, _i, _vp, _vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pn2_panoptic_workspace_bytes": (_i64, [_i, _i64]),
    "pn2_panoptic_count": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i, _vp, _vp, _i, _vp, _i64, _vp, _vp, _vp]),
    "pn2_lovasz_tile_rows": (_i, []),
    "pn2_lovasz_workspace_bytes": (_i64, [_i64, _i, _i]),
    "pn2_lovasz_fwd": (_i, [_vp, _i, _i64, _vp, _i64, _i, _i, _i64, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "pn2_lovasz_bwd": (_i, [_vp, _i, _i64, _vp, _i64, _i, _i, _vp, _vp, _vp]),
}

# The launch entry points: they return a status and take the stream handle as their last (pointer) argument.  Everything else
# is a host-only call (sizes, capability questions, options); pn2_get_option has the same shape and launches nothing.
LAUNCHES = frozenset(name for name, (res, args) in SIGNATURES.items()
                     if res is _i and args and args[-1] is _vp and name != "pn2_get_option")
HOST_ONLY = frozenset(SIGNATURES) - LAUNCHES

ABI_VERSION = 15
PN2_EUNSUPPORTED = -3            # include/pn2.h
PN2_OK_SPLIT = 1                 # pn2_conv1x1_bwd_pair: done as two launches
DWX_REPLICAS = 32        # PN2_DWX_REPLICAS of include/pn2.h
SCAN_TILE = 1024         # PN2_SCAN_TILE of include/pn2.h: rows per workgroup of pn2_scan_filter
SCAN_ERR_CLASS, SCAN_ERR_ROWS = 1, 2     # PN2_SCAN_ERR_* of include/pn2.h
CHANNELS_RGB, CHANNELS_BGR = 0, 1         # PN2_CHANNELS_* of include/pn2.h: pn2_sample_image / pn2_hsv_to_rgb
IMAGE_RGB, IMAGE_HSV = 0, 1               # PN2_IMAGE_* of include/pn2.h: pn2_sample_image's mode
IMAGE_ERR_ROWS = 1                        # PN2_IMAGE_ERR_ROWS: a cloud's rows left the buffers and were skipped
KNN_MAX_K = 32           # pn2_knn / pn2_knn_vote: larger K is PN2_EUNSUPPORTED
KNN_ERR_LABEL, KNN_ERR_DST = 1, 2        # the err bits of pn2_knn_vote
GRID_ERR_CAND, GRID_ERR_QUERY = 1, 2     # PN2_GRID_ERR_* of include/pn2.h: the err bits of pn2_grid_build / pn2_grid_knn
GRID_VISIT_SORTED = 1    # PN2_GRID_VISIT_SORTED: pn2_grid_knn's flag, a self-search serves the records in cell order
ICP_POINT, ICP_PLANE = 0, 1              # PN2_ICP_* of include/pn2.h: pn2_icp_step's metric
ICP_EVAL_ONLY = 1        # PN2_ICP_EVAL_ONLY: pn2_icp_step's flag, sums / count / corr only
ICP_CONVERGED, ICP_SINGULAR = 1, 2       # its status bits
ICP_ERR_QUERY, ICP_ERR_SINGULAR, ICP_ERR_NONFINITE = 1, 2, 4         # its err bits
PLANE_NONE, PLANE_DEGENERATE, PLANE_SMALL = 1, 2, 4      # PN2_PLANE_* of include/pn2.h: the status bits of the plane entry points
PLANE_ERR_NONFINITE, PLANE_ERR_NONE = 1, 2               # their err bits
FPFH_ERR_EMPTY, FPFH_ERR_NONFINITE = 1, 2   # PN2_FPFH_ERR_* of include/pn2.h: the err bits of pn2_spfh / pn2_fpfh
MATCH_MAX_D = 64         # PN2_MATCH_MAX_D: the widest feature of pn2_feature_nn2
CORR_NONE, CORR_DEGENERATE = 1, 2        # PN2_CORR_* of include/pn2.h: the status bits of pn2_corr_ransac / pn2_corr_refit
CORR_ERR_PAIR, CORR_ERR_NONFINITE, CORR_ERR_NONE = 1, 2, 4           # their err bits
CORR_EVAL_ONLY = 1       # PN2_CORR_EVAL_ONLY: pn2_corr_refit's flag, sums / inliers / rmse only
CORR_SUMS = 17           # PN2_CORR_SUMS: the words of pn2_corr_refit's sums
PCA_ERR_FEW, PCA_ERR_NONFINITE = 1, 2     # PN2_PCA_ERR_* of include/pn2.h: the err bits of pn2_local_pca
VOXEL_TILE = 1024        # PN2_VOXEL_TILE of include/pn2.h: rows per workgroup of pn2_voxel_grid's compaction passes
VOXEL_MAX_ROWS = 1 << 29                 # PN2_VOXEL_MAX_ROWS: the largest max_rows of pn2_voxel_grid
VOXEL_ERR_RANGE, VOXEL_ERR_ROWS = 1, 2   # PN2_VOXEL_ERR_* of include/pn2.h
SEGMENT_MAX_COLS = 16    # PN2_SEGMENT_MAX_COLS: the widest pn2_segment_mean / pn2_segment_mean_bwd call
SEGMENT_ERR_RANGE, SEGMENT_ERR_NONFINITE = 4, 8      # PN2_SEGMENT_ERR_* (disjoint from VOXEL_ERR_*: they share VoxelGrid.error_flag)
CLUSTER_ERR_INDEX, CLUSTER_ERR_CELL, CLUSTER_ERR_CAP, CLUSTER_ERR_ROWS = 16, 32, 64, 128     # PN2_CLUSTER_ERR_* (disjoint from both)
PANOPTIC_ERR_CLASS, PANOPTIC_ERR_ROWS = 256, 512     # PN2_PANOPTIC_ERR_* (disjoint from all of the above)
BOX_ERR_RANGE, BOX_ERR_NONFINITE = 1024, 2048        # PN2_BOX_ERR_* (disjoint from all of the above: a downsample -> cluster -> boxes chain shares one word)
BOX_MAX_ANGLES = 256     # PN2_BOX_MAX_ANGLES: the longest angle table of pn2_segment_boxes
BOX_SPLIT_ROWS = 4096    # pn2_segment_boxes' split_rows = 0: the rows from which a workgroup sweeps a segment instead of a wave


class BnLazy(ctypes.Structure):
    """pn2_bn_lazy of include/pn2.h: statistics -> affine block inside the first launch that reads the block."""
    _fields_ = [("stats", _vp), ("gamma", _vp), ("beta", _vp), ("eps", _f), ("momentum", _f), ("running_mean", _vp),
                ("running_var", _vp), ("num_batches_tracked", _vp), ("affine", _vp), ("count", _i64), ("C", _i)]


class BnCoefLazy(ctypes.Structure):
    """pn2_bn_coef_lazy of include/pn2.h: reductions -> backward coefficients inside the first launch that reads them."""
    _fields_ = [("red", _vp), ("gamma", _vp), ("affine", _vp), ("coef", _vp), ("dgamma", _vp), ("dbeta", _vp),
                ("accumulate", _i), ("count", _i64), ("C", _i)]


class EvalLayer(ctypes.Structure):
    """pn2_eval_layer of include/pn2.h."""
    _fields_ = [("W", _vp), ("bias", _vp), ("K", _i), ("N", _i), ("ldw", _i)]


class Src(ctypes.Structure):
    """pn2_src of include/pn2.h: one per-point source of a K-concatenated operand."""
    _fields_ = [("X", _vp), ("ldx", _i), ("K", _i), ("affine", _vp), ("relu", _i)]


def src_table(entries):
    """[(X ptr, ldx, K, affine ptr or None, relu)] -> a ctypes pn2_src[n] (pass it as the table pointer)."""
    return (Src * len(entries))(*[Src(x, ldx, k, aff, relu) for x, ldx, k, aff, relu in entries])


class Pn2Error(RuntimeError):
    pass


def build(force=False):
    """Compile libpn2_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return LIB_PATH


_lib = None
_raw = None
_profile = None          # None, or a list receiving (name, args, start_event, end_event) per call


class _Timed:
    """Proxy handed out while a call profile is active: brackets every launch with HIP events recorded on
    the stream the kernel is launched on (the handle passed as the last argument of every launch entry point)."""

    def __getattr__(self, name):
        fn = getattr(_raw, name)
        if name not in LAUNCHES:
            return fn

        def timed(*args):
            import torch
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h = args[-1]
            s = torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream()
            _raw.pn2_clear_last_kernel()
            a.record(s)
            rc = fn(*args)
            b.record(s)
            if rc != PN2_EUNSUPPORTED:         # (a refused shape launched nothing: the caller takes its other route)
                # (pn2_conv1x1_bwd_pair that ran as two launches is booked under a name of its own: bench.py splits it)
                kern = _raw.pn2_last_kernel()      # the GEMM launchers say which template instantiation they enqueued (or None)
                _profile.append((name + "_split" if (name == "pn2_conv1x1_bwd_pair" and rc == PN2_OK_SPLIT) else name, args, a, b,
                                 kern.decode() if kern else None))
            return rc
        return timed


class call_profile:
    """``with call_profile() as calls:`` -> list of (entry point, args, start, end, kernel name or None) for every C-ABI call made
    inside; ``start.elapsed_time(end)`` after a synchronize gives that launch's device time in ms."""

    def __enter__(self):
        global _lib, _profile
        load()
        _profile = []
        _lib = _Timed()
        return _profile

    def __exit__(self, *exc):
        global _lib, _profile
        _lib = _raw
        _profile = None
        return False


def load():
    """Load the library and bind every symbol of SIGNATURES; raises if anything is missing."""
    global _lib, _raw
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Pn2Error("libpn2_hip.so not found at %s -- build it with `python -c \"import __graft_entry__ as g; "
                       "g.build()\"` (hipcc, gfx950). There is no fallback path." % LIB_PATH)
    # torch first: its ROCm wheel carries a HIP runtime of its own under a file name (libamdhip64.so) that is not the SONAME this
    # library asks for (libamdhip64.so.7).  Loaded after torch, the library binds to the runtime torch already mapped; loaded
    # before it, the process ends up with TWO runtimes, and every launch on one of torch's streams fails with PN2_ELAUNCH.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.pn2_version() != ABI_VERSION:
        raise Pn2Error("libpn2_hip.so ABI version %d, expected %d -- rebuild it" % (lib.pn2_version(), ABI_VERSION))
    forward_env_options(lib)         # (before the library is published: a malformed PN2_<OPTION> raises on EVERY load, not only the first)
    _lib = _raw = lib
    return lib


def options(lib=None):
    """{name: value} of every library option (pn2_option_name / pn2_get_option)."""
    lib = lib or load()
    out, i = {}, 0
    while True:
        name = lib.pn2_option_name(i)
        if name is None:
            return out
        v = ctypes.c_int(0)
        if lib.pn2_get_option(name, ctypes.addressof(v)) == 0:
            out[name.decode()] = v.value
        i += 1


_option_hooks = []


def on_option_change(hook):
    """Register ``hook()``, called after every successful ``set_option``: Python-side state that was derived from what the
    library answered under the old options (which route a shape takes) is dropped there."""
    _option_hooks.append(hook)
    return hook


def set_option(name, value):
    """pn2_set_option; raises on an unknown name."""
    check(load().pn2_set_option(name.encode(), int(value)), "pn2_set_option(%s)" % name)
    for hook in _option_hooks:
        hook()


def forward_env_options(lib):
    """The library itself never reads the environment (include/pn2.h, options): A/B runs set PN2_<OPTION>=<int> in the
    environment of THIS binding, which hands them to pn2_set_option once at load time."""
    for name in options(lib):
        v = os.environ.get(name)
        if v is not None:
            try:
                value = int(v)
            except ValueError:
                raise Pn2Error("%s=%r is not an integer" % (name, v))
            rc = lib.pn2_set_option(name.encode(), value)
            if rc != 0:
                raise Pn2Error("pn2_set_option(%s, %d) failed: %d" % (name, value, rc))


def check(rc, what):
    if rc != 0:
        raise Pn2Error("%s failed: %s (%d)" % (what, load().pn2_error_string(rc).decode(), rc))


def workspace_bytes(entry, args, error, message):
    """``entry(*args)`` for a ``pn2_*_workspace_bytes`` entry point (host-only calls); a refused shape raises ``error(message)``."""
    n = int(getattr(load(), entry)(*args))
    if n < 0:
        raise error(message)
    return n


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream

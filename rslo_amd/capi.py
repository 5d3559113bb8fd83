"""ctypes binding of librslo_hip.so (include/rslo_hip.h) for torch tensors on a ROCm device.

This is the only place where Python meets the C ABI.  Tensors are passed as raw device
pointers plus sizes; work is enqueued on torch's current HIP stream.  There is NO fallback:
if the library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSLO_HIP_LIB") or os.path.join(_HERE, "librslo_hip.so")   # override: kernel experiments only
_lib = None

_I3 = C.c_int32 * 3
_F3 = C.c_float * 3
_F6 = C.c_float * 6

# name -> (restype, argtypes); checked against include/rslo_hip.h by tests/test_cabi.py
_vp, _i, _i64, _sz, _f = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float
SIGNATURES = {
    "rslo_abi_version": (C.c_int, []),
    "rslo_last_error": (C.c_char_p, []),
    "rslo_voxelize_ws_bytes": (_sz, [_i64]),
    "rslo_voxelize": (C.c_int, [_vp, _i64, _i, _vp, _vp, _vp, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "rslo_vfe_mean": (C.c_int, [_vp, _vp, _i64, _i, _i, _vp, _vp]),
    "rslo_hash_capacity": (_i64, [_i64]),
    "rslo_hash_build": (C.c_int, [_vp, _i64, _i, _vp, _vp, _vp, _i64, _vp]),
    "rslo_rulebook_subm": (C.c_int, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "rslo_conv_bitmap_words": (_i64, [_i, _vp]),
    "rslo_scan_ws_bytes": (_sz, [_i64]),
    "rslo_conv_out_count": (C.c_int, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _sz, _vp, _vp]),
    "rslo_conv_out_coords": (C.c_int, [_vp, _vp, _i64, _i, _vp, _vp, _i64, _vp]),
    "rslo_rulebook_conv": (C.c_int, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "rslo_rulebook_conv_T": (C.c_int, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "rslo_spconv_fwd": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _f, _vp, _vp, _vp]),
    "rslo_spconv_dgrad": (C.c_int, [_vp, _i, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp]),
    "rslo_weight_transpose": (C.c_int, [_vp, _i, _i, _i, _vp, _vp]),
    "rslo_weight_split_bytes": (_sz, [_i, _i, _i]),
    "rslo_weight_split": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "rslo_weight_split_many": (C.c_int, [_vp, _i, _i64, _vp]),
    "rslo_spconv_fwd_split": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, C.c_float, _vp, _vp, _vp]),
    "rslo_peer_create_host": (C.c_int, [C.c_char_p, _i, _i, _i, C.POINTER(C.c_void_p)]),
    "rslo_peer_host_unlink": (C.c_int, [_vp]),
    "rslo_peer_ipc_handle_bytes": (C.c_int, []),
    "rslo_peer_create_device_begin": (C.c_int, [_i, _i, _i, C.POINTER(C.c_void_p), _vp]),
    "rslo_peer_create_device_finish": (C.c_int, [_vp, _vp]),
    "rslo_peer_set_timeout_ms": (C.c_int, [_vp, _i]),
    "rslo_peer_allreduce_f64": (C.c_int, [_vp, _vp, _i, _vp]),
    "rslo_peer_status": (C.c_ulonglong, [_vp, C.POINTER(C.c_int)]),
    "rslo_peer_destroy": (C.c_int, [_vp]),
    "rslo_tuning_set": (C.c_int, [C.c_char_p, _i]),
    "rslo_tuning_get": (C.c_int, [C.c_char_p, _vp]),
    "rslo_tuning_name": (C.c_char_p, [_i]),
    "rslo_weight_to_bf16": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "rslo_spconv_fwd_bf16": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, C.c_float, _vp, _vp]),
    "rslo_spconv_wgrad_ws_bytes": (_sz, [_i64, _i, _i, _i]),
    "rslo_spconv_wgrad": (C.c_int, [_vp, _i, _vp, _i, _vp, _i64, _i, _vp, _sz, _vp, _vp, _vp]),
    "rslo_rulebook_row_order": (C.c_int, [_vp, _i64, _i, _i, _vp, _vp]),
    "rslo_leaky_bwd_colsum_bf16_blocks": (_i64, [_i64, _i]),
    "rslo_leaky_bwd_colsum_bf16": (C.c_int, [_vp, _vp, _i64, _i, C.c_float, _vp, _vp, _vp]),
    "rslo_spconv_wgrad_pairs_bf16": (C.c_int, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i64, _i, _vp, _sz, _vp, _vp, _vp, _i,
                                               _vp]),
    "rslo_rulebook_pairs_ws_bytes": (_sz, [_i64, _i]),
    "rslo_rulebook_pairs": (C.c_int, [_vp, _i64, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
    "rslo_spconv_wgrad_pairs_ws_bytes": (_sz, [_i64, _i, _i, _i]),
    "rslo_spconv_wgrad_pairs": (C.c_int, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i64, _i, _vp, _sz, _vp, _vp, _vp, _i, _vp]),
    "rslo_leaky_bwd_colsum_blocks": (_i64, [_i64, _i]),
    "rslo_leaky_bwd_colsum": (C.c_int, [_vp, _vp, _i64, _i, C.c_float, _vp, _vp, _vp]),
    "rslo_leaky_bwd": (C.c_int, [_vp, _vp, _i64, _f, _vp, _vp]),
    "rslo_segbn_ws_bytes": (_sz, [_i, _i64, _i]),
    "rslo_segbn_fwd": (C.c_int, [_vp, _i, _vp, _i, _i64, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _sz, _vp, _vp, _vp, _vp]),
    "rslo_segbn_bwd": (C.c_int, [_vp, _vp, _vp, _i, _vp, _i, _i64, _vp, _vp, _vp, _f, _vp, _sz, _vp, _vp, _vp, _vp]),
    "rslo_dense_scatter": (C.c_int, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "rslo_dense_gather": (C.c_int, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "rslo_dense_scatter_frames": (C.c_int, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp]),
    "rslo_dense_gather_frames": (C.c_int, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp]),
    "rslo_bev_channel_sums": (C.c_int, [_vp, _i, _i, _i, _i64, _vp, _vp]),
    "rslo_chamfer_ws_bytes": (_sz, [_i, _i, _i]),
    "rslo_chamfer_nn": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "rslo_chamfer_nn_ragged": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "rslo_chamfer_brute_nn": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "rslo_chamfer_grid_ws_bytes": (_sz, [_i, _i, _i]),
    "rslo_chamfer_grid_nn": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "rslo_chamfer_grad": (C.c_int, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "rslo_cov_residual_ws_bytes": (_sz, [_i, _i]),
    "rslo_cov_residual_fwd": (C.c_int, [_vp] * 8 + [_i, _i, _i, _f, _vp, _sz, _vp, _vp, _vp]),
    "rslo_cov_residual_bwd": (C.c_int, [_vp] * 10 + [_i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "rslo_cov_residual_bwd_ws_bytes": (_sz, [_i, _i, _i]),
    "rslo_icp_ws_bytes": (_sz, [_i, _i]),
    "rslo_icp_step": (C.c_int, [_vp] * 6 + [_i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "rslo_icp_step_first": (C.c_int, [_vp] * 6 + [_i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "rslo_transform_points": (C.c_int, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "rslo_transform_rows": (C.c_int, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "rslo_transform_rows_bwd_ws_bytes": (_sz, [_i, _i]),
    "rslo_transform_rows_bwd": (C.c_int, [_vp, _i, _vp, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
    "rslo_bn2d_ws_bytes": (_sz, [_i, _i, _i]),
    "rslo_bn2d_stats": (C.c_int, [_vp, _i, _i, _i, _vp, _sz, _vp, _vp, _vp]),
    "rslo_bn2d_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp,
                                  _vp, _vp, _vp]),
    "rslo_bn2d_bwd_reduce": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, _i, _vp, _sz, _vp, _vp, _vp, _vp,
                                       _vp]),
    "rslo_bn2d_bwd_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _i, _i, _i, C.c_float, _i, _vp,
                                      _vp, _vp]),
    "rslo_bn2d_fwd_local": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _sz, _vp]),
    "rslo_bn2d_bwd_local": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, _i, _vp, _vp, _vp, _vp, _vp,
                                      _sz, _vp]),
    "rslo_roi_threshold": (C.c_int, [_vp, _i, _i, _vp, C.c_double, _vp, _vp]),
    "rslo_vote_ws_bytes": (_sz, [_i, _i, _i]),
    "rslo_vote_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "rslo_vote_bwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rslo_conv2d_wgrad_supported": (C.c_int, [_i, _i, _i, _i, _i]),
    "rslo_conv2d_wgrad_ws_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "rslo_conv1x1s2_wgrad_supported": (C.c_int, [_i, _i, _i, _i]),
    "rslo_conv1x1s2_wgrad_ws_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "rslo_conv1x1s2_wgrad": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "rslo_conv2d_wgrad": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "rslo_conv2d_fwd_supported": (C.c_int, [_i, _i, _i, _i]),
    "rslo_conv2d_wsplit_bytes": (_sz, [_i, _i]),
    "rslo_conv2d_wsplit": (C.c_int, [_vp, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_wsplit_k": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_s2_supported": (C.c_int, [_i, _i, _i]),
    "rslo_conv2d_fwd_s2": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_dgrad_s2": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_wsplit_many": (C.c_int, [_vp, _i, _i64, _vp]),
    "rslo_conv2d_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_fwd_bf16": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_cat_upsample_fwd": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_cat_upsample_bwd": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "rslo_bev_channel_sums_masks": (C.c_int, [_vp, _i, _i, _i, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "rslo_pose_tail_fwd": (C.c_int, [_vp, _i, _vp, _vp, _vp]),
    "rslo_pose_tail_bwd": (C.c_int, [_vp, _vp, _vp, _i, _vp, _vp]),
    "rslo_bev_display_ws_bytes": (_sz, [_i]),
    "rslo_bev_display": (C.c_int, [_vp, _i, _i, _i, C.c_int64, _vp, _vp, _vp, _sz, _vp]),
    "rslo_conv2d_dgrad_s2_add": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_fwd_add": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_fwd_add_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_wgrad_bf16": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "rslo_conv1x1_supported": (C.c_int, [_i, _i]),
    "rslo_conv1x1_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv1x1_dgrad": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv1x1_wgrad_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "rslo_conv1x1_wgrad": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "rslo_quat_to_rot": (C.c_int, [_vp, _i, _vp, _vp]),
    "rslo_quat_to_rot_bwd": (C.c_int, [_vp, _vp, _i, _vp, _vp]),
    "rslo_pose_targets": (C.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "rslo_pose_targets_tq": (C.c_int, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "rslo_pair_rows_fwd": (C.c_int, [_vp, _i64, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "rslo_pad_rows_fwd": (C.c_int, [_vp, _i64, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "rslo_pad_rows_bwd": (C.c_int, [_vp, _i64, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "rslo_pyramid_l2_ws_bytes": (_sz, [_vp, _i, _i]),
    "rslo_pyramid_l2_fwd": (C.c_int, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "rslo_pyramid_l2_bwd": (C.c_int, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "rslo_plan_encoder_layout": (C.c_int, [_vp, _i, _vp, _vp]),
    "rslo_plan_encoder_pad_tails": (C.c_int, [_vp, _vp, _vp, _vp]),
    "rslo_plan_encoder": (C.c_int, [_vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
    "rslo_tq_normalize_fwd": (C.c_int, [_vp, _i, _i64, _vp, _vp]),
    "rslo_tq_normalize_bwd": (C.c_int, [_vp, _vp, _i, _i64, _vp, _vp]),
    "rslo_conf_softmax_fwd": (C.c_int, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "rslo_conf_softmax_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "rslo_head_masks_fwd": (C.c_int, [_vp, _vp]),
    "rslo_head_masks_bwd": (C.c_int, [_vp, _vp]),
    "rslo_loss_tail_fwd": (C.c_int, [_vp, _vp, _vp]),
    "rslo_loss_tail_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rslo_peer_wait_samples": (C.c_int, [_vp, _vp, _i]),
    "rslo_bn1d_eval_act": (C.c_int, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp]),
    "rslo_wgrad_reduce_defer": (C.c_int, [_vp, _i, _vp]),
    "rslo_wgrad_reduce_many": (C.c_int, [_vp, _i, _vp]),
    "rslo_peer_capture_begin": (C.c_int, [_vp]),
    "rslo_peer_capture_end": (C.c_int, [_vp, _vp]),
    "rslo_peer_replay_prepare": (C.c_int, [_vp, _i, _vp]),
    "rslo_bn2d_peer_supported": (C.c_int, [_i, _i, _i]),
    "rslo_bn2d_fwd_peer": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp]),
    "rslo_bn2d_bwd_peer": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, _i, _vp, _vp, _vp, _vp,
                                     _vp]),
    "rslo_opl_bytes": (_sz, [_i, _i, _i, _i]),
    "rslo_opl_from_nchw": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "rslo_conv2d_fwd_p_supported": (C.c_int, [_i, _i, _i, _i]),
    "rslo_conv2d_fwd_p": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "rslo_opt_clip_grad_norm": (C.c_int, [_vp, _vp, _i, _f, _vp, _vp, _vp]),
    "rslo_opt_adam_step": (C.c_int, [_vp, _vp, _i, _vp, _f, _vp]),
    "rslo_conv2d_fwd_bn": (C.c_int, [_vp] * 6 + [_i, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "rslo_conv2d_fwd_s2_bn": (C.c_int, [_vp] * 6 + [_i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "rslo_bn_fold_many": (C.c_int, [_vp, _i, _i, _vp]),
    "rslo_pose_chain": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "rslo_normals_ws_bytes": (_sz, [_i]),
    "rslo_estimate_normals": (C.c_int, [_vp, _i, _i, _f, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "rslo_voxel_downsample_ws_bytes": (_sz, [_i]),
    "rslo_voxel_downsample": (C.c_int, [_vp, _i, _vp, _i, _i, C.c_double, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "rslo_map_bytes": (_sz, [_i64]),
    "rslo_map_reset": (C.c_int, [_vp, _sz, _i64, C.c_double, C.c_double, C.c_double, _vp]),
    "rslo_map_insert_ws_bytes": (_sz, [_i]),
    "rslo_map_insert": (C.c_int, [_vp, _sz, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "rslo_map_lookup": (C.c_int, [_vp, _sz, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "rslo_map_export": (C.c_int, [_vp, _sz, _i, _vp, C.c_double, _vp, _vp, _vp, _i64, _vp, _vp]),
    "rslo_map_insert_frames": (C.c_int, [_vp, _sz, _vp, _sz, _i64, _i, _vp, _i, _vp]),
    "rslo_map_prune_ws_bytes": (_sz, [_i64]),
    "rslo_map_prune": (C.c_int, [_vp, _sz, _vp, C.c_double, _i, _i, _vp, _sz, _vp]),
    "rslo_range_image": (C.c_int, [_vp, _i, _i, _i, _i, C.c_double, C.c_double, _vp, _vp]),
    "rslo_map_carve_ws_bytes": (_sz, [_i64]),
    "rslo_map_carve": (C.c_int, [_vp, _sz, _vp, _i, _i, C.c_double, C.c_double, _vp, _i, _i, C.c_double, C.c_double,
                                 C.c_double, _i, _vp, _sz, _vp]),
    "rslo_map_params": (C.c_int, [_vp, _sz, _vp, _vp]),
    "rslo_map_nearest": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _vp, C.c_double, _i, _vp, _vp, _vp, _vp]),
    "rslo_map_register_ws_bytes": (_sz, [_i]),
    "rslo_map_normal_eq": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _i, _vp, _i, C.c_double, _i, _vp, _vp, _sz, _vp]),
    "rslo_map_register": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _i, _vp, _i, _i, C.c_double, _i, C.c_double, _i,
                                    C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "rslo_map_normal_eq_w": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _i, _vp, _i, C.c_double, _i, C.c_double, _vp, _vp,
                                       _sz, _vp]),
    "rslo_map_register_w": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _i, _vp, _i, _i, C.c_double, _i, C.c_double, _i,
                                      C.c_double, C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "rslo_map_register_sched": (C.c_int, [_vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i, _i, C.c_double, _i,
                                          C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "rslo_place_bytes": (_sz, [_i64, _i, _i]),
    "rslo_place_reset": (C.c_int, [_vp, _sz, _i64, _i, _i, _vp]),
    "rslo_place_describe": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    "rslo_place_add": (C.c_int, [_vp, _sz, _i64, _i, _i, _vp, _vp, _vp, _vp]),
    "rslo_place_query_ws_bytes": (_sz, [_i64]),
    "rslo_place_query": (C.c_int, [_vp, _sz, _i64, _i, _i, _vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _sz, _vp]),
    "rslo_posegraph_ws_bytes": (_sz, [_i, _i]),
    "rslo_posegraph_optimize": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i] + [C.c_double] * 5 +
                                [_vp, _vp, _sz, _vp]),
    "rslo_posegraph_cost": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.c_double, _vp, _vp, _sz, _vp]),
    "rslo_posegraph_linearize": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.c_double, _vp, _vp, _vp, _vp, _sz,
                                           _vp]),
    "rslo_posegraph_matvec": (C.c_int, [_vp, _vp, _i, _i, C.c_double, _vp, _sz, _vp]),
    "rslo_posegraph_chain_solve": (C.c_int, [_vp, _vp, _i, _i, _vp, _sz, _vp]),
    "rslo_pose_between": (C.c_int, [_vp, _vp, _i, _vp, _vp]),
    "rslo_keyframe_bytes": (_sz, [_i64, _i]),
    "rslo_keyframe_reset": (C.c_int, [_vp, _sz, _i64, _i, _vp]),
    "rslo_keyframe_prepare_ws_bytes": (_sz, [_i]),
    "rslo_keyframe_prepare": (C.c_int, [_vp, _i, _i, _i, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _sz, _vp]),
    "rslo_keyframe_add": (C.c_int, [_vp, _sz, _i64, _i, _vp, _vp, _vp]),
    "rslo_loop_verify": (C.c_int, [_vp, _sz, _i64, _i, _vp, _vp, _vp, _i, _vp, _vp, _i] + [C.c_double] * 4 +
                         [_i, C.c_double, _vp, _vp, _vp, _vp]),
    "rslo_loop_edges_reset": (C.c_int, [_vp, _vp, _vp, _vp, _i, _vp]),
    "rslo_loop_emit": (C.c_int, [_vp, _i, _vp, _sz, _i64, _i, _vp, _vp, _vp, _vp, _i, C.c_double, C.c_double, _vp]),
    "rslo_surfel_bytes": (_sz, [_i64]),
    "rslo_surfel_reset": (C.c_int, [_vp, _sz, _i64, C.c_double, C.c_double, C.c_double, _i, C.c_double, C.c_double, _vp]),
    "rslo_surfel_insert_ws_bytes": (_sz, [_i]),
    "rslo_surfel_insert": (C.c_int, [_vp, _sz, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "rslo_surfel_insert_frames": (C.c_int, [_vp, _sz, _vp, _sz, _i64, _i, _vp, _i, _vp]),
    "rslo_surfel_export": (C.c_int, [_vp, _sz, _i, _vp, C.c_double, _vp, _vp, _vp, _i64, _vp, _vp]),
    "rslo_surfel_nearest": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    "rslo_surfel_prune_ws_bytes": (_sz, [_i64]),
    "rslo_surfel_prune": (C.c_int, [_vp, _sz, _vp, C.c_double, C.c_double, _i, _vp, _sz, _vp]),
    "rslo_surfel_register_ws_bytes": (_sz, [_i]),
    "rslo_surfel_normal_eq": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _vp, C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "rslo_surfel_register": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _vp, _i, C.c_double, C.c_double, _i, C.c_double,
                                       C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "rslo_surfel_nearest_d": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _vp, C.c_double, _i, C.c_double, C.c_double, _vp,
                                        _vp, _vp, _vp, _vp]),
    "rslo_surfel_normal_eq_d": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _vp, C.c_double, _i, C.c_double, C.c_double,
                                          C.c_double, _vp, _vp, _sz, _vp]),
    "rslo_surfel_register_d": (C.c_int, [_vp, _sz, C.c_double, _vp, _i, _i, _vp, _i, C.c_double, C.c_double, _i, C.c_double,
                                         C.c_double, C.c_double, _i, C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "rslo_deskew": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i, C.c_double, _vp, _i, _vp,
                              _vp]),
}


class RsloHipError(RuntimeError):
    pass


def lib():
    """Load librslo_hip.so; raise (never fall back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RsloHipError(
                "librslo_hip.so not found at %s -- build it with `python -m rslo_amd.build` "
                "(there is no CPU fallback for the RSLO hot path)" % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib if _proxy is None else _proxy


_proxy = None


def probe_streams(on, points_only=None):
    """bench.py: while on, lib() hands out streamprobe.LibProxy -- every launching entry point is bracketed by HIP events on
    its stream (rslo_amd/streamprobe.py).  Off (the default, and during every timed step): the plain library."""
    global _proxy
    from rslo_amd import streamprobe
    if on:
        _proxy = streamprobe.LibProxy(lib() if _proxy is None else _proxy._lib, SIGNATURES, points_only)
        streamprobe.start()
    else:
        streamprobe.stop()
        _proxy = None


def tuning_set(name, value):
    """rslo_tuning_set: an explicit switch of the launch code (the library reads no environment variable)."""
    _chk(lib().rslo_tuning_set(name.encode(), int(value)), "rslo_tuning_set")


def tuning_get(name):
    v = C.c_int(0)
    _chk(lib().rslo_tuning_get(name.encode(), C.byref(v)), "rslo_tuning_get")
    return v.value


class tuning:
    """with capi.tuning(conv2d_fwd_kc=2, ...): switches set for the block and restored afterwards (tests, A/B scripts)."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = tuning_get(k)
            tuning_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            tuning_set(k, v)
        return False


def _chk(rc, name):
    if rc != 0:
        raise RsloHipError("%s failed (%d): %s" % (name, rc, lib().rslo_last_error().decode()))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    # raw hipStream_t of torch's current stream: two C calls (torch.cuda.current_device() re-checks the lazy initialisation in
    # Python on every call: 1.5 us x ~270 launches per step); falls back to the public API
    # (a plain int is what a c_void_p parameter wants: no wrapper object per launch)
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t, dtype=None, name="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise RsloHipError("%s must live on the GPU (the RSLO hot path has no CPU fallback)" % name)
    if dtype is not None and t.dtype != dtype:
        raise RsloHipError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise RsloHipError("%s must be contiguous" % name)
    return t.data_ptr()


def _dp(t):
    """data pointer of an optional tensor the caller already knows to be a contiguous CUDA tensor of the right type"""
    return None if t is None else t.data_ptr()


def _i3(x):
    return _I3(*[int(v) for v in x])


def _ws(nbytes, device):
    return torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)


# --------------------------------------------------------------------------------------
# deferred weight-gradient reduces (csrc/wgrad_reduce.hip)
# --------------------------------------------------------------------------------------
class RsloWgradReduce(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_blocks", C.c_int32), ("ws", C.c_void_p), ("dW", C.c_void_p), ("aux", C.c_void_p),
                ("dbias", C.c_void_p), ("koff", C.c_void_p), ("p", C.c_int32 * 8)]


import threading as _threading
_tls = _threading.local()      # .sink: the ReduceSink installed by THIS thread (the C library's sink is per thread as well)


class ReduceSink:
    """Collects the second stage (partials -> gradient) of the weight-gradient entry points called inside `with
    sink.collect():` instead of launching it per layer; `flush()` runs everything collected as ONE launch on the current
    stream (rslo_wgrad_reduce_many: same block bodies, same bits).  The workspaces / bias partials the descriptors point to are
    kept referenced until the flush.  The caller (rslo_amd/streams.py) flushes before anything can read a gradient."""
    CAP = 256

    def __init__(self):
        self.arr = (RsloWgradReduce * self.CAP)()
        self.count = C.c_int(0)
        self.keep = []

    class _Collect:
        def __init__(self, sink):
            self.sink = sink

        def __enter__(self):
            self.prev = getattr(_tls, "sink", None)
            _tls.sink = self.sink
            _chk(lib().rslo_wgrad_reduce_defer(self.sink.arr, ReduceSink.CAP, C.byref(self.sink.count)), "rslo_wgrad_reduce_defer")
            return self.sink

        def __exit__(self, *exc):
            _tls.sink = self.prev
            if self.prev is not None:
                lib().rslo_wgrad_reduce_defer(self.prev.arr, ReduceSink.CAP, C.byref(self.prev.count))
            else:
                lib().rslo_wgrad_reduce_defer(None, 0, None)
            return False

    def collect(self):
        return ReduceSink._Collect(self)

    def pending(self):
        return self.count.value

    def flush(self):
        n = self.count.value
        if n:
            rc = lib().rslo_wgrad_reduce_many(self.arr, n, _stream())
            self.count.value = 0
            self.keep.clear()
            _chk(rc, "rslo_wgrad_reduce_many")
        else:
            self.keep.clear()


def _keep_for_reduce(*tensors):
    """Inside ReduceSink.collect(): the buffers a deferred reduce will read stay referenced until its flush."""
    sink = getattr(_tls, "sink", None)
    if sink is not None:
        sink.keep.extend(t for t in tensors if t is not None)


# --------------------------------------------------------------------------------------
# voxelization / VFE
# --------------------------------------------------------------------------------------
def voxelize(points, pc_range, voxel_size, grid_xyz, max_points, max_voxels):
    """points [P,F] f32 cuda -> (voxels [max_voxels,T,F], coords [max_voxels,3] zyx, num [max_voxels],
    d_nvox [1] int32 on device).  Rows >= nvox are zero; the caller slices after reading nvox."""
    P, F = points.shape
    dev = points.device
    # one block, laid out voxels | num | coords | nvox: the library zero-fills it with a single memset
    nv, nn, nc = max_voxels * max_points * F, max_voxels, max_voxels * 3
    block = torch.empty((nv + nn + nc + 4,), dtype=torch.int32, device=dev)
    voxels = block[:nv].view(torch.float32).view(max_voxels, max_points, F)
    num = block[nv:nv + nn]
    coords = block[nv + nn:nv + nn + nc].view(max_voxels, 3)
    nvox = block[nv + nn + nc:nv + nn + nc + 1]
    wsb = lib().rslo_voxelize_ws_bytes(P)
    ws = _ws(wsb, dev)
    r = _F6(*[float(v) for v in pc_range])
    v = _F3(*[float(x) for x in voxel_size])
    g = _i3(grid_xyz)
    _chk(lib().rslo_voxelize(_ptr(points, torch.float32, "points"), P, F, r, v, g, int(max_points),
                             int(max_voxels), _ptr(ws), wsb, _ptr(voxels), _ptr(coords), _ptr(num),
                             _ptr(nvox), _stream()), "rslo_voxelize")
    return voxels, coords, num, nvox


def vfe_mean(voxels, num_points):
    M, T, F = voxels.shape
    out = torch.empty((M, F), dtype=torch.float32, device=voxels.device)
    _chk(lib().rslo_vfe_mean(_ptr(voxels, torch.float32, "voxels"), _ptr(num_points, torch.int32, "num_points"),
                             M, T, F, _ptr(out), _stream()), "rslo_vfe_mean")
    return out


# --------------------------------------------------------------------------------------
# site index + rulebooks
# --------------------------------------------------------------------------------------
class SiteIndex:
    """Hash over the active sites of one level: coords [N,4] int32 (b,z,y,x)."""

    def __init__(self, coords, batch, dims):
        self.coords = coords
        self.batch = int(batch)
        self.dims = [int(d) for d in dims]
        N = coords.shape[0]
        self.cap = int(lib().rslo_hash_capacity(N))
        self.keys = torch.empty((self.cap,), dtype=torch.int32, device=coords.device)
        self.vals = torch.empty((self.cap,), dtype=torch.int32, device=coords.device)
        _chk(lib().rslo_hash_build(_ptr(coords, torch.int32, "coords"), N, self.batch, _i3(self.dims),
                                   _ptr(self.keys), _ptr(self.vals), self.cap, _stream()), "rslo_hash_build")


    @classmethod
    def from_parts(cls, coords, batch, dims, keys, vals, cap):
        """A site index whose hash already exists (built inside rslo_plan_encoder)."""
        self = cls.__new__(cls)
        self.coords, self.batch, self.dims = coords, int(batch), [int(d) for d in dims]
        self.keys, self.vals, self.cap = keys, vals, int(cap)
        return self


# -- rslo_plan_encoder: the structures of include/rslo_hip.h -------------------------------------------------------
PLAN_MAX_LEVELS, PLAN_MAX_CLOUDS = 8, 64
PLAN_CNT_OVERFLOW, PLAN_CNT_ROWS, PLAN_CNT_NVOX, PLAN_CNT_BOFF = 0, 1, 32, 176
PLAN_CNT_WORDS = 176 + PLAN_MAX_LEVELS * (PLAN_MAX_CLOUDS + 1)
_L3 = (C.c_int32 * 3) * PLAN_MAX_LEVELS
_LU64 = C.c_uint64 * PLAN_MAX_LEVELS
_LI64 = C.c_int64 * PLAN_MAX_LEVELS


class EncoderSpec(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("dims0", C.c_int32 * 3), ("subm_ks", _L3), ("conv_ks", _L3),
                ("conv_stride", _L3), ("conv_pad", _L3), ("want_pairs", C.c_int32), ("want_orders", C.c_int32),
                ("range6", C.c_float * 6), ("vsize3", C.c_float * 3), ("grid_xyz", C.c_int32 * 3),
                ("max_points", C.c_int32), ("max_voxels", C.c_int32), ("n_features", C.c_int32), ("cap_rows", _LI64)]


class PlanLayout(C.Structure):
    _fields_ = [("total_bytes", C.c_uint64), ("dims", _L3), ("cap_rows", _LI64), ("hash_cap", _LI64),
                ("counts_off", C.c_uint64), ("voxels_off", C.c_uint64), ("num_points_off", C.c_uint64),
                ("coords_frame_off", C.c_uint64), ("coords_off", _LU64), ("keys_off", _LU64), ("vals_off", _LU64),
                ("subm_nbr_off", _LU64), ("subm_pin_off", _LU64), ("subm_pout_off", _LU64), ("subm_koff_off", _LU64),
                ("conv_nbr_off", _LU64), ("conv_nbrT_off", _LU64), ("conv_order_off", _LU64), ("conv_pin_off", _LU64),
                ("conv_pout_off", _LU64), ("conv_koff_off", _LU64), ("scratch_words", C.c_int64),
                ("vox_ws_off", C.c_uint64), ("bitmap_off", C.c_uint64), ("prefix_off", C.c_uint64),
                ("scan_ws_off", C.c_uint64), ("pair_ws_off", C.c_uint64), ("keys_end_off", C.c_uint64),
                ("bitmap_level_off", _LU64), ("bitmap_end_off", C.c_uint64)]


def plan_encoder_layout(spec, n_points):
    """spec: EncoderSpec, n_points: per-cloud point counts -> PlanLayout (offsets into one arena, capacities)."""
    lay = PlanLayout()
    arr = (C.c_int64 * len(n_points))(*[int(n) for n in n_points])
    _chk(lib().rslo_plan_encoder_layout(C.byref(spec), len(n_points), arr, C.byref(lay)), "rslo_plan_encoder_layout")
    return lay


def plan_encoder(spec, lay, clouds, clouds_per_frame, arena, h_counts):
    """Enqueue voxelization + the whole rulebook chain for `clouds` (CUDA fp32 [P,F] tensors, frame-major) on the current
    stream: ONE foreign call, no host read.  arena: uint8 CUDA tensor of >= lay.total_bytes; h_counts: pinned int32
    tensor [PLAN_CNT_WORDS] that receives the counts block (valid once an event recorded after this call has passed)."""
    n = len(clouds)
    ptrs = (C.c_void_p * n)(*[_ptr(c, torch.float32, "cloud") if c.shape[0] else None for c in clouds])
    cnts = (C.c_int64 * n)(*[int(c.shape[0]) for c in clouds])
    _chk(lib().rslo_plan_encoder(C.byref(spec), C.byref(lay), n, int(clouds_per_frame), ptrs, cnts, _ptr(arena),
                                 arena.numel(), C.c_void_p(h_counts.data_ptr()), _stream()), "rslo_plan_encoder")


def plan_encoder_pad_tails(spec, lay, arena):
    """Behind plan_encoder on the current stream: rows past every level's count become padding rows (capacity-sized plan)."""
    _chk(lib().rslo_plan_encoder_pad_tails(C.byref(spec), C.byref(lay), _ptr(arena), _stream()), "rslo_plan_encoder_pad_tails")


def rulebook_subm(index, ks):
    N = index.coords.shape[0]
    K = int(ks[0] * ks[1] * ks[2])
    nbr = torch.empty((N, K), dtype=torch.int32, device=index.coords.device)
    _chk(lib().rslo_rulebook_subm(_ptr(index.coords), N, index.batch, _i3(index.dims), _i3(ks),
                                  _ptr(index.keys), _ptr(index.vals), index.cap, _ptr(nbr), _stream()),
         "rslo_rulebook_subm")
    return nbr


def conv_out_dims(in_dims, ks, stride, pad):
    return [(int(d) + 2 * int(p) - int(k)) // int(s) + 1 for d, k, s, p in zip(in_dims, ks, stride, pad)]


def rulebook_conv(index, ks, stride, pad):
    """Strided conv rulebook.  Returns (out_index: SiteIndex, nbr [M,K], nbrT [N,K]).
    One device->host read (the output count) is unavoidable: it sizes the output tensors."""
    dev = index.coords.device
    N = index.coords.shape[0]
    K = int(ks[0] * ks[1] * ks[2])
    od = conv_out_dims(index.dims, ks, stride, pad)
    words = int(lib().rslo_conv_bitmap_words(index.batch, _i3(od)))
    bitmap = torch.empty((words,), dtype=torch.int32, device=dev)
    prefix = torch.empty((words,), dtype=torch.int32, device=dev)
    swb = lib().rslo_scan_ws_bytes(words)
    sws = _ws(swb, dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    _chk(lib().rslo_conv_out_count(_ptr(index.coords), N, index.batch, _i3(ks), _i3(stride), _i3(pad),
                                   _i3(od), _ptr(bitmap), _ptr(prefix), words, _ptr(sws), swb, _ptr(cnt),
                                   _stream()), "rslo_conv_out_count")
    M = int(cnt.item())
    out_coords = torch.empty((M, 4), dtype=torch.int32, device=dev)
    _chk(lib().rslo_conv_out_coords(_ptr(bitmap), _ptr(prefix), words, index.batch, _i3(od),
                                    _ptr(out_coords), M, _stream()), "rslo_conv_out_coords")
    out_index = SiteIndex(out_coords, index.batch, od)
    nbr = torch.empty((M, K), dtype=torch.int32, device=dev)
    _chk(lib().rslo_rulebook_conv(_ptr(out_coords), M, index.batch, _i3(index.dims), _i3(ks), _i3(stride),
                                  _i3(pad), _ptr(index.keys), _ptr(index.vals), index.cap, _ptr(nbr),
                                  _stream()), "rslo_rulebook_conv")
    nbrT = torch.empty((N, K), dtype=torch.int32, device=dev)
    _chk(lib().rslo_rulebook_conv_T(_ptr(index.coords), N, index.batch, _i3(od), _i3(ks), _i3(stride),
                                    _i3(pad), _ptr(out_index.keys), _ptr(out_index.vals), out_index.cap,
                                    _ptr(nbrT), _stream()), "rslo_rulebook_conv_T")
    return out_index, nbr, nbrT


# --------------------------------------------------------------------------------------
# sparse conv arithmetic
# --------------------------------------------------------------------------------------
SPLIT_BF16 = os.environ.get("RSLO_SPCONV_SPLIT", "1") != "0"     # fp32 via 3-way bf16 splitting on the matrix cores


class WeightSplitDesc(C.Structure):
    _fields_ = [("W", C.c_void_p), ("ws_fwd", C.c_void_p), ("ws_dgrad", C.c_void_p), ("K", C.c_int32), ("cin", C.c_int32),
                ("cout", C.c_int32)]


def weight_split_many(weights):
    """weights: list of [K,cin,cout] fp32 CUDA tensors with 32/64 channels.  -> (plan, [(ws_fwd, ws_dgrad)]); run
    weight_split_run(plan) after every weight update (one launch for all layers and both orientations)."""
    dev = weights[0].device
    sizes = [lib().rslo_weight_split_bytes(*w.shape) for w in weights]
    pool = torch.empty((2 * sum(sizes),), dtype=torch.uint8, device=dev)
    arr = (WeightSplitDesc * len(weights))()
    views, off = [], 0
    for i, (w, n) in enumerate(zip(weights, sizes)):
        f, t = pool[off:off + n], pool[off + n:off + 2 * n]
        off += 2 * n
        views.append((f, t))
        arr[i] = WeightSplitDesc(_ptr(w, torch.float32, "w"), f.data_ptr(), t.data_ptr(), *w.shape)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    return {"table": table, "n": len(weights), "max": max(int(w.numel()) for w in weights), "pool": pool,
            "ptrs": [w.data_ptr() for w in weights]}, views


def weight_split_run(plan):
    _chk(lib().rslo_weight_split_many(_ptr(plan["table"]), plan["n"], plan["max"], _stream()), "rslo_weight_split_many")


def weight_split(W, transpose=False):
    """W [K,Cin,Cout] fp32 -> split-bf16 operand planes for rslo_spconv_fwd_split (transpose: data-gradient operator).
    Operands refreshed for the whole model by weight_split_many (kept on the parameter object) are reused while the
    parameter is unchanged."""
    pre = getattr(W, "_hip_split", None)
    if pre is not None and pre[2] == W._version and pre[3] == W.data_ptr():
        return pre[1] if transpose else pre[0]
    K, cin, cout = W.shape
    cin_op, cout_op = (cout, cin) if transpose else (cin, cout)
    Ws = torch.empty((lib().rslo_weight_split_bytes(K, cin, cout),), dtype=torch.uint8, device=W.device)
    _chk(lib().rslo_weight_split(_ptr(W, torch.float32, "W"), K, cin_op, cout_op, int(transpose), _ptr(Ws), _stream()),
         "rslo_weight_split")
    return Ws


ROW_ORDER = os.environ.get("RSLO_ROW_ORDER", "1") != "0"        # mask-sorted tile order (rslo_rulebook_row_order)


def rulebook_row_order(nbr, flip_k=False):
    """Scheduling order of the table's rows (int32 [n]); None when switched off (RSLO_ROW_ORDER=0)."""
    if not ROW_ORDER:
        return None
    n, K = nbr.shape
    order = torch.empty((n,), dtype=torch.int32, device=nbr.device)
    _chk(lib().rslo_rulebook_row_order(_ptr(nbr, torch.int32, "nbr"), n, K, int(flip_k), _ptr(order), _stream()),
         "rslo_rulebook_row_order")
    return order


def spconv_fwd_split(x, Ws, bias, nbr, cin, cout, flip_k=False, act_slope=1.0, order=None, n_live=None):
    n_out, K = nbr.shape
    if x.shape[1] != cin:
        raise RsloHipError("spconv_fwd_split: shape mismatch")
    out = torch.empty((n_out, cout), dtype=torch.float32, device=x.device)
    _chk(lib().rslo_spconv_fwd_split(_ptr(x, torch.float32, "x"), cin, _ptr(Ws), _ptr(bias, torch.float32, "bias"),
                                     _ptr(nbr, torch.int32, "nbr"), _ptr(order, torch.int32, "order"), n_out, K, cout,
                                     int(flip_k), float(act_slope), _ptr(out),
                                     _ptr(n_live, torch.int32, "n_live") if order is None else None, _stream()),
         "rslo_spconv_fwd_split")
    return out


def weight_to_bf16(W, transpose=False):
    """W [K,Cin,Cout] fp32 -> bf16 operand plane for rslo_spconv_fwd_bf16."""
    K, cin, cout = W.shape
    cin_op, cout_op = (cout, cin) if transpose else (cin, cout)
    Wb = torch.empty((K * cin * cout,), dtype=torch.bfloat16, device=W.device)
    _chk(lib().rslo_weight_to_bf16(_ptr(W, torch.float32, "W"), K, cin_op, cout_op, int(transpose), _ptr(Wb), _stream()),
         "rslo_weight_to_bf16")
    return Wb


def spconv_fwd_bf16(x, W, bias, nbr, flip_k=False, act_slope=1.0, transpose=False, order=None):
    """bf16 feature path: x [Nin,Cin] bfloat16, W [K,Cin,Cout] fp32 master weights, bias fp32 -> [Nout,Cout] bfloat16.
    transpose=True applies W[k]^T (the data gradient; x is then dout [Nout,Cout], nbr the transposed table)."""
    n_out, K = nbr.shape
    Kw, cin, cout = W.shape
    cin_op, cout_op = (cout, cin) if transpose else (cin, cout)
    if Kw != K or x.shape[1] != cin_op or x.dtype != torch.bfloat16:
        raise RsloHipError("spconv_fwd_bf16: shape / dtype mismatch")
    out = torch.empty((n_out, cout_op), dtype=torch.bfloat16, device=x.device)
    _chk(lib().rslo_spconv_fwd_bf16(_ptr(x, torch.bfloat16, "x"), cin_op, _ptr(weight_to_bf16(W, transpose)),
                                    _ptr(bias, torch.float32, "bias"), _ptr(nbr, torch.int32, "nbr"),
                                    _ptr(order, torch.int32, "order"), n_out, K, cout_op,
                                    int(flip_k), float(act_slope), _ptr(out), _stream()), "rslo_spconv_fwd_bf16")
    return out


def _splittable(cin, cout):
    return SPLIT_BF16 and cin in (32, 64) and cout in (32, 64)


def spconv_fwd(x, W, bias, nbr, flip_k=False, act_slope=1.0, order=None, n_live=None):
    """x [Nin,Cin], W [K,Cin,Cout], nbr [Nout,K] -> [Nout,Cout].  order: optional rulebook_row_order(nbr).
    n_live: device int32 word = how many leading rows of a capacity-laid-out table are real (n_live_dev of
    rslo_spconv_fwd / rslo_spconv_fwd_split); rows past it are left unwritten.  Ignored with an order."""
    n_out, K = nbr.shape
    Kw, cin, cout = W.shape
    if Kw != K or x.shape[1] != cin:
        raise RsloHipError("spconv_fwd: shape mismatch x%s W%s nbr%s" % (tuple(x.shape), tuple(W.shape), tuple(nbr.shape)))
    if _splittable(cin, cout):
        return spconv_fwd_split(x, weight_split(W), bias, nbr, cin, cout, flip_k, act_slope, order, n_live)
    return spconv_fwd_direct(x, W, bias, nbr, flip_k, act_slope, order, n_live)


def spconv_fwd_direct(x, W, bias, nbr, flip_k=False, act_slope=1.0, order=None, n_live=None):
    """rslo_spconv_fwd itself (fp32 MFMA kernels)."""
    n_out, K = nbr.shape
    Kw, cin, cout = W.shape
    out = torch.empty((n_out, cout), dtype=torch.float32, device=x.device)
    _chk(lib().rslo_spconv_fwd(_ptr(x, torch.float32, "x"), cin, _ptr(W, torch.float32, "W"),
                               _ptr(bias, torch.float32, "bias"), _ptr(nbr, torch.int32, "nbr"),
                               _ptr(order, torch.int32, "order"), n_out, K, cout,
                               int(flip_k), float(act_slope), _ptr(out),
                               _ptr(n_live, torch.int32, "n_live") if order is None else None, _stream()),
         "rslo_spconv_fwd")
    return out


def weight_transpose(W):
    """W [K,Cin,Cout] -> [K,Cout,Cin]."""
    K, cin, cout = W.shape
    Wt = torch.empty((K, cout, cin), dtype=torch.float32, device=W.device)
    _chk(lib().rslo_weight_transpose(_ptr(W, torch.float32, "W"), K, cin, cout, _ptr(Wt), _stream()),
         "rslo_weight_transpose")
    return Wt


def spconv_dgrad(dout, W, nbrT, flip_k=False, order=None):
    """dout [Nout,Cout], W [K,Cin,Cout], nbrT [Nin,K] -> din [Nin,Cin].
    For MFMA-shaped channel counts the gradient runs through the forward kernel on the transposed weights
    (coalesced weight reads); other shapes use the dedicated entry point."""
    Kw, cin, cout = W.shape
    if _splittable(cout, cin):
        return spconv_fwd_split(dout, weight_split(W, transpose=True), None, nbrT, cout, cin, flip_k, order=order)
    if cin % 16 == 0 and cout % 16 == 0:
        return spconv_fwd(dout, weight_transpose(W), None, nbrT, flip_k=flip_k, order=order)
    return spconv_dgrad_direct(dout, W, nbrT, flip_k, order)


def spconv_dgrad_direct(dout, W, nbrT, flip_k=False, order=None):
    """rslo_spconv_dgrad itself (weights read in place, transposed access)."""
    n_in, K = nbrT.shape
    Kw, cin, cout = W.shape
    if Kw != K or dout.shape[1] != cout:
        raise RsloHipError("spconv_dgrad: shape mismatch")
    din = torch.empty((n_in, cin), dtype=torch.float32, device=dout.device)
    _chk(lib().rslo_spconv_dgrad(_ptr(dout, torch.float32, "dout"), cout, _ptr(W, torch.float32, "W"),
                                 _ptr(nbrT, torch.int32, "nbrT"), _ptr(order, torch.int32, "order"), n_in, K, cin,
                                 int(flip_k), _ptr(din), _stream()), "rslo_spconv_dgrad")
    return din


def spconv_wgrad(x, dout, nbr, cin, cout, with_bias=True):
    n_out, K = nbr.shape
    dev = x.device
    dW = torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if with_bias else None
    wsb = lib().rslo_spconv_wgrad_ws_bytes(n_out, K, cin, cout)
    ws = _ws(wsb, dev)
    _chk(lib().rslo_spconv_wgrad(_ptr(x, torch.float32, "x"), cin, _ptr(dout, torch.float32, "dout"), cout,
                                 _ptr(nbr, torch.int32, "nbr"), n_out, K, _ptr(ws), wsb, _ptr(dW), _ptr(db),
                                 _stream()), "rslo_spconv_wgrad")
    return dW, db


def rulebook_pairs(nbr):
    """nbr [rows,K] -> (pairs_in [rows*K cap], pairs_out [rows*K cap], koff [K+1] on device)."""
    n, K = nbr.shape
    dev = nbr.device
    cap = max(n * K, 1)
    pin = torch.empty((cap,), dtype=torch.int32, device=dev)
    pout = torch.empty((cap,), dtype=torch.int32, device=dev)
    koff = torch.empty((K + 1,), dtype=torch.int32, device=dev)
    wsb = lib().rslo_rulebook_pairs_ws_bytes(n, K)
    ws = _ws(wsb, dev)
    _chk(lib().rslo_rulebook_pairs(_ptr(nbr, torch.int32, "nbr"), n, K, _ptr(ws), wsb, _ptr(pin), _ptr(pout),
                                   _ptr(koff), _stream()), "rslo_rulebook_pairs")
    return pin, pout, koff


def spconv_wgrad_pairs(x, dout, pairs, n_out, K, cin, cout, with_bias=True, bias_partial=None):
    """pairs = (pairs_in, pairs_out, koff) over rows of x (in) and dout (out).
    bias_partial: per-block column sums of dout from leaky_bwd(..., colsum=True) (saves a pass over dout)."""
    pin, pout, koff = pairs
    dev = x.device
    dW = torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if with_bias else None
    wsb = lib().rslo_spconv_wgrad_pairs_ws_bytes(n_out, K, cin, cout)
    ws = _ws(wsb, dev)
    _chk(lib().rslo_spconv_wgrad_pairs(_ptr(x, torch.float32, "x"), cin, _ptr(dout, torch.float32, "dout"), cout,
                                       _ptr(pin, torch.int32, "pairs_in"), _ptr(pout, torch.int32, "pairs_out"),
                                       _ptr(koff, torch.int32, "koff"), n_out, K, _ptr(ws), wsb, _ptr(dW), _ptr(db),
                                       _ptr(bias_partial if with_bias else None),
                                       0 if bias_partial is None else bias_partial.shape[0], _stream()),
         "rslo_spconv_wgrad_pairs")
    _keep_for_reduce(ws, bias_partial, koff)
    return dW, db


def leaky_bwd(y, dout, slope, colsum=False):
    """g = dout * (y > 0 ? 1 : slope); colsum=True also returns per-block column sums of g ([blocks, cols]) when the
    row width divides 1024 (else None)."""
    g = torch.empty_like(dout)
    if colsum:
        rows, cols = dout.shape
        if cols >= 4 and 1024 % cols == 0:
            nblk = int(lib().rslo_leaky_bwd_colsum_blocks(rows, cols))
            part = torch.empty((nblk, cols), dtype=torch.float32, device=dout.device)
            _chk(lib().rslo_leaky_bwd_colsum(_ptr(y, torch.float32, "y"), _ptr(dout, torch.float32, "dout"), rows, cols,
                                             float(slope), _ptr(g), _ptr(part), _stream()), "rslo_leaky_bwd_colsum")
            return g, part
        colsum = None
    _chk(lib().rslo_leaky_bwd(_ptr(y, torch.float32, "y"), _ptr(dout, torch.float32, "dout"), y.numel(),
                              float(slope), _ptr(g), _stream()), "rslo_leaky_bwd")
    return (g, None) if colsum is None else g


def leaky_bwd_bf16(y, dout, slope, colsum=False):
    """bf16 rows: g = dout * (y > 0 ? 1 : slope) in bf16; colsum -> (g, per-block fp32 column sums [blocks, cols])."""
    rows, cols = dout.shape
    g = torch.empty_like(dout)
    part = None
    if colsum:
        nblk = int(lib().rslo_leaky_bwd_colsum_bf16_blocks(rows, cols))
        part = torch.empty((nblk, cols), dtype=torch.float32, device=dout.device)
    _chk(lib().rslo_leaky_bwd_colsum_bf16(_ptr(y, torch.bfloat16, "y"), _ptr(dout, torch.bfloat16, "dout"), rows, cols,
                                          float(slope), _ptr(g), _ptr(part), _stream()), "rslo_leaky_bwd_colsum_bf16")
    return (g, part) if colsum else g


def spconv_wgrad_pairs_bf16(x, dout, pairs, n_out, K, cin, cout, bias_partial=None):
    """bf16 rows on both sides -> fp32 (dW [K,cin,cout], dbias or None); dbias needs bias_partial (leaky_bwd_bf16)."""
    pin, pout, koff = pairs
    dev = x.device
    dW = torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if bias_partial is not None else None
    wsb = lib().rslo_spconv_wgrad_pairs_ws_bytes(n_out, K, cin, cout)
    ws = _ws(wsb, dev)
    _chk(lib().rslo_spconv_wgrad_pairs_bf16(_ptr(x, torch.bfloat16, "x"), cin, _ptr(dout, torch.bfloat16, "dout"), cout,
                                            _ptr(pin, torch.int32, "pairs_in"), _ptr(pout, torch.int32, "pairs_out"),
                                            _ptr(koff, torch.int32, "koff"), n_out, K, _ptr(ws), wsb, _ptr(dW), _ptr(db),
                                            _ptr(bias_partial), 0 if bias_partial is None else bias_partial.shape[0],
                                            _stream()), "rslo_spconv_wgrad_pairs_bf16")
    _keep_for_reduce(ws, bias_partial, koff)
    return dW, db


def segbn_fwd(x, seg_off, S, max_len, gamma, beta, running_mean, running_var, momentum, eps, act_slope):
    """-> (y, save_mean [S,C], save_invstd [S,C]); running stats updated in place, segment after segment."""
    n, Cc = x.shape
    dev = x.device
    y = torch.empty_like(x)
    mean = torch.empty((S, Cc), dtype=torch.float32, device=dev)
    invstd = torch.empty((S, Cc), dtype=torch.float32, device=dev)
    wsb = lib().rslo_segbn_ws_bytes(S, max_len, Cc)
    ws = _ws(wsb, dev)
    _chk(lib().rslo_segbn_fwd(_ptr(x, torch.float32, "x"), Cc, _ptr(seg_off, torch.int32, "seg_off"), S, max_len,
                              _ptr(gamma, torch.float32, "gamma"), _ptr(beta, torch.float32, "beta"),
                              _ptr(running_mean, torch.float32, "running_mean"),
                              _ptr(running_var, torch.float32, "running_var"), float(momentum), float(eps),
                              float(act_slope), _ptr(ws), wsb, _ptr(y), _ptr(mean), _ptr(invstd), _stream()),
         "rslo_segbn_fwd")
    return y, mean, invstd


def bn1d_eval_act(x, running_mean, running_var, gamma, beta, eps, act_slope=1.0, n_live=None):
    """Eval-mode BatchNorm1d + (Leaky)ReLU over [n, C] fp32 rows in one launch (rslo_bn1d_eval_act)."""
    n, Cc = x.shape
    y = torch.empty_like(x)
    _chk(lib().rslo_bn1d_eval_act(_ptr(x, torch.float32, "x"), n, Cc, _ptr(running_mean, torch.float32, "running_mean"),
                                  _ptr(running_var, torch.float32, "running_var"), _ptr(gamma, torch.float32, "gamma"),
                                  _ptr(beta, torch.float32, "beta"), float(eps), float(act_slope),
                                  _ptr(n_live, torch.int32, "n_live"), _ptr(y), _stream()), "rslo_bn1d_eval_act")
    return y


def segbn_bwd(x, y, gy, seg_off, S, max_len, gamma, mean, invstd, act_slope):
    n, Cc = x.shape
    dev = x.device
    gx = torch.empty_like(x)
    dgamma = torch.empty((Cc,), dtype=torch.float32, device=dev)
    dbeta = torch.empty((Cc,), dtype=torch.float32, device=dev)
    wsb = lib().rslo_segbn_ws_bytes(S, max_len, Cc) + 2 * S * Cc * 4
    ws = _ws(wsb, dev)
    _chk(lib().rslo_segbn_bwd(_ptr(x, torch.float32, "x"), _ptr(y, torch.float32, "y"), _ptr(gy, torch.float32, "gy"),
                              Cc, _ptr(seg_off, torch.int32, "seg_off"), S, max_len,
                              _ptr(gamma, torch.float32, "gamma"), _ptr(mean), _ptr(invstd), float(act_slope),
                              _ptr(ws), wsb, _ptr(gx), _ptr(dgamma), _ptr(dbeta), _stream()), "rslo_segbn_bwd")
    return gx, dgamma, dbeta


def dense_scatter(feat, coords, batch, dims, frames=1, out=None):
    """[M,C] rows -> [batch, C, D, H, W]; frames > 1: [batch / frames, frames, C, D, H, W] (rows of frame t of sample b
    carry the batch index t * (batch / frames) + b).  out: a contiguous fp32 buffer of that many elements to write into
    (the static input of a replayed head graph: rslo_amd/headgraph.py) -- returned viewed to the shape above."""
    M, Cc = feat.shape
    shape = (batch, Cc, dims[0], dims[1], dims[2]) if frames == 1 else (batch // frames, frames, Cc, dims[0], dims[1], dims[2])
    if out is not None:
        n = 1
        for v in shape:
            n *= int(v)
        if not (out.is_contiguous() and out.dtype == torch.float32 and out.device == feat.device and out.numel() == n):
            raise RsloHipError("dense_scatter: `out` must be a contiguous fp32 buffer of %d elements on %s" % (n, feat.device))
        # a tensor of its own over the same memory (not a view of `out`: the result is an autograd output)
        strides, acc = [], 1
        for v in reversed(shape):
            strides.append(acc)
            acc *= int(v)
        out = torch.empty(0, dtype=torch.float32, device=feat.device).set_(out.untyped_storage(), out.storage_offset(), shape,
                                                                          tuple(reversed(strides)))
    else:
        out = torch.empty(shape, dtype=torch.float32, device=feat.device)
    _chk(lib().rslo_dense_scatter_frames(_ptr(feat, torch.float32, "feat"), _ptr(coords, torch.int32, "coords"), M, Cc,
                                         int(batch), int(frames), _i3(dims), _ptr(out), _stream()), "rslo_dense_scatter")
    return out


def dense_gather(dense, coords, C_, batch, dims, frames=1):
    M = coords.shape[0]
    out = torch.empty((M, C_), dtype=torch.float32, device=dense.device)
    _chk(lib().rslo_dense_gather_frames(_ptr(dense, torch.float32, "dense"), _ptr(coords, torch.int32, "coords"), M, C_,
                                        int(batch), int(frames), _i3(dims), _ptr(out), _stream()), "rslo_dense_gather")
    return out


def bev_channel_sums(bev, groups, masks=False):
    """bev [B, groups * Cg, H, W] fp32 -> [B, groups, H, W]: per-cell sum over each channel group, one pass.
    masks=True: also (mask_f float, mask_b bool, outside_b bool) [B,1,H,W] = occupancy of group 0 from the same launch."""
    B, Ct, H, W = bev.shape
    out = torch.empty((B, groups, H, W), dtype=torch.float32, device=bev.device)
    if masks:
        mf = torch.empty((B, 1, H, W), dtype=torch.float32, device=bev.device)
        mb = torch.empty((B, 1, H, W), dtype=torch.bool, device=bev.device)
        ob = torch.empty((B, 1, H, W), dtype=torch.bool, device=bev.device)
        _chk(lib().rslo_bev_channel_sums_masks(_ptr(bev, torch.float32, "bev"), B, int(groups), Ct // int(groups), H * W,
                                               _ptr(out), _ptr(mf), _ptr(mb), _ptr(ob), _stream()),
             "rslo_bev_channel_sums_masks")
        return out, mf, mb, ob
    _chk(lib().rslo_bev_channel_sums(_ptr(bev, torch.float32, "bev"), B, int(groups), Ct // int(groups), H * W, _ptr(out),
                                     _stream()), "rslo_bev_channel_sums")
    return out


def pose_tail_fwd(odom):
    """odom [B,7] -> (t [B,3], r [B,4] = q / (|q| + 1e-12))."""
    B = odom.shape[0]
    t = torch.empty((B, 3), dtype=torch.float32, device=odom.device)
    r = torch.empty((B, 4), dtype=torch.float32, device=odom.device)
    _chk(lib().rslo_pose_tail_fwd(_ptr(odom, torch.float32, "odom"), B, _ptr(t), _ptr(r), _stream()), "rslo_pose_tail_fwd")
    return t, r


def pose_tail_bwd(odom, g_t, g_r):
    B = odom.shape[0]
    d = torch.empty((B, 7), dtype=torch.float32, device=odom.device)
    _chk(lib().rslo_pose_tail_bwd(_ptr(odom, torch.float32, "odom"), _dp(g_t), _dp(g_r), B, _ptr(d), _stream()),
         "rslo_pose_tail_bwd")
    return d


def cat_upsample_fwd(a, b, scale):
    """a [B,Ca,H,W], b [B,Cb,H,W] contiguous fp32 -> nearest upsampling by `scale` of cat([a, b], 1), one launch."""
    B, Ca, H, W = a.shape
    Cb = b.shape[1]
    if tuple(b.shape) != (B, Cb, H, W):
        raise ValueError("cat_upsample_fwd: shapes %s / %s" % (tuple(a.shape), tuple(b.shape)))
    out = torch.empty((B, Ca + Cb, H * scale, W * scale), dtype=torch.float32, device=a.device)
    _chk(lib().rslo_cat_upsample_fwd(_ptr(a, torch.float32, "a"), _ptr(b, torch.float32, "b"), B, Ca, Cb, H, W, int(scale),
                                     _ptr(out), _stream()), "rslo_cat_upsample_fwd")
    return out


def cat_upsample_bwd(grad, Ca, Cb, scale, need_a=True, need_b=True):
    """grad [B,Ca+Cb,s*H,s*W] -> (da [B,Ca,H,W], db [B,Cb,H,W]) (None where not needed)."""
    B, Ct, Hs, Ws = grad.shape
    H, W = Hs // scale, Ws // scale
    da = torch.empty((B, Ca, H, W), dtype=torch.float32, device=grad.device) if need_a else None
    db = torch.empty((B, Cb, H, W), dtype=torch.float32, device=grad.device) if need_b else None
    _chk(lib().rslo_cat_upsample_bwd(_ptr(grad, torch.float32, "grad"), B, Ca, Cb, H, W, int(scale), _dp(da), _dp(db),
                                     _stream()), "rslo_cat_upsample_bwd")
    return da, db


def bev_display(sums, channels):
    """sums [B, T, H, W] from bev_channel_sums over `channels` channels per frame -> (feature_mask [B,1,H,W],
    [middle_feature_t [B,1,H,W] for t]) in two launches (see rslo_bev_display)."""
    B, T, H, W = sums.shape
    mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=sums.device)
    disp = torch.empty((T, B, 1, H, W), dtype=torch.float32, device=sums.device)
    wsb = lib().rslo_bev_display_ws_bytes(T)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=sums.device)
    _chk(lib().rslo_bev_display(_ptr(sums, torch.float32, "sums"), B, T, int(channels), H * W, _ptr(mask), _ptr(disp),
                                ws.data_ptr(), wsb, _stream()), "rslo_bev_display")
    return mask, list(disp.unbind(0))


# --------------------------------------------------------------------------------------
# chamfer
# --------------------------------------------------------------------------------------
def chamfer_nn(xyz1, xyz2, dist=None, idx=None, ncnt=None, mcnt=None, method=None):
    """ncnt / mcnt: optional int32 [B] device tensors for a ragged (padded) batch.
    method: None (library picks), "brute" (exhaustive scan) or "grid" (pruned search) -- identical results."""
    entry = {None: "rslo_chamfer_nn_ragged", "brute": "rslo_chamfer_brute_nn", "grid": "rslo_chamfer_grid_nn"}[method]
    B, N, _ = xyz1.shape
    M = xyz2.shape[1]
    dev = xyz1.device
    if dist is None:
        dist = torch.empty((B, N), dtype=torch.float32, device=dev)
    if idx is None:
        idx = torch.empty((B, N), dtype=torch.int32, device=dev)
    wsb = lib().rslo_chamfer_ws_bytes(B, N, M)
    ws = _ws(wsb, dev)
    _chk(getattr(lib(), entry)(_ptr(xyz1, torch.float32, "xyz1"), _ptr(xyz2, torch.float32, "xyz2"), B, N, M,
                               _ptr(ncnt, torch.int32, "ncnt"), _ptr(mcnt, torch.int32, "mcnt"),
                               _ptr(dist, torch.float32, "dist"), _ptr(idx, torch.int32, "idx"), _ptr(ws), wsb,
                               _stream()), entry)
    return dist, idx


# --------------------------------------------------------------------------------------
# point normals of a raw scan (csrc/normals.hip)
# --------------------------------------------------------------------------------------
def estimate_normals(points, radius=0.6, max_nn=30, viewpoint=None, zero_vertical=False, out=None, counts=None, ws=None):
    """points: contiguous fp32 CUDA [P, F >= 3] (x, y, z first; read in place through its row stride).  Returns
    (normals [P, 3] fp32, counts [P] int32): script/create_hdf5.py:130-147 on the current stream (rules: include/rslo_hip.h).
    out / counts / ws: optional preallocated outputs and workspace (ws: uint8, >= rslo_normals_ws_bytes(P))."""
    src = _ptr(points, torch.float32, "points")
    if points.dim() != 2 or points.shape[1] < 3:
        raise RsloHipError("estimate_normals: points must be [P, F >= 3], got %s" % (tuple(points.shape),))
    P, F = points.shape
    dev = points.device
    if out is None:
        out = torch.empty((P, 3), dtype=torch.float32, device=dev)
    if counts is None:
        counts = torch.empty((P,), dtype=torch.int32, device=dev)
    if out.shape != (P, 3) or counts.shape != (P,):
        raise RsloHipError("estimate_normals: out must be [P, 3] and counts [P]")
    wsb = lib().rslo_normals_ws_bytes(P)
    if ws is None:
        ws = _ws(wsb, dev)
    vp = None if viewpoint is None else _F3(*[float(v) for v in viewpoint])
    _chk(lib().rslo_estimate_normals(src, F, P, float(radius), int(max_nn), vp, int(bool(zero_vertical)),
                                     _ptr(out, torch.float32, "out"), _ptr(counts, torch.int32, "counts"), _ptr(ws),
                                     ws.numel() * ws.element_size(), _stream()), "rslo_estimate_normals")
    return out, counts


def append_normals(points_xyzi, radius=0.6, max_nn=30, viewpoint=None, out=None, counts=None, ws=None, normals=None):
    """A raw [P, 4] scan (or [P, 3]: intensity 0) -> the [P, 7] cloud the reference's reader produces
    (kitti_dataset_hdf5.py:253-261): cat(x, y, z, intensity, normals with the reader's zero_vertical rule).
    out: optional [>= P, 7] fp32 buffer whose first P rows are written and returned; normals / counts / ws: optional
    [>= P, 3] fp32, [>= P] int32 and workspace buffers (a caller that must not allocate passes all four)."""
    _ptr(points_xyzi, torch.float32, "points")
    if points_xyzi.dim() != 2 or points_xyzi.shape[1] not in (3, 4):
        raise RsloHipError("append_normals: a raw scan is [P, 4] (x, y, z, intensity) or [P, 3], got %s"
                           % (tuple(points_xyzi.shape),))
    P, F = points_xyzi.shape
    if out is None:
        out = torch.empty((P, 7), dtype=torch.float32, device=points_xyzi.device)
    if out.dim() != 2 or out.shape[1] != 7 or out.shape[0] < P or not out.is_contiguous():
        raise RsloHipError("append_normals: out must be a contiguous [>= P, 7] buffer")
    cloud = out[:P]
    cloud[:, :F].copy_(points_xyzi)
    if F == 3:
        cloud[:, 3].zero_()
    nrm, _ = estimate_normals(points_xyzi, radius, max_nn, viewpoint, True, out=None if normals is None else normals[:P],
                              counts=None if counts is None else counts[:P], ws=ws)
    cloud[:, 4:].copy_(nrm)
    return cloud


# --------------------------------------------------------------------------------------
# voxel down-sample of a cloud (csrc/downsample.hip)
# --------------------------------------------------------------------------------------
def _rows3(t, name):
    """(pointer, row stride in floats) of an fp32 CUDA [P, >= 3] tensor or column view whose rows are read in place"""
    if not t.is_cuda:
        raise RsloHipError("%s must live on the GPU (the RSLO hot path has no CPU fallback)" % name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < 3:
        raise RsloHipError("%s must be fp32 [P, >= 3], got %s %s" % (name, t.dtype, tuple(t.shape)))
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < 3):
        raise RsloHipError("%s: rows must be unit-stride with a row stride >= 3, got strides %s" % (name, t.stride()))
    return t.data_ptr(), (int(t.stride(0)) if t.shape[0] > 1 else max(int(t.shape[1]), 3))


def voxel_downsample(points, normals=None, voxel_size=0.1, *, out=None, index=None, npts=None, counts=None, ws=None,
                     sync=True):
    """script/create_hdf5.py:149-165 (Open3D voxel_down_sample) on the current stream; rules: include/rslo_hip.h.
    points: fp32 CUDA [P, F >= 3], read in place through its row stride.  normals: None (rows are xyz only) or [P, 3],
    possibly a strided view such as cloud[:, 4:7].  Rows are [., 6] with normals and [., 3] without.
    index / npts: None = not wanted, True = allocate, or a preallocated int32 [P]: the output row of every point (-1
    for an invalid one) and the points per output row.  out [P, 6 | 3], counts int32 [2] and ws (uint8, >=
    rslo_voxel_downsample_ws_bytes(P)) may be preallocated too.
    sync=True reads counts once, raises RsloHipError on the overflow flag and returns out[:Q], or the tuple
    (out[:Q], [index,] [npts[:Q]]) when index / npts were asked for.  sync=False reads nothing on the host (the form
    to use under capture) and returns (out, index, npts, counts): capacity-sized buffers, None where not asked for, and
    the device counts = {Q, flags}."""
    src, stride = _rows3(points, "points")
    P = points.shape[0]
    dev = points.device
    nsrc, nstride = None, 0
    if normals is not None:
        nsrc, nstride = _rows3(normals, "normals")
        if normals.shape != (P, 3):
            raise RsloHipError("voxel_downsample: normals must be [P, 3], got %s" % (tuple(normals.shape),))
    width = 3 if normals is None else 6
    if out is None:
        out = torch.empty((P, width), dtype=torch.float32, device=dev)
    if out.shape != (P, width):
        raise RsloHipError("voxel_downsample: out must be [P, %d], got %s" % (width, tuple(out.shape)))
    if index is True:
        index = torch.empty((P,), dtype=torch.int32, device=dev)
    if npts is True:
        npts = torch.empty((P,), dtype=torch.int32, device=dev)
    for name, t in (("index", index), ("npts", npts)):
        if t is not None and t.shape != (P,):
            raise RsloHipError("voxel_downsample: %s must be [P]" % name)
    if counts is None:
        counts = torch.empty((2,), dtype=torch.int32, device=dev)
    if counts.shape != (2,):
        raise RsloHipError("voxel_downsample: counts must be [2]")
    if ws is None:
        ws = _ws(lib().rslo_voxel_downsample_ws_bytes(P), dev)
    _chk(lib().rslo_voxel_downsample(src, stride, nsrc, nstride, P, float(voxel_size), _ptr(out, torch.float32, "out"),
                                     _ptr(index, torch.int32, "index"), _ptr(npts, torch.int32, "npts"),
                                     _ptr(counts, torch.int32, "counts"), _ptr(ws), ws.numel() * ws.element_size(),
                                     _stream()), "rslo_voxel_downsample")
    if not sync:
        return out, index, npts, counts
    Q, flags = counts.tolist()
    if flags & 1:
        raise RsloHipError("voxel_downsample: the cloud spans 2^21 or more cells of %g along an axis" % float(voxel_size))
    res = (out[:Q],) + (() if index is None else (index,)) + (() if npts is None else (npts[:Q],))
    return res[0] if len(res) == 1 else res


# --------------------------------------------------------------------------------------
# world voxel map of a streamed trajectory (csrc/map.hip); the owning class is rslo_amd/mapping.py VoxelMap
# --------------------------------------------------------------------------------------
MAP_HDR_COUNTERS = 8      # first int64 word of the six counters in a map's header (include/rslo_hip.h)
MAP_COUNTERS = ("n_scans", "n_cells", "n_points", "dropped_invalid", "dropped_range", "dropped_full")


def map_bytes(capacity):
    """rslo_map_bytes: bytes of a map of `capacity` slots, 0 unless capacity is a power of two >= 1024."""
    return int(lib().rslo_map_bytes(int(capacity)))


def _map_buf(buf):
    if not (torch.is_tensor(buf) and buf.is_cuda and buf.dtype == torch.int64 and buf.dim() == 1 and buf.is_contiguous()):
        raise RsloHipError("map: the buffer must be a contiguous int64 CUDA vector of rslo_map_bytes(capacity) bytes")
    return buf.data_ptr(), buf.numel() * 8


def _pose7(pose, name):
    if not (torch.is_tensor(pose) and pose.is_cuda and pose.dtype == torch.float64 and pose.numel() == 7
            and pose.is_contiguous()):
        raise RsloHipError("%s: pose must be 7 contiguous float64 values (t, q wxyz) on the GPU" % name)
    return pose.data_ptr()


def _insert_frames(name, buf, store_buf, capacity, K, poses):
    """the body of map_insert_frames / surfel_insert_frames: rslo_<name> with the checks both make"""
    ptr, nbytes = _map_buf(buf)
    sptr, sbytes = _map_buf(store_buf)
    if not (torch.is_tensor(poses) and poses.is_cuda and poses.dtype == torch.float64 and poses.dim() == 2
            and poses.shape[1] == 7 and poses.is_contiguous()):
        raise RsloHipError("%s: poses must be contiguous float64 [n, 7] rows (t, q wxyz) on the GPU" % name)
    if poses.device != buf.device or store_buf.device != buf.device:
        raise RsloHipError("%s: the map, the store and the poses must live on one device" % name)
    if poses.shape[0] == 0:      # an empty tensor has no address to hand over; the call would launch nothing
        return
    _chk(getattr(lib(), "rslo_" + name)(ptr, nbytes, sptr, sbytes, int(capacity), int(K), poses.data_ptr(),
                                        int(poses.shape[0]), _stream()), "rslo_" + name)


def _prune_ws(name, capacity, device):
    """the body of map_prune_ws / surfel_prune_ws: rslo_<name>_bytes(capacity) bytes as an int64 tensor"""
    nbytes = int(getattr(lib(), "rslo_%s_bytes" % name)(int(capacity)))
    if nbytes == 0:
        raise RsloHipError("%s: capacity must be a power of two >= 1024, got %r" % (name, capacity))
    return torch.empty((nbytes // 8,), dtype=torch.int64, device=device)


def _center3(name, center, exact):
    """the address of a centre argument, None for None: float64 CUDA, contiguous, of 3 (exact: an export) or >= 3
    elements (a prune)"""
    if center is None:
        return None
    if not (torch.is_tensor(center) and center.is_cuda and center.dtype == torch.float64 and center.is_contiguous()
            and (center.numel() == 3 if exact else center.numel() >= 3)):
        raise RsloHipError("%s: center must be %s contiguous float64 values on the GPU" % (name, "3" if exact else ">= 3"))
    return center.data_ptr()


def map_reset(buf, capacity, voxel_size, min_range=0.0, max_range=float("inf")):
    """rslo_map_reset on the current stream: empties the table and writes the header (rules: include/rslo_hip.h)."""
    ptr, nbytes = _map_buf(buf)
    _chk(lib().rslo_map_reset(ptr, nbytes, int(capacity), float(voxel_size), float(min_range), float(max_range),
                              _stream()), "rslo_map_reset")


def map_insert(buf, points, pose, ws):
    """rslo_map_insert: one scan (fp32 CUDA [P, F >= 3], read in place; F >= 4: column 3 is the intensity) under pose
    (float64 CUDA [7]) on the current stream.  ws: uint8, >= rslo_map_insert_ws_bytes(P).  No host read."""
    ptr, nbytes = _map_buf(buf)
    src, stride = _rows3(points, "points")
    _chk(lib().rslo_map_insert(ptr, nbytes, src, stride, int(points.shape[1]), int(points.shape[0]),
                               _pose7(pose, "map_insert"), _ptr(ws), ws.numel() * ws.element_size(), _stream()),
         "rslo_map_insert")


def map_insert_frames(buf, store_buf, capacity, K, poses):
    """rslo_map_insert_frames on the current stream: every frame of the keyframe store store_buf (its capacity and K as
    handed to keyframe_reset) under its own row of poses (float64 CUDA [n, 7], contiguous, read in place), as n
    successive map_insert calls would leave the map; n is clamped to the store's entry count on the device.  Three
    launches, no workspace, no host read."""
    _insert_frames("map_insert_frames", buf, store_buf, capacity, K, poses)


def map_lookup(buf, points, pose, hits=None, tags=None):
    """rslo_map_lookup: hits int32 [P] (-1 skipped / out of range, 0 not in the map, else the cell's hits); tags: None =
    not wanted, True = allocate, or an int64 [P] tensor (all-ones, i.e. -1, where hits <= 0).  Returns hits or (hits, tags)."""
    ptr, nbytes = _map_buf(buf)
    src, stride = _rows3(points, "points")
    P = points.shape[0]
    if hits is None:
        hits = torch.empty((P,), dtype=torch.int32, device=points.device)
    if tags is True:
        tags = torch.empty((P,), dtype=torch.int64, device=points.device)
    if hits.shape != (P,) or (tags is not None and tags.shape != (P,)):
        raise RsloHipError("map_lookup: hits and tags must be [P]")
    _chk(lib().rslo_map_lookup(ptr, nbytes, src, stride, P, _pose7(pose, "map_lookup"), _ptr(hits, torch.int32, "hits"),
                               _ptr(tags, torch.int64, "tags"), _stream()), "rslo_map_lookup")
    return hits if tags is None else (hits, tags)


def map_export(buf, min_hits=1, center=None, radius=0.0, rows=None, tags=None, hits=None, counts=None):
    """rslo_map_export into preallocated rows fp32 [R, 4], tags int64 [R], hits int32 [R] (all None: R = 0, count only);
    center: None or float64 CUDA [3].  Returns counts, int64 CUDA [2] = {matching, written}.  No host read."""
    ptr, nbytes = _map_buf(buf)
    R = 0 if rows is None else rows.shape[0]
    if R and (rows.shape != (R, 4) or tags is None or hits is None or tags.shape != (R,) or hits.shape != (R,)):
        raise RsloHipError("map_export: rows [R, 4], tags [R] and hits [R] go together")
    cptr = _center3("map_export", center, exact=True)
    if counts is None:
        counts = torch.empty((2,), dtype=torch.int64, device=buf.device)
    _chk(lib().rslo_map_export(ptr, nbytes, int(min_hits), cptr, float(radius),
                               _ptr(rows, torch.float32, "rows") if R else None,
                               _ptr(tags, torch.int64, "tags") if R else None,
                               _ptr(hits, torch.int32, "hits") if R else None, R,
                               _ptr(counts, torch.int64, "counts"), _stream()), "rslo_map_export")
    return counts


MAP_HDR_PRUNE = 5         # first int64 word of n_prunes, n_evicted, n_lost in a map's header
MAP_PRUNE_COUNTERS = ("n_prunes", "n_evicted", "n_lost")


def map_prune_ws(capacity, device):
    """a workspace for map_prune on a map of `capacity` slots: rslo_map_prune_ws_bytes(capacity) bytes"""
    return _prune_ws("map_prune_ws", capacity, device)


def map_prune(buf, ws, center=None, radius=0.0, min_hits=1, grace=0):
    """rslo_map_prune on the current stream: evict the cells that are not within radius of center (None: no such test;
    else float64 CUDA, contiguous, >= 3 elements, read in place: a [7] trajectory row will do) or that have fewer than
    min_hits hits and are at least `grace` scans old, by rebuilding the table through ws (map_prune_ws).  No host read."""
    ptr, nbytes = _map_buf(buf)
    cptr = _center3("map_prune", center, exact=False)
    if not (torch.is_tensor(ws) and ws.is_cuda and ws.is_contiguous()):
        raise RsloHipError("map_prune: ws must be a contiguous CUDA tensor (map_prune_ws)")
    _chk(lib().rslo_map_prune(ptr, nbytes, cptr, float(radius), int(min_hits),
                              int(grace), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()), "rslo_map_prune")


# free-space carving (csrc/carve.hip; rules: include/rslo_hip.h "Free-space carving")
MAP_HDR_CARVE = 14        # first int64 word of n_carves, n_carved in a map's header
MAP_CARVE_COUNTERS = ("n_carves", "n_carved")


def _range_img(img, H, W, name):
    if not (torch.is_tensor(img) and img.is_cuda and img.dtype == torch.int32 and img.shape == (int(H), int(W))
            and img.is_contiguous()):
        raise RsloHipError("%s: the image must be a contiguous int32 CUDA [%d, %d] tensor (the uint32 range words)"
                           % (name, H, W))
    return img.data_ptr()


def range_image(points, img, tan_lo, tan_hi):
    """rslo_range_image on the current stream: the rows of points (fp32 CUDA [P, F >= 3], read in place, any row stride)
    binned into img (int32 CUDA [H, W], holding the uint32 bit patterns of the nearest range per pixel, all-ones = empty)
    over the elevation tangents [tan_lo, tan_hi).  Two launches, no host read."""
    src, stride = _rows3(points, "range_image: points")
    H, W = img.shape if torch.is_tensor(img) and img.dim() == 2 else (0, 0)
    N = int(points.shape[0])
    _chk(lib().rslo_range_image(src if N else None, stride, N, int(H), int(W), float(tan_lo), float(tan_hi),
                                _range_img(img, H, W, "range_image"), _stream()), "rslo_range_image")
    return img


def map_carve(buf, ws, img, tan_lo, tan_hi, pose, win_rows=1, win_cols=1, margin_abs=0.3, margin_rel=0.0,
              max_range=60.0, grace=1):
    """rslo_map_carve on the current stream: evict the cells of the map that the scan behind img (range_image) sees
    through from pose (float64 CUDA [7], read in place), by rebuilding the table through ws (map_prune_ws).  No host
    read."""
    ptr, nbytes = _map_buf(buf)
    H, W = img.shape if torch.is_tensor(img) and img.dim() == 2 else (0, 0)
    if not (torch.is_tensor(ws) and ws.is_cuda and ws.is_contiguous()):
        raise RsloHipError("map_carve: ws must be a contiguous CUDA tensor (map_prune_ws)")
    _chk(lib().rslo_map_carve(ptr, nbytes, _range_img(img, H, W, "map_carve"), int(H), int(W), float(tan_lo), float(tan_hi),
                              _pose7(pose, "map_carve"), int(win_rows), int(win_cols), float(margin_abs), float(margin_rel),
                              float(max_range), int(grace), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()),
         "rslo_map_carve")


# scan-to-map registration (csrc/mapreg.hip; rules: include/rslo_hip.h "Scan-to-map registration")
MAP_METRICS = {"point": 0, "plane": 1}


def map_params(buf):
    """rslo_map_params: (voxel_size, min_range, max_range) of a map, read on the host (synchronises the current stream)."""
    ptr, nbytes = _map_buf(buf)
    out = (C.c_double * 3)()
    _chk(lib().rslo_map_params(ptr, nbytes, out, _stream()), "rslo_map_params")
    return tuple(out)


def _map_metric(metric):
    if metric not in MAP_METRICS:
        raise RsloHipError("map: metric must be \"point\" or \"plane\", got %r" % (metric,))
    return MAP_METRICS[metric]


def map_nearest(buf, points, pose, voxel_size=None, max_dist=None, min_hits=1, rows=None, tags=None, d2=None):
    """rslo_map_nearest: the exact nearest stored point of every point (fp32 CUDA [P, F >= 3], read in place) under pose
    (float64 CUDA [7]) within max_dist (None: voxel_size; voxel_size None: read from the map, one host read).  Returns
    (tags int64 [P], d2 float64 [P]) -- -1 / -1.0 without a match -- and, with rows=True or an fp32 [P, 4] tensor, the
    matched rows (zeros without a match).  Read-only, no host read."""
    ptr, nbytes = _map_buf(buf)
    src, stride = _rows3(points, "points")
    P = points.shape[0]
    if voxel_size is None:
        voxel_size = map_params(buf)[0]
    if tags is None:
        tags = torch.empty((P,), dtype=torch.int64, device=points.device)
    if d2 is None:
        d2 = torch.empty((P,), dtype=torch.float64, device=points.device)
    if rows is True:
        rows = torch.empty((P, 4), dtype=torch.float32, device=points.device)
    if tags.shape != (P,) or d2.shape != (P,) or (rows is not None and rows.shape != (P, 4)):
        raise RsloHipError("map_nearest: tags and d2 must be [P], rows [P, 4]")
    _chk(lib().rslo_map_nearest(ptr, nbytes, float(voxel_size), src, stride, P, _pose7(pose, "map_nearest"),
                                float(voxel_size if max_dist is None else max_dist), int(min_hits),
                                _ptr(tags, torch.int64, "tags"), _ptr(d2, torch.float64, "d2"),
                                _ptr(rows, torch.float32, "rows"), _stream()), "rslo_map_nearest")
    return (tags, d2) if rows is None else (tags, d2, rows)


def map_register_ws(n_points, device):
    """a workspace for map_normal_eq / map_register over up to n_points points"""
    return torch.empty((int(lib().rslo_map_register_ws_bytes(int(n_points))) // 8,), dtype=torch.int64, device=device)


def _register_ws(family, ws, P, device):
    """the workspace of a normal_eq / register call of the "map" or the "surfel" family: the caller's, or a new one"""
    if ws is None:
        return (map_register_ws if family == "map" else surfel_register_ws)(P, device)
    if not (ws.is_cuda and ws.is_contiguous()):
        raise RsloHipError("%s: the workspace must be a contiguous CUDA tensor" % family)
    return ws


def _gn_args(name, buf, points, voxel_size, max_dist, result, ws, iters=None):
    """What the normal_eq and register wrappers of both map families do before their call: -> (head, P, max_dist,
    result, ws) with head = (map pointer, map bytes, voxel size, points pointer, stride in floats) and result the [29] sums
    (iters None) or the [iters, 8] info rows, the caller's or a new tensor.  voxel_size None is read from a voxel map."""
    family = name.split("_")[0]
    ptr, nbytes = _map_buf(buf)
    src, stride = _rows3(points, "points")
    P = points.shape[0]
    if voxel_size is None and family == "map":
        voxel_size = map_params(buf)[0]
    shape, what = ((29,), "out must be [29]") if iters is None else ((iters, 8), "info must be [iters, 8]")
    if result is None:
        result = torch.empty(tuple(max(n, 0) for n in shape), dtype=torch.float64, device=points.device)
    if result.shape != shape:
        raise RsloHipError("%s: %s" % (name, what))
    ws = _register_ws(family, ws, P, points.device)
    return ((ptr, nbytes, float(voxel_size), src, stride), P, float(voxel_size if max_dist is None else max_dist), result, ws)


def _gn_tail(result, what, ws):
    """the last four arguments of those calls: the result, the workspace and its bytes, the stream"""
    return _ptr(result, torch.float64, what), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()


def map_normal_eq(buf, points, pose, voxel_size=None, metric="plane", max_dist=None, min_hits=1, out=None, ws=None,
                  robust_scale=None):
    """rslo_map_normal_eq: out float64 CUDA [29] = the upper triangle of H (21), g (6), cost, pairs at pose, over the
    matches of map_nearest.  metric "plane" reads the normals at columns 4..6 of points.  No host read.
    robust_scale (not None): rslo_map_normal_eq_w, every matched point's addends times its Geman-McClure weight
    (0.0: no weights, the bits of rslo_map_normal_eq)."""
    head, P, max_dist, out, ws = _gn_args("map_normal_eq", buf, points, voxel_size, max_dist, out, ws)
    sym = "map_normal_eq" if robust_scale is None else "map_normal_eq_w"
    args = [*head, int(points.shape[1]), P, _pose7(pose, sym), _map_metric(metric), max_dist, int(min_hits)]
    if robust_scale is not None:
        args.append(float(robust_scale))
    _chk(getattr(lib(), "rslo_" + sym)(*args, *_gn_tail(out, "out", ws)), "rslo_" + sym)
    return out


def map_register(buf, points, pose, voxel_size=None, iters=5, metric="plane", max_dist=None, min_hits=1, damping=0.0,
                 min_pairs=50, tol_t=0.0, tol_r=0.0, info=None, ws=None, robust_scale=None):
    """rslo_map_register: `iters` Gauss-Newton iterations of points against the map; pose (float64 CUDA [7]) is updated
    IN PLACE.  Returns info float64 CUDA [iters, 8]: rows {status, pairs, cost, |dt|, theta, 0, 0, 0}, status 0 step taken, 1
    too few pairs, 2 not positive definite, 3 skipped after convergence.  No host read, a fixed number of launches: capturable.
    robust_scale (not None): rslo_map_register_w, Geman-McClure weights of that scale (0.0: no weights, the same bits)."""
    iters = int(iters)
    head, P, max_dist, info, ws = _gn_args("map_register", buf, points, voxel_size, max_dist, info, ws, iters)
    sym = "map_register" if robust_scale is None else "map_register_w"
    args = [*head, int(points.shape[1]), P, _pose7(pose, sym), iters, _map_metric(metric), max_dist, int(min_hits),
            float(damping), int(min_pairs), float(tol_t), float(tol_r)]
    if robust_scale is not None:
        args.append(float(robust_scale))
    _chk(getattr(lib(), "rslo_" + sym)(*args, *_gn_tail(info, "info", ws)), "rslo_" + sym)
    return info


def map_register_sched(bufs, voxel_sizes, stages, points, pose, metric="plane", min_hits=1, damping=0.0, min_pairs=50,
                       tol_t=0.0, tol_r=0.0, info=None, ws=None):
    """rslo_map_register_sched: the stages (rows of (level, iters, max_dist, robust_scale), host numbers) run in order
    on pose (float64 CUDA [7], updated IN PLACE), each against bufs[level] with cell edge voxel_sizes[level].  Returns
    info float64 CUDA [sum of iters, 8]: rows {status, pairs, cost, |dt|, theta, stage, level, 0}.  The arrays are read at
    enqueue time; no host read of the device, a number of launches fixed by the schedule: capturable."""
    src, stride = _rows3(points, "points")
    P = points.shape[0]
    L = len(bufs)
    if L < 1 or len(voxel_sizes) != L:
        raise RsloHipError("map_register_sched: one voxel size per map, and at least one map")
    ptrs = [_map_buf(b) for b in bufs]
    maps = (C.c_void_p * L)(*[p for p, _ in ptrs])
    nbytes = (C.c_size_t * L)(*[n for _, n in ptrs])
    voxels = (C.c_double * L)(*[float(v) for v in voxel_sizes])
    rows = [tuple(float(v) for v in st) for st in stages]
    if any(len(r) != 4 for r in rows):
        raise RsloHipError("map_register_sched: a stage is (level, iters, max_dist, robust_scale)")
    flat = (C.c_double * (4 * len(rows)))(*[v for r in rows for v in r])
    total = sum(int(r[1]) for r in rows if r[1] == r[1] and abs(r[1]) < 1e9)      # (the library refuses what is not an integer >= 1)
    if info is None:
        info = torch.empty((max(total, 0), 8), dtype=torch.float64, device=points.device)
    if info.shape != (total, 8):
        raise RsloHipError("map_register_sched: info must be [sum of iters, 8] = [%d, 8]" % total)
    ws = _register_ws("map", ws, P, points.device)
    _chk(lib().rslo_map_register_sched(maps, nbytes, voxels, L, flat, len(rows), src, stride, int(points.shape[1]), P,
                                       _pose7(pose, "map_register_sched"), _map_metric(metric), int(min_hits),
                                       float(damping), int(min_pairs), float(tol_t), float(tol_r),
                                       _ptr(info, torch.float64, "info"), ws.data_ptr(), ws.numel() * ws.element_size(),
                                       _stream()), "rslo_map_register_sched")
    return info


# --------------------------------------------------------------------------------------
# surfel map (csrc/surfel.hip; rules: include/rslo_hip.h "Surfel map"); the owning class is rslo_amd/surfels.py SurfelMap
# --------------------------------------------------------------------------------------
SURFEL_HDR_COUNTERS = 8   # first int64 word of the seven counters in a surfel map's header
SURFEL_COUNTERS = ("n_scans", "n_cells", "n_points", "dropped_invalid", "dropped_range", "dropped_full", "n_planar")


def surfel_bytes(capacity):
    """rslo_surfel_bytes: bytes of a surfel map of `capacity` slots, 0 unless capacity is a power of two >= 1024."""
    return int(lib().rslo_surfel_bytes(int(capacity)))


def surfel_insert_ws(n_points, device):
    """a workspace for surfel_insert of up to n_points points"""
    return torch.empty((int(lib().rslo_surfel_insert_ws_bytes(int(n_points))),), dtype=torch.uint8, device=device)


def surfel_register_ws(n_points, device):
    """a workspace for surfel_normal_eq / surfel_register over up to n_points points"""
    return torch.empty((int(lib().rslo_surfel_register_ws_bytes(int(n_points))) // 8,), dtype=torch.int64, device=device)


def surfel_reset(buf, capacity, voxel_size, min_range=0.0, max_range=float("inf"), min_points=5, planar_ratio=0.1,
                 line_ratio=0.05):
    """rslo_surfel_reset on the current stream: empties the table and writes the header."""
    ptr, nbytes = _map_buf(buf)
    _chk(lib().rslo_surfel_reset(ptr, nbytes, int(capacity), float(voxel_size), float(min_range), float(max_range),
                                 int(min_points), float(planar_ratio), float(line_ratio), _stream()), "rslo_surfel_reset")


def surfel_insert(buf, points, pose, ws):
    """rslo_surfel_insert: one scan (fp32 CUDA [P, F >= 3], read in place, only x y z are read) under pose (float64 CUDA
    [7]) on the current stream.  ws: >= rslo_surfel_insert_ws_bytes(P) bytes.  Three launches, no host read."""
    ptr, nbytes = _map_buf(buf)
    src, stride = _rows3(points, "points")
    _chk(lib().rslo_surfel_insert(ptr, nbytes, src, stride, int(points.shape[0]), _pose7(pose, "surfel_insert"), _ptr(ws),
                                  ws.numel() * ws.element_size(), _stream()), "rslo_surfel_insert")


def surfel_insert_frames(buf, store_buf, capacity, K, poses):
    """rslo_surfel_insert_frames: every frame of the keyframe store store_buf under its own row of poses (float64 CUDA
    [n, 7], contiguous), as n successive surfel_insert calls would leave the table.  Three launches, no host read."""
    _insert_frames("surfel_insert_frames", buf, store_buf, capacity, K, poses)


def surfel_export(buf, min_flag=1, center=None, radius=0.0, keys=None, moments=None, rows=None, counts=None):
    """rslo_surfel_export into preallocated keys int64 [R], moments int64 [R, 10], rows float64 [R, 8] (all None: R = 0,
    count only); center: None or float64 CUDA [3].  Returns counts, int64 CUDA [2] = {matching, written}.  No host read."""
    ptr, nbytes = _map_buf(buf)
    R = 0 if keys is None else keys.shape[0]
    if R and (keys.shape != (R,) or moments is None or rows is None or moments.shape != (R, 10) or rows.shape != (R, 8)):
        raise RsloHipError("surfel_export: keys [R], moments [R, 10] and rows [R, 8] go together")
    cptr = _center3("surfel_export", center, exact=True)
    if counts is None:
        counts = torch.empty((2,), dtype=torch.int64, device=buf.device)
    _chk(lib().rslo_surfel_export(ptr, nbytes, int(min_flag), cptr, float(radius),
                                  _ptr(keys, torch.int64, "keys") if R else None,
                                  _ptr(moments, torch.int64, "moments") if R else None,
                                  _ptr(rows, torch.float64, "rows") if R else None, R,
                                  _ptr(counts, torch.int64, "counts"), _stream()), "rslo_surfel_export")
    return counts


SURFEL_HDR_PRUNE = 15     # first int64 word of n_prunes, n_evicted, n_lost in a surfel map's header
SURFEL_PRUNE_COUNTERS = ("n_prunes", "n_evicted", "n_lost")


def surfel_prune_ws(capacity, device):
    """a workspace for surfel_prune on a map of `capacity` slots: rslo_surfel_prune_ws_bytes(capacity) bytes"""
    return _prune_ws("surfel_prune_ws", capacity, device)


def surfel_prune(buf, ws, center=None, radius=0.0, inner_radius=0.0, min_count=1):
    """rslo_surfel_prune on the current stream: evict the cells whose centre is not within radius of center (None: no
    such test; else float64 CUDA, contiguous, >= 3 elements, read in place: a [7] trajectory row will do) or that hold
    fewer than min_count points and lie at least inner_radius from it, by rebuilding the table through ws
    (surfel_prune_ws).  Five launches, no host read."""
    ptr, nbytes = _map_buf(buf)
    cptr = _center3("surfel_prune", center, exact=False)
    if not (torch.is_tensor(ws) and ws.is_cuda and ws.is_contiguous()):
        raise RsloHipError("surfel_prune: ws must be a contiguous CUDA tensor (surfel_prune_ws)")
    _chk(lib().rslo_surfel_prune(ptr, nbytes, cptr, float(radius),
                                 float(inner_radius), int(min_count), ws.data_ptr(), ws.numel() * ws.element_size(),
                                 _stream()), "rslo_surfel_prune")


def surfel_nearest(buf, points, pose, voxel_size, max_dist=None, rows=None, keys=None, d2=None):
    """rslo_surfel_nearest: the planar cell whose mean is nearest to every point (fp32 CUDA [P, F >= 3]) under pose within
    max_dist (None: voxel_size).  Returns (keys int64 [P], d2 float64 [P]) -- -1 / -1.0 without a match -- and, with
    rows=True or a float64 [P, 8] tensor, the matched rows (zeros without a match).  Read-only, no host read."""
    ptr, nbytes = _map_buf(buf)
    src, stride = _rows3(points, "points")
    P = points.shape[0]
    if keys is None:
        keys = torch.empty((P,), dtype=torch.int64, device=points.device)
    if d2 is None:
        d2 = torch.empty((P,), dtype=torch.float64, device=points.device)
    if rows is True:
        rows = torch.empty((P, 8), dtype=torch.float64, device=points.device)
    if keys.shape != (P,) or d2.shape != (P,) or (rows is not None and rows.shape != (P, 8)):
        raise RsloHipError("surfel_nearest: keys and d2 must be [P], rows [P, 8]")
    _chk(lib().rslo_surfel_nearest(ptr, nbytes, float(voxel_size), src, stride, P, _pose7(pose, "surfel_nearest"),
                                   float(voxel_size if max_dist is None else max_dist), _ptr(keys, torch.int64, "keys"),
                                   _ptr(d2, torch.float64, "d2"), _ptr(rows, torch.float64, "rows"), _stream()),
         "rslo_surfel_nearest")
    return (keys, d2) if rows is None else (keys, d2, rows)


def surfel_normal_eq(buf, points, pose, voxel_size, max_dist=None, robust_scale=0.0, out=None, ws=None):
    """rslo_surfel_normal_eq: out float64 CUDA [29] = the upper triangle of H (21), g (6), cost, pairs of the plane terms
    of the matches of surfel_nearest at pose; robust_scale > 0: Geman-McClure weights.  No host read."""
    head, P, max_dist, out, ws = _gn_args("surfel_normal_eq", buf, points, voxel_size, max_dist, out, ws)
    _chk(lib().rslo_surfel_normal_eq(*head, P, _pose7(pose, "surfel_normal_eq"), max_dist, float(robust_scale),
                                     *_gn_tail(out, "out", ws)), "rslo_surfel_normal_eq")
    return out


def surfel_register(buf, points, pose, voxel_size, iters=4, max_dist=None, damping=0.0, min_pairs=50, tol_t=0.0, tol_r=0.0,
                    robust_scale=0.0, info=None, ws=None):
    """rslo_surfel_register: `iters` Gauss-Newton iterations of points against the surfel map; pose (float64 CUDA [7]) is
    updated IN PLACE.  Returns info float64 CUDA [iters, 8]: rows {status, pairs, cost, |dt|, theta, 0, 0, 0}, statuses
    as map_register.  No host read, a fixed number of launches: capturable."""
    iters = int(iters)
    head, P, max_dist, info, ws = _gn_args("surfel_register", buf, points, voxel_size, max_dist, info, ws, iters)
    _chk(lib().rslo_surfel_register(*head, P, _pose7(pose, "surfel_register"), iters, max_dist, float(damping),
                                    int(min_pairs), float(tol_t), float(tol_r), float(robust_scale),
                                    *_gn_tail(info, "info", ws)), "rslo_surfel_register")
    return info


def surfel_nearest_d(buf, points, pose, voxel_size, max_dist=None, min_flag=1, reg_rel=0.01, reg_abs=0.02, rows=None,
                     info=None, keys=None, d2=None):
    """rslo_surfel_nearest_d: surfel_nearest among the cells with flag >= min_flag (1 or 2).  Returns (keys, d2[, rows]
    [, info]): with info=True or a float64 [P, 8] tensor, the rows {M00, M01, M02, M11, M12, M22, det, lam} of the matched
    cells' information matrices (include/rslo_hip.h "Distribution cost"), zeros without a match.  Read-only, no host read."""
    ptr, nbytes = _map_buf(buf)
    src, stride = _rows3(points, "points")
    P = points.shape[0]
    if keys is None:
        keys = torch.empty((P,), dtype=torch.int64, device=points.device)
    if d2 is None:
        d2 = torch.empty((P,), dtype=torch.float64, device=points.device)
    if rows is True:
        rows = torch.empty((P, 8), dtype=torch.float64, device=points.device)
    if info is True:
        info = torch.empty((P, 8), dtype=torch.float64, device=points.device)
    if keys.shape != (P,) or d2.shape != (P,) or any(t is not None and t.shape != (P, 8) for t in (rows, info)):
        raise RsloHipError("surfel_nearest_d: keys and d2 must be [P], rows and info [P, 8]")
    _chk(lib().rslo_surfel_nearest_d(ptr, nbytes, float(voxel_size), src, stride, P, _pose7(pose, "surfel_nearest_d"),
                                     float(voxel_size if max_dist is None else max_dist), int(min_flag), float(reg_rel),
                                     float(reg_abs), _ptr(keys, torch.int64, "keys"), _ptr(d2, torch.float64, "d2"),
                                     _ptr(rows, torch.float64, "rows"), _ptr(info, torch.float64, "info"), _stream()),
         "rslo_surfel_nearest_d")
    return (keys, d2) + tuple(t for t in (rows, info) if t is not None)


def surfel_normal_eq_d(buf, points, pose, voxel_size, max_dist=None, min_flag=1, reg_rel=0.01, reg_abs=0.02,
                       robust_scale=0.0, out=None, ws=None):
    """rslo_surfel_normal_eq_d: out float64 CUDA [29] = the upper triangle of H (21), g (6), cost, pairs of the
    distribution terms of the matches of surfel_nearest_d at pose; robust_scale > 0 (in sigmas): Geman-McClure weights.
    No host read."""
    head, P, max_dist, out, ws = _gn_args("surfel_normal_eq_d", buf, points, voxel_size, max_dist, out, ws)
    _chk(lib().rslo_surfel_normal_eq_d(*head, P, _pose7(pose, "surfel_normal_eq_d"), max_dist, int(min_flag), float(reg_rel),
                                       float(reg_abs), float(robust_scale), *_gn_tail(out, "out", ws)),
         "rslo_surfel_normal_eq_d")
    return out


def surfel_register_d(buf, points, pose, voxel_size, iters=4, max_dist=None, damping=0.0, min_pairs=50, tol_t=0.0,
                      tol_r=0.0, robust_scale=0.0, min_flag=1, reg_rel=0.01, reg_abs=0.02, info=None, ws=None):
    """rslo_surfel_register_d: surfel_register with the distribution cost: pose (float64 CUDA [7]) is updated IN PLACE.
    Returns info float64 CUDA [iters, 8] as surfel_register.  No host read, a fixed number of launches: capturable."""
    iters = int(iters)
    head, P, max_dist, info, ws = _gn_args("surfel_register_d", buf, points, voxel_size, max_dist, info, ws, iters)
    _chk(lib().rslo_surfel_register_d(*head, P, _pose7(pose, "surfel_register_d"), iters, max_dist, float(damping),
                                      int(min_pairs), float(tol_t), float(tol_r), float(robust_scale), int(min_flag),
                                      float(reg_rel), float(reg_abs), *_gn_tail(info, "info", ws)), "rslo_surfel_register_d")
    return info


def _rows_of(t, name):
    """(pointer, stride in floats) of an fp32 CUDA [N, F] tensor whose rows are contiguous and evenly spaced"""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2
            and (t.shape[1] == 0 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])):
        raise RsloHipError("%s must be an fp32 CUDA [N, F] tensor with contiguous rows" % name)
    return t.data_ptr(), int(t.stride(0)) if t.shape[0] > 1 else int(max(t.stride(0), t.shape[1]))


def deskew(points, out, times=None, rel7=None, pose_a=None, pose_b=None, stamp=0.5, az_start_turn=-0.5, az_clockwise=False,
           max_angle=1.5707963267948966, normal_col=-1, motion_out=None):
    """rslo_deskew on the current stream: the rows of points (fp32 CUDA [N, F], rows contiguous, any row stride) moved to
    the sensor frame at sweep fraction `stamp` into out (the same shape; may be points itself).  times: fp32 CUDA [N]
    sweep fractions, or None: from the azimuth.  Motion: rel7 (fp32 CUDA [7]), or pose_a and pose_b (float64 CUDA [7]
    each: A^-1 o B), or none of them (a copy).  motion_out: float64 CUDA [8] or None.  One launch, no host read."""
    src, stride = _rows_of(points, "deskew: points")
    dst, ostride = _rows_of(out, "deskew: out")
    if out.shape != points.shape or out.device != points.device:
        raise RsloHipError("deskew: out must have the shape and the device of points")
    N, F = points.shape
    if times is not None and not (torch.is_tensor(times) and times.is_cuda and times.dtype == torch.float32
                                  and times.shape == (N,) and times.is_contiguous()):
        raise RsloHipError("deskew: times must be a contiguous fp32 CUDA [N] tensor")
    if rel7 is not None and not (torch.is_tensor(rel7) and rel7.is_cuda and rel7.dtype == torch.float32
                                 and rel7.numel() == 7 and rel7.is_contiguous()):
        raise RsloHipError("deskew: rel7 must be 7 contiguous fp32 values on the GPU")
    if motion_out is not None and not (torch.is_tensor(motion_out) and motion_out.is_cuda and motion_out.shape == (8,)
                                       and motion_out.dtype == torch.float64 and motion_out.is_contiguous()):
        raise RsloHipError("deskew: motion_out must be a contiguous float64 CUDA [8] tensor")
    _chk(lib().rslo_deskew(src if N else None, stride, N, F, int(normal_col), _dp(times), _dp(rel7),
                           None if pose_a is None else _pose7(pose_a, "deskew"),
                           None if pose_b is None else _pose7(pose_b, "deskew"), float(stamp), float(az_start_turn),
                           int(bool(az_clockwise)), float(max_angle), dst if N else None, ostride, _dp(motion_out), _stream()),
         "rslo_deskew")
    return out


def chamfer_grad(xyz1, xyz2, graddist1, idx1, g1=None, g2=None):
    B, N, _ = xyz1.shape
    M = xyz2.shape[1]
    if g1 is None:
        g1 = torch.empty_like(xyz1)
    if g2 is None:
        g2 = torch.empty_like(xyz2)
    _chk(lib().rslo_chamfer_grad(_ptr(xyz1, torch.float32, "xyz1"), _ptr(xyz2, torch.float32, "xyz2"), B, N, M,
                                 _ptr(graddist1, torch.float32, "graddist1"), _ptr(idx1, torch.int32, "idx1"),
                                 _ptr(g1), _ptr(g2), _stream()), "rslo_chamfer_grad")
    return g1, g2


# --------------------------------------------------------------------------------------
# consistency loss
# --------------------------------------------------------------------------------------
def cov_residual_fwd(p1, tgt, cov1, cov2, idx, dist, thr, Rd, reg_weight):
    """-> loss [B], cnt [B] (see include/rslo_hip.h)."""
    B, N, _ = p1.shape
    M = tgt.shape[1]
    dev = p1.device
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    cnt = torch.empty((B,), dtype=torch.float32, device=dev)
    wsb = lib().rslo_cov_residual_ws_bytes(B, N)
    ws = _ws(wsb, dev)
    _chk(lib().rslo_cov_residual_fwd(_ptr(p1, torch.float32, "p1"), _ptr(tgt, torch.float32, "tgt"),
                                     _ptr(cov1, torch.float32, "cov1"), _ptr(cov2, torch.float32, "cov2"),
                                     _ptr(idx, torch.int32, "idx"), _ptr(dist, torch.float32, "dist"),
                                     _ptr(thr, torch.float32, "thr"), _ptr(Rd, torch.float32, "Rd"), B, N, M,
                                     float(reg_weight), _ptr(ws), wsb, _ptr(loss), _ptr(cnt), _stream()),
         "rslo_cov_residual_fwd")
    return loss, cnt


_resid_bwd_ws = {}


def cov_residual_bwd(p1, tgt, cov1, cov2, idx, dist, thr, Rd, gloss, cnt, reg_weight, need_gp1=False):
    B, N, _ = p1.shape
    M = tgt.shape[1]
    gp1 = torch.empty_like(p1) if need_gp1 else None
    gtgt = torch.empty_like(tgt)
    gcov1 = torch.empty_like(cov1)
    gcov2 = torch.empty_like(cov2)
    key = (B, N, M)
    wsb = _resid_bwd_ws.get(key)
    if wsb is None:
        wsb = _resid_bwd_ws[key] = lib().rslo_cov_residual_bwd_ws_bytes(B, N, M)
    ws = _ws(wsb, p1.device)
    _chk(lib().rslo_cov_residual_bwd(_ptr(p1, torch.float32, "p1"), _ptr(tgt, torch.float32, "tgt"),
                                     _ptr(cov1, torch.float32, "cov1"), _ptr(cov2, torch.float32, "cov2"),
                                     _ptr(idx, torch.int32, "idx"), _ptr(dist, torch.float32, "dist"),
                                     _ptr(thr, torch.float32, "thr"), _ptr(Rd, torch.float32, "Rd"),
                                     _ptr(gloss, torch.float32, "gloss"), _ptr(cnt, torch.float32, "cnt"), B, N, M,
                                     float(reg_weight), _ptr(gp1), _ptr(gtgt), _ptr(gcov1), _ptr(gcov2), _ptr(ws), wsb,
                                     _stream()),
         "rslo_cov_residual_bwd")
    return gp1, gtgt, gcov1, gcov2


def icp_step(p1, n1, tgt, idx, dist, thr, res_r, res_t, first=False):
    """One Kabsch refinement over the ROI; composes res_r [B,3,3] / res_t [B,3] IN PLACE.
    first: the running motion is the identity -- res_r / res_t are written without being read (no fill by the caller)."""
    B, N, _ = p1.shape
    M = tgt.shape[1]
    wsb = lib().rslo_icp_ws_bytes(B, N)
    ws = _ws(wsb, p1.device)
    entry = "rslo_icp_step_first" if first else "rslo_icp_step"
    _chk(getattr(lib(), entry)(_ptr(p1, torch.float32, "p1"), _ptr(n1, torch.float32, "n1"),
                               _ptr(tgt, torch.float32, "tgt"), _ptr(idx, torch.int32, "idx"),
                               _ptr(dist, torch.float32, "dist"), _ptr(thr, torch.float32, "thr"), B, N, M, _ptr(ws), wsb,
                               _ptr(res_r, torch.float32, "res_r"), _ptr(res_t, torch.float32, "res_t"), None, None,
                               _stream()), entry)


def transform_points(x, R, t):
    B, M, _ = x.shape
    out = torch.empty_like(x)
    _chk(lib().rslo_transform_points(_ptr(x, torch.float32, "x"), _ptr(R, torch.float32, "R"),
                                     _ptr(t, torch.float32, "t"), B, M, _ptr(out), _stream()), "rslo_transform_points")
    return out


# --------------------------------------------------------------------------------------
# pyramid supervision
# --------------------------------------------------------------------------------------
class _PyramidLevel(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("mask", C.c_void_p), ("dpred", C.c_void_p),
                ("h", C.c_int32), ("w", C.c_int32), ("mask_channels", C.c_int32)]


_py_done = {}


def _pyramid_levels(preds, masks, dpreds=None):
    B = preds[0].shape[0]
    arr = (_PyramidLevel * len(preds))()
    for l, (p, m) in enumerate(zip(preds, masks)):
        if p.dim() != 4 or p.shape[1] != 7 or m.shape[0] != B or p.shape[0] != B or m.shape[2:] != p.shape[2:]:
            raise RsloHipError("pyramid_l2: level %d pred %s / mask %s" % (l, tuple(p.shape), tuple(m.shape)))
        arr[l].pred = _ptr(p, torch.float32, "pred")
        arr[l].mask = _ptr(m, torch.float32, "mask")
        arr[l].dpred = _ptr(dpreds[l], torch.float32, "dpred") if dpreds is not None else None
        arr[l].h, arr[l].w, arr[l].mask_channels = p.shape[2], p.shape[3], m.shape[1]
    return arr, B


def pyramid_l2_fwd(preds, masks, tq, H0, W0, origin, vsize):
    """preds[l] [B,7,h,w], masks[l] [B,Cm,h,w], tq [B,7] -> (loss_b [L,B,2], den [L,B,2])."""
    arr, B = _pyramid_levels(preds, masks)
    dev = tq.device
    L = len(preds)
    done = _py_done.get(dev)
    if done is None or done.numel() < L * B:
        done = _py_done[dev] = torch.zeros((max(L * B, 64),), dtype=torch.int32, device=dev)
    wsb = lib().rslo_pyramid_l2_ws_bytes(arr, L, B)
    ws = _ws(wsb, dev)
    loss_b = torch.empty((L, B, 2), dtype=torch.float32, device=dev)
    den = torch.empty((L, B, 2), dtype=torch.float32, device=dev)
    _chk(lib().rslo_pyramid_l2_fwd(arr, L, B, _ptr(tq, torch.float32, "tq"), int(H0), int(W0),
                                   _F3(*[float(v) for v in origin]), _F3(*[float(v) for v in vsize]), _ptr(ws), wsb,
                                   _ptr(done), _ptr(loss_b), _ptr(den), _stream()), "rslo_pyramid_l2_fwd")
    return loss_b, den


def pyramid_l2_bwd(preds, masks, tq, H0, W0, origin, vsize, grad_loss_b, den):
    dpreds = [torch.empty_like(p) for p in preds]
    arr, B = _pyramid_levels(preds, masks, dpreds)
    _chk(lib().rslo_pyramid_l2_bwd(arr, len(preds), B, _ptr(tq, torch.float32, "tq"), int(H0), int(W0),
                                   _F3(*[float(v) for v in origin]), _F3(*[float(v) for v in vsize]),
                                   _ptr(grad_loss_b, torch.float32, "grad"), _ptr(den, torch.float32, "den"),
                                   _stream()), "rslo_pyramid_l2_bwd")
    return dpreds


class HeadMasks(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("conf", C.c_void_p), ("tq", C.c_void_p), ("tq_g", C.c_void_p),
                ("pred", C.c_void_p * 3), ("w", C.c_void_p * 4), ("occ", C.c_void_p * 4), ("mpred", C.c_void_p * 3),
                ("mtq", C.c_void_p), ("mtq_g", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("levels", C.c_int32)]


class HeadMasksBwd(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("occ", C.c_void_p * 4), ("g_mpred", C.c_void_p * 3), ("g_mtq", C.c_void_p),
                ("d_pred", C.c_void_p * 3), ("d_tq", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("levels", C.c_int32)]


def tq_normalize_fwd(tq):
    B, _, H, W = tq.shape
    out = torch.empty_like(tq)
    _chk(lib().rslo_tq_normalize_fwd(_ptr(tq, torch.float32, "tq"), B, H * W, _ptr(out), _stream()), "rslo_tq_normalize_fwd")
    return out


def tq_normalize_bwd(tq, g):
    B, _, H, W = tq.shape
    d = torch.empty_like(tq)
    _chk(lib().rslo_tq_normalize_bwd(_ptr(tq, torch.float32, "tq"), _ptr(g, torch.float32, "grad"), B, H * W, _ptr(d),
                                     _stream()), "rslo_tq_normalize_bwd")
    return d


def conf_softmax_fwd(t_logit, r_logit, outside, temperature):
    """t_logit, r_logit [B,1,H,W] fp32, outside [B,1,H,W] bool -> (t_conf, r_conf [B,1,H,W], conf_temp [B,2,H,W])."""
    B, _, H, W = t_logit.shape
    t_conf, r_conf = torch.empty_like(t_logit), torch.empty_like(r_logit)
    ct = torch.empty((B, 2, H, W), dtype=torch.float32, device=t_logit.device)
    _chk(lib().rslo_conf_softmax_fwd(_ptr(t_logit, torch.float32, "t_logit"), _ptr(r_logit, torch.float32, "r_logit"),
                                     _ptr(outside, torch.bool, "outside"), B, H * W, float(temperature), _ptr(t_conf),
                                     _ptr(r_conf), _ptr(ct), _stream()), "rslo_conf_softmax_fwd")
    return t_conf, r_conf, ct


def conf_softmax_bwd(t_conf, r_conf, g_t, g_r, outside):
    B, _, H, W = t_conf.shape
    d_t, d_r = torch.empty_like(t_conf), torch.empty_like(r_conf)
    _chk(lib().rslo_conf_softmax_bwd(_ptr(t_conf, torch.float32, "t_conf"), _ptr(r_conf, torch.float32, "r_conf"),
                                     _ptr(g_t, torch.float32, "g_t"), _ptr(g_r, torch.float32, "g_r"),
                                     _ptr(outside, torch.bool, "outside"), B, H * W, _ptr(d_t), _ptr(d_r), _stream()),
         "rslo_conf_softmax_bwd")
    return d_t, d_r


def head_masks_fwd(mask, conf, tq, tq_g, preds):
    """mask [B,1,H,W], conf [B,2,H,W], tq / tq_g [B,7,H,W], preds = [pred of level 1, level 2, ...] (finest first)
    -> (w [levels], occ [levels] (occ[0] = mask), mpreds, mtq, mtq_g)."""
    B, _, H, W = mask.shape
    dev = mask.device
    L = 1 + len(preds)
    a = HeadMasks()
    a.mask, a.conf, a.tq, a.tq_g = _ptr(mask, torch.float32, "mask"), _ptr(conf, torch.float32, "conf"), \
        _ptr(tq, torch.float32, "tq"), _ptr(tq_g, torch.float32, "tq_g")
    w, occ, mp = [], [mask], []
    for k in range(L):
        wk = torch.empty((B, 2, H >> k, W >> k), dtype=torch.float32, device=dev)
        w.append(wk)
        a.w[k] = wk.data_ptr()
        if k:
            ok = torch.empty((B, 1, H >> k, W >> k), dtype=torch.float32, device=dev)
            occ.append(ok)
            a.occ[k] = ok.data_ptr()
            a.pred[k - 1] = _ptr(preds[k - 1], torch.float32, "pred")
            m = torch.empty_like(preds[k - 1])
            mp.append(m)
            a.mpred[k - 1] = m.data_ptr()
    mtq, mtq_g = torch.empty_like(tq), torch.empty_like(tq_g)
    a.mtq, a.mtq_g = mtq.data_ptr(), mtq_g.data_ptr()
    a.B, a.H, a.W, a.levels = B, H, W, L
    _chk(lib().rslo_head_masks_fwd(C.byref(a), _stream()), "rslo_head_masks_fwd")
    return w, occ, mp, mtq, mtq_g


def head_masks_bwd(mask, occ, g_mpreds, g_mtq, pred_shapes):
    B, _, H, W = mask.shape
    dev = mask.device
    L = len(occ)
    a = HeadMasksBwd()
    a.mask = mask.data_ptr()
    a.g_mtq = _dp(g_mtq)
    d_tq = torch.empty((B, 7, H, W), dtype=torch.float32, device=dev)
    a.d_tq = d_tq.data_ptr()
    d_preds = []
    for k in range(1, L):
        a.occ[k] = occ[k].data_ptr()
        a.g_mpred[k - 1] = _dp(g_mpreds[k - 1])
        d = torch.empty(pred_shapes[k - 1], dtype=torch.float32, device=dev)
        d_preds.append(d)
        a.d_pred[k - 1] = d.data_ptr()
    a.B, a.H, a.W, a.levels = B, H, W, L
    _chk(lib().rslo_head_masks_bwd(C.byref(a), _stream()), "rslo_head_masks_bwd")
    return d_preds, d_tq


class LossTail(C.Structure):
    _fields_ = [("t_pred", C.c_void_p), ("t_tgt", C.c_void_p), ("q_pred", C.c_void_p), ("q_tgt", C.c_void_p),
                ("alpha_T", C.c_void_p), ("alpha_R", C.c_void_p), ("pyr_loss_b", C.c_void_p), ("alpha_pT", C.c_void_p),
                ("alpha_pR", C.c_void_p), ("pair_loss", C.c_void_p), ("alpha_C", C.c_void_p), ("B", C.c_int32),
                ("L", C.c_int32), ("n_pairs", C.c_int32), ("reserved", C.c_int32), ("w_T", C.c_float), ("w_R", C.c_float),
                ("w_pT", C.c_float), ("w_pR", C.c_float), ("c_scale", C.c_float), ("level_w", C.c_float * 8)]


def loss_tail_fwd(desc, device):
    out = torch.empty((5,), dtype=torch.float32, device=device)
    _chk(lib().rslo_loss_tail_fwd(C.byref(desc), _ptr(out), _stream()), "rslo_loss_tail_fwd")
    return out


def loss_tail_bwd(desc, grad_out, B, L, n_pairs):
    dev = grad_out.device
    d_t = torch.empty((B, 3), dtype=torch.float32, device=dev)
    d_q = torch.empty((B, 4), dtype=torch.float32, device=dev)
    d_pyr = torch.empty((L, B, 2), dtype=torch.float32, device=dev) if L else None
    d_pair = torch.empty((n_pairs,), dtype=torch.float32, device=dev) if n_pairs else None
    d_alpha = torch.empty((5, 4), dtype=torch.float32, device=dev)      # 16-byte slots (include/rslo_hip.h: stride 4)
    _chk(lib().rslo_loss_tail_bwd(C.byref(desc), _ptr(grad_out, torch.float32, "grad"), _ptr(d_t), _ptr(d_q), _ptr(d_pyr),
                                  _ptr(d_pair), _ptr(d_alpha), _stream()), "rslo_loss_tail_bwd")
    return d_t, d_q, d_pyr, d_pair, d_alpha[:, 0]


def pad_rows_fwd(src, off, length, Lmax):
    """src [N,C] -> [B,Lmax,C]: rows off[b] .. off[b]+len[b] of src, zero padded."""
    N, Cc = src.shape
    B = off.shape[0]
    out = torch.empty((B, Lmax, Cc), dtype=torch.float32, device=src.device)
    _chk(lib().rslo_pad_rows_fwd(_ptr(src, torch.float32, "src"), N, Cc, _ptr(off, torch.int32, "off"),
                                 _ptr(length, torch.int32, "len"), B, int(Lmax), _ptr(out), _stream()), "rslo_pad_rows_fwd")
    return out


def pair_rows_fwd(feats, conf, off, length, Lmax):
    """feats [N,F] (F = 7: xyz, intensity, normal | 6: xyz, normal), conf [N,Cc] -> xyz [B,Lmax,3], nrm [B,Lmax,3],
    cov [B,Lmax,Cc]: rows off[b] .. off[b]+len[b] of both, zero padded, in one launch."""
    N, F = feats.shape
    Cc = conf.shape[1]
    B = off.shape[0]
    dev = feats.device
    xyz = torch.empty((B, Lmax, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((B, Lmax, 3), dtype=torch.float32, device=dev)
    cov = torch.empty((B, Lmax, Cc), dtype=torch.float32, device=dev)
    _chk(lib().rslo_pair_rows_fwd(_ptr(feats, torch.float32, "feats"), N, F, _ptr(conf, torch.float32, "conf"), Cc,
                                  _ptr(off, torch.int32, "off"), _ptr(length, torch.int32, "len"), B, int(Lmax),
                                  _ptr(xyz), _ptr(nrm), _ptr(cov), _stream()), "rslo_pair_rows_fwd")
    return xyz, nrm, cov


def pad_rows_bwd(dout, off, length, N):
    B, Lmax, Cc = dout.shape
    dsrc = torch.empty((N, Cc), dtype=torch.float32, device=dout.device)
    _chk(lib().rslo_pad_rows_bwd(_ptr(dout, torch.float32, "dout"), N, Cc, _ptr(off, torch.int32, "off"),
                                 _ptr(length, torch.int32, "len"), B, int(Lmax), _ptr(dsrc), _stream()), "rslo_pad_rows_bwd")
    return dsrc


def _rows_view(x):
    """[B,M,3] view whose rows are `stride` floats apart inside a contiguous [B,M,C] tensor -> (ptr, stride)."""
    B, M, three = x.shape
    if three != 3 or x.dtype != torch.float32 or not x.is_cuda:
        raise RsloHipError("transform_rows: need a float32 cuda [B,M,3] tensor")
    sb, sm, sc = x.stride()
    if sc != 1 or sb != M * sm or sm < 3:
        x = x.contiguous()
        sm = 3
    return x, C.c_void_p(x.data_ptr()), sm


def transform_rows(x, R, t=None):
    """out[b,j] = R[b] x[b,j] (+ t[b]);  x may be a column slice of a wider row-major tensor."""
    x, ptr, stride = _rows_view(x)
    B, M, _ = x.shape
    out = torch.empty((B, M, 3), dtype=torch.float32, device=x.device)
    _chk(lib().rslo_transform_rows(ptr, stride, _ptr(R, torch.float32, "R"), _ptr(t, torch.float32, "t"), B, M,
                                   _ptr(out), _stream()), "rslo_transform_rows")
    return out


_tr_done = {}


def transform_rows_bwd(x, gout):
    """-> (dR [B,3,3], dt [B,3]) of out = R x + t."""
    x, ptr, stride = _rows_view(x)
    B, M, _ = x.shape
    dev = x.device
    done = _tr_done.get(dev)
    if done is None or done.numel() < B:
        done = _tr_done[dev] = torch.zeros((max(B, 64),), dtype=torch.int32, device=dev)
    wsb = lib().rslo_transform_rows_bwd_ws_bytes(B, M)
    ws = _ws(wsb, dev)
    dR = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    dt = torch.empty((B, 3), dtype=torch.float32, device=dev)
    _chk(lib().rslo_transform_rows_bwd(ptr, stride, _ptr(gout, torch.float32, "gout"), B, M, _ptr(ws), wsb, _ptr(done),
                                       _ptr(dR), _ptr(dt), _stream()), "rslo_transform_rows_bwd")
    return dR, dt


# --------------------------------------------------------------------------------------
# fused (Sync)BatchNorm2d + activation + residual of the dense head
# --------------------------------------------------------------------------------------
_bn_done = {}


def _bn_counters(dev, C_):
    done = _bn_done.get(dev)
    if done is None or done.numel() < C_:
        done = _bn_done[dev] = torch.zeros((max(C_, 512),), dtype=torch.int32, device=dev)
    return done


def bn2d_stats(x):
    """x [N,C,H,W] -> stats [2C+1] float64 (sum, sum of squares per channel, element count)."""
    N, Cc, H, W = x.shape
    dev = x.device
    wsb = lib().rslo_bn2d_ws_bytes(N, Cc, H * W)
    ws = _ws(wsb, dev)
    stats = torch.empty((2 * Cc + 1,), dtype=torch.float64, device=dev)
    _chk(lib().rslo_bn2d_stats(_ptr(x, torch.float32, "x"), N, Cc, H * W, _ptr(ws), wsb, _ptr(_bn_counters(dev, Cc)),
                               _ptr(stats), _stream()), "rslo_bn2d_stats")
    return stats


def bn2d_apply(x, res, stats, gamma, beta, running_mean, running_var, momentum, eps, slope):
    N, Cc, H, W = x.shape
    dev = x.device
    y = torch.empty_like(x)
    mean = torch.empty((Cc,), dtype=torch.float32, device=dev)
    invstd = torch.empty((Cc,), dtype=torch.float32, device=dev)
    _chk(lib().rslo_bn2d_apply(_ptr(x, torch.float32, "x"), _ptr(res, torch.float32, "res"), _ptr(stats, torch.float64),
                               _ptr(gamma, torch.float32, "gamma"), _ptr(beta, torch.float32, "beta"), N, Cc, H * W,
                               float(eps), float(momentum), float(slope), _ptr(running_mean, torch.float32),
                               _ptr(running_var, torch.float32), _ptr(mean), _ptr(invstd), _ptr(y), _stream()),
         "rslo_bn2d_apply")
    return y, mean, invstd


def bn2d_bwd_reduce(dy, y, x, mean, invstd, slope, has_act, want_affine=True):
    N, Cc, H, W = x.shape
    dev = x.device
    wsb = lib().rslo_bn2d_ws_bytes(N, Cc, H * W)
    ws = _ws(wsb, dev)
    red = torch.empty((2 * Cc,), dtype=torch.float64, device=dev)
    dgamma = torch.empty((Cc,), dtype=torch.float32, device=dev) if want_affine else None
    dbeta = torch.empty((Cc,), dtype=torch.float32, device=dev) if want_affine else None
    _chk(lib().rslo_bn2d_bwd_reduce(_ptr(dy, torch.float32, "dy"), _ptr(y, torch.float32, "y"), _ptr(x, torch.float32, "x"),
                                    _ptr(mean), _ptr(invstd), N, Cc, H * W, float(slope), int(has_act), _ptr(ws), wsb,
                                    _ptr(_bn_counters(dev, Cc)), _ptr(red), _ptr(dgamma), _ptr(dbeta), _stream()),
         "rslo_bn2d_bwd_reduce")
    return red, dgamma, dbeta


def bn2d_bwd_apply(dy, y, x, gamma, mean, invstd, red, count, slope, has_act, want_res, count_dev=None):
    N, Cc, H, W = x.shape
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_res else None
    _chk(lib().rslo_bn2d_bwd_apply(_ptr(dy, torch.float32, "dy"), _ptr(y, torch.float32, "y"), _ptr(x, torch.float32, "x"),
                                   _ptr(gamma, torch.float32, "gamma"), _ptr(mean), _ptr(invstd), _ptr(red, torch.float64),
                                   float(count), _ptr(count_dev, torch.float64, "count_dev"), N, Cc, H * W, float(slope),
                                   int(has_act), _ptr(dx), _ptr(dres),
                                   _stream()), "rslo_bn2d_bwd_apply")
    return dx, dres


_bn_ws_bytes = {}


def _bn2d_ws(N, Cc, HW, dev):
    key = (N, Cc, HW)
    n = _bn_ws_bytes.get(key)
    if n is None:
        n = _bn_ws_bytes[key] = lib().rslo_bn2d_ws_bytes(N, Cc, HW)
    return torch.empty((n,), dtype=torch.uint8, device=dev), n


def bn2d_fwd_local(x, res, gamma, beta, running_mean, running_var, momentum, eps, slope):
    """Single-rank y = act(BN_train(x) + res): two launches.  -> y, save_mean, save_invstd.  (Hot host path: x / res are
    checked, everything else comes from module state or is allocated here.)"""
    N, Cc, H, W = x.shape
    dev = x.device
    HW = H * W
    ws, wsb = _bn2d_ws(N, Cc, HW, dev)
    y = torch.empty_like(x)
    stat = torch.empty((2, Cc), dtype=torch.float32, device=dev)
    rc = lib().rslo_bn2d_fwd_local(_ptr(x, torch.float32, "x"), _ptr(res, torch.float32, "res"), _dp(gamma), _dp(beta), N,
                                   Cc, HW, eps, momentum, slope, _dp(running_mean), _dp(running_var), stat.data_ptr(),
                                   stat.data_ptr() + 4 * Cc, y.data_ptr(), ws.data_ptr(), wsb, _stream())
    if rc:
        _chk(rc, "rslo_bn2d_fwd_local")
    return y, stat[0], stat[1]


def bn2d_bwd_local(dy, y, x, gamma, mean, invstd, slope, has_act, want_res, want_affine=True):
    N, Cc, H, W = x.shape
    dev = x.device
    HW = H * W
    ws, wsb = _bn2d_ws(N, Cc, HW, dev)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_res else None
    if want_affine:
        dgb = torch.empty((2, Cc), dtype=torch.float32, device=dev)
        dgamma, dbeta = dgb[0], dgb[1]
        pg, pb = dgb.data_ptr(), dgb.data_ptr() + 4 * Cc
    else:
        dgamma = dbeta = pg = pb = None
    rc = lib().rslo_bn2d_bwd_local(_ptr(dy, torch.float32, "dy"), _dp(y), x.data_ptr(), _dp(gamma), mean.data_ptr(),
                                   invstd.data_ptr(), N, Cc, HW, slope, 1 if has_act else 0, dx.data_ptr(), _dp(dres), pg,
                                   pb, ws.data_ptr(), wsb, _stream())
    if rc:
        _chk(rc, "rslo_bn2d_bwd_local")
    return dx, dres, dgamma, dbeta


_bn_peer_ok = {}


def bn2d_peer_supported(N, Cc, HW):
    key = (N, Cc, HW)
    v = _bn_peer_ok.get(key)
    if v is None:
        v = _bn_peer_ok[key] = bool(lib().rslo_bn2d_peer_supported(N, Cc, HW))
    return v


def bn2d_fwd_peer(comm, x, res, gamma, beta, running_mean, running_var, momentum, eps, slope):
    """Multi-rank y = act(BN_train(x) + res) in ONE launch: the per-channel sums meet the other ranks' inside the kernel
    (rslo_bn2d_fwd_peer; comm = rslo_amd.peer.PeerComm).  -> y, save_mean, save_invstd, count_all (device double [1])."""
    N, Cc, H, W = x.shape
    dev = x.device
    y = torch.empty_like(x)
    stat = torch.empty((2, Cc), dtype=torch.float32, device=dev)
    cnt = torch.empty((1,), dtype=torch.float64, device=dev)
    rc = lib().rslo_bn2d_fwd_peer(comm.handle, _ptr(x, torch.float32, "x"), _ptr(res, torch.float32, "res"), _dp(gamma),
                                  _dp(beta), N, Cc, H * W, eps, momentum, slope, _dp(running_mean), _dp(running_var),
                                  stat.data_ptr(), stat.data_ptr() + 4 * Cc, cnt.data_ptr(), y.data_ptr(), _stream())
    if rc:
        _chk(rc, "rslo_bn2d_fwd_peer")
    return y, stat[0], stat[1], cnt


def bn2d_bwd_peer(comm, dy, y, x, gamma, mean, invstd, count_all, slope, has_act, want_res, want_affine=True):
    N, Cc, H, W = x.shape
    dev = x.device
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_res else None
    if want_affine:
        dgb = torch.empty((2, Cc), dtype=torch.float32, device=dev)
        dgamma, dbeta = dgb[0], dgb[1]
        pg, pb = dgb.data_ptr(), dgb.data_ptr() + 4 * Cc
    else:
        dgamma = dbeta = pg = pb = None
    rc = lib().rslo_bn2d_bwd_peer(comm.handle, _ptr(dy, torch.float32, "dy"), _dp(y), x.data_ptr(), _dp(gamma),
                                  mean.data_ptr(), invstd.data_ptr(), count_all.data_ptr(), N, Cc, H * W, slope,
                                  1 if has_act else 0, dx.data_ptr(), _dp(dres), pg, pb, _stream())
    if rc:
        _chk(rc, "rslo_bn2d_bwd_peer")
    return dx, dres, dgamma, dbeta


def roi_threshold(dist, counts, ratio):
    """dist [B,N] (+inf padded), counts int32 [B] or None -> thr [B] = max(kth(dist_b, 1 + int(cnt_b * ratio)), 1)."""
    B, N = dist.shape
    thr = torch.empty((B,), dtype=torch.float32, device=dist.device)
    _chk(lib().rslo_roi_threshold(_ptr(dist, torch.float32, "dist"), B, N, _ptr(counts, torch.int32, "counts"),
                                  float(ratio), _ptr(thr), _stream()), "rslo_roi_threshold")
    return thr


# --------------------------------------------------------------------------------------
# local -> global + ego-motion vote
# --------------------------------------------------------------------------------------
_vote_done = {}


def vote_fwd(tq_map, t_conf, r_conf, origin, vsize):
    B, _, H, W = tq_map.shape
    dev = tq_map.device
    done = _vote_done.get(dev)
    if done is None or done.numel() < B:
        done = _vote_done[dev] = torch.zeros((max(B, 64),), dtype=torch.int32, device=dev)
    wsb = lib().rslo_vote_ws_bytes(B, H, W)
    ws = _ws(wsb, dev)
    tq_g = torch.empty_like(tq_map)
    odom = torch.empty((B, 7), dtype=torch.float32, device=dev)
    sums = torch.empty((B, 2), dtype=torch.float32, device=dev)
    _chk(lib().rslo_vote_fwd(_ptr(tq_map, torch.float32, "tq_map"), _ptr(t_conf, torch.float32, "t_conf"),
                             _ptr(r_conf, torch.float32, "r_conf"), B, H, W, _F3(*[float(v) for v in origin]),
                             _F3(*[float(v) for v in vsize]), _ptr(ws), wsb, _ptr(done), _ptr(tq_g), _ptr(odom),
                             _ptr(sums), _stream()), "rslo_vote_fwd")
    return tq_g, odom, sums


def vote_bwd(tq_map, t_conf, r_conf, origin, vsize, odom, sums, g_odom):
    B, _, H, W = tq_map.shape
    d_tq = torch.empty_like(tq_map)
    d_tc = torch.empty_like(t_conf)
    d_rc = torch.empty_like(r_conf)
    _chk(lib().rslo_vote_bwd(_ptr(tq_map, torch.float32, "tq_map"), _ptr(t_conf, torch.float32, "t_conf"),
                             _ptr(r_conf, torch.float32, "r_conf"), B, H, W, _F3(*[float(v) for v in origin]),
                             _F3(*[float(v) for v in vsize]), _ptr(odom), _ptr(sums), _ptr(g_odom, torch.float32, "g"),
                             _ptr(d_tq), _ptr(d_tc), _ptr(d_rc), _stream()), "rslo_vote_bwd")
    return d_tq, d_tc, d_rc


# --------------------------------------------------------------------------------------
# dense 3x3 conv2d weight gradient (BEV head)
# --------------------------------------------------------------------------------------
def conv2d_wgrad_supported(cin, cout, H, W, stride):
    return bool(lib().rslo_conv2d_wgrad_supported(int(cin), int(cout), int(H), int(W), int(stride)))


_c2w_ws_bytes = {}


def conv2d_wgrad(x, dout, stride=1, want_bias=False, lp=False):
    """x [B,cin,H,W], dout [B,cout,Ho,Wo] (contiguous NCHW fp32) -> dW [cout,cin,3,3] of a 3x3 / padding-1 conv;
    want_bias (stride 1): -> (dW, dbias [cout]) with the bias gradient from the same pass.  lp: bf16 operands (C4)."""
    B, cin, H, W = x.shape
    cout = dout.shape[1]
    key = (B, cin, cout, H, W, stride)
    wsb = _c2w_ws_bytes.get(key)
    if wsb is None:
        wsb = _c2w_ws_bytes[key] = lib().rslo_conv2d_wgrad_ws_bytes(B, cin, cout, H, W, stride)
    if wsb == 0:
        raise RsloHipError("rslo_conv2d_wgrad: unsupported shape %s -> %s stride %d" % (tuple(x.shape), tuple(dout.shape), stride))
    dev = x.device
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    dW = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=dev)
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if want_bias else None
    fn = lib().rslo_conv2d_wgrad_bf16 if lp else lib().rslo_conv2d_wgrad
    rc = fn(_ptr(x, torch.float32, "x"), _ptr(dout, torch.float32, "dout"), B, cin, cout, H, W,
            stride, dW.data_ptr(), _dp(db), ws.data_ptr(), wsb, _stream())
    if rc:
        _chk(rc, "rslo_conv2d_wgrad")
    _keep_for_reduce(ws)
    return (dW, db) if want_bias else dW


def conv1x1s2_wgrad(x, dout):
    """x [B,cin,H,W], dout [B,cout,Ho,Wo] -> dW [cout,cin,1,1] of a 1x1 / stride-2 / padding-0 conv (rslo_conv1x1s2_wgrad);
    None when the shape is outside the kernel's range (the caller falls back to a batched GEMM)."""
    B, cin, H, W = x.shape
    cout = dout.shape[1]
    key = (B, cin, cout, H, W, "1x1s2")
    wsb = _c2w_ws_bytes.get(key)
    if wsb is None:
        wsb = _c2w_ws_bytes[key] = lib().rslo_conv1x1s2_wgrad_ws_bytes(B, cin, cout, H, W)
    if wsb == 0:
        return None
    ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
    dW = torch.empty((cout, cin, 1, 1), dtype=torch.float32, device=x.device)
    rc = lib().rslo_conv1x1s2_wgrad(_ptr(x, torch.float32, "x"), _ptr(dout, torch.float32, "dout"), B, cin, cout, H, W,
                                    dW.data_ptr(), ws.data_ptr(), wsb, _stream())
    if rc:
        _chk(rc, "rslo_conv1x1s2_wgrad")
    _keep_for_reduce(ws)
    return dW


def conv2d_fwd_supported(cin, cout, H, W):
    return bool(lib().rslo_conv2d_fwd_supported(int(cin), int(cout), int(H), int(W)))


def conv2d_wsplit(w, transpose=False):
    """w [cout,cin,3,3] fp32 -> split-bf16 MFMA operands (int16 tensor) for conv2d_fwd; transpose=True: data gradient."""
    cout, cin = w.shape[0], w.shape[1]
    ws = torch.empty((lib().rslo_conv2d_wsplit_bytes(cin, cout) // 2,), dtype=torch.int16, device=w.device)
    _chk(lib().rslo_conv2d_wsplit(_ptr(w, torch.float32, "w"), cin, cout, 1 if transpose else 0, _ptr(ws), _stream()),
         "rslo_conv2d_wsplit")
    return ws


class Conv2dSplitDesc(C.Structure):
    _fields_ = [("W", C.c_void_p), ("ws_fwd", C.c_void_p), ("ws_dgrad", C.c_void_p), ("cin", C.c_int32),
                ("cout", C.c_int32), ("ntap", C.c_int32), ("reserved", C.c_int32)]


def conv2d_wsplit_many(weights):
    """weights: list of [cout,cin,3,3] (or [cout,cin,1,1]) fp32 CUDA tensors.  Returns (plan, [(ws_fwd, ws_dgrad) per
    layer]); call conv2d_wsplit_run(plan) after every weight update: it refreshes all operands in one launch."""
    dev = weights[0].device
    sizes = [lib().rslo_conv2d_wsplit_bytes(w.shape[1], w.shape[0]) // 2 * (w.shape[2] * w.shape[3]) // 9 for w in weights]
    pool = torch.empty((2 * sum(sizes),), dtype=torch.int16, device=dev)
    views, off = [], 0
    arr = (Conv2dSplitDesc * len(weights))()
    for i, (w, n) in enumerate(zip(weights, sizes)):
        f, t = pool[off:off + n], pool[off + n:off + 2 * n]
        off += 2 * n
        views.append((f, t))
        arr[i] = Conv2dSplitDesc(_ptr(w, torch.float32, "w"), f.data_ptr(), t.data_ptr(), w.shape[1], w.shape[0],
                                 w.shape[2] * w.shape[3], 0)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    table = host.to(dev)
    plan = {"table": table, "n": len(weights), "max": max(int(w.numel()) for w in weights), "pool": pool,
            "ptrs": [w.data_ptr() for w in weights]}
    return plan, views


def conv2d_wsplit_run(plan):
    _chk(lib().rslo_conv2d_wsplit_many(_ptr(plan["table"]), plan["n"], plan["max"], _stream()), "rslo_conv2d_wsplit_many")


def conv2d_fwd_bn(x, ws, bias, scale, shift, cout, residual=None, slope=None, out=None):
    """Eval-mode 3x3 / stride 1 / padding 1 convolution with the folded BatchNorm in its epilogue (rslo_conv2d_fwd_bn):
    act((conv(x) + bias) * scale + shift + residual), slope None = no activation, 0 = ReLU, else LeakyReLU(slope)."""
    B, cin, H, W = x.shape
    if out is None:
        out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    if residual is not None and (tuple(residual.shape) != tuple(out.shape) or not residual.is_contiguous()):
        raise ValueError("conv2d_fwd_bn: residual must be a contiguous %s tensor" % (tuple(out.shape),))
    rc = lib().rslo_conv2d_fwd_bn(_ptr(x, torch.float32, "x"), ws.data_ptr(), _dp(bias), _ptr(scale, torch.float32, "scale"),
                                  _ptr(shift, torch.float32, "shift"), _dp(residual), B, cin, cout, H, W,
                                  0 if slope is None else 1, 0.0 if slope is None else float(slope), out.data_ptr(), _stream())
    if rc:
        _chk(rc, "rslo_conv2d_fwd_bn")
    return out


def conv2d_fwd_s2_bn(x, ws, bias, scale, shift, cout, ksize, residual=None, slope=None):
    """Eval-mode stride-2 convolution (ksize 3 / padding 1 or 1 / padding 0) with the folded BatchNorm, an optional
    residual and activation in its epilogue (rslo_conv2d_fwd_s2_bn); ws from conv2d_wsplit_k(w, False)."""
    B, cin, H, W = x.shape
    out = torch.empty((B, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    if residual is not None and (tuple(residual.shape) != tuple(out.shape) or not residual.is_contiguous()):
        raise ValueError("conv2d_fwd_s2_bn: residual must be a contiguous %s tensor" % (tuple(out.shape),))
    rc = lib().rslo_conv2d_fwd_s2_bn(_ptr(x, torch.float32, "x"), ws.data_ptr(), _dp(bias),
                                     _ptr(scale, torch.float32, "scale"), _ptr(shift, torch.float32, "shift"), _dp(residual),
                                     B, cin, cout, H, W, ksize, 0 if slope is None else 1,
                                     0.0 if slope is None else float(slope), out.data_ptr(), _stream())
    if rc:
        _chk(rc, "rslo_conv2d_fwd_s2_bn")
    return out


class BnFoldDesc(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("mean", C.c_void_p), ("var", C.c_void_p),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("C", C.c_int32), ("eps", C.c_float)]


def bn_fold_many(bns):
    """bns: BatchNorm modules with running statistics (CUDA fp32).  Returns (plan, [(scale, shift) per layer]); every
    bn_fold_run(plan) re-derives scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale for all
    layers in one launch from the LIVE parameter and buffer storage."""
    dev = bns[0].running_mean.device
    sizes = [int(b.running_mean.numel()) for b in bns]
    pool = torch.empty((2 * sum(sizes),), dtype=torch.float32, device=dev)
    arr = (BnFoldDesc * len(bns))()
    views, off = [], 0
    for i, (b, n) in enumerate(zip(bns, sizes)):
        sc, sh = pool[off:off + n], pool[off + n:off + 2 * n]
        off += 2 * n
        views.append((sc, sh))
        g = _ptr(b.weight, torch.float32, "bn.weight") if b.weight is not None else None
        be = _ptr(b.bias, torch.float32, "bn.bias") if b.bias is not None else None
        arr[i] = BnFoldDesc(g, be, _ptr(b.running_mean, torch.float32, "running_mean"),
                            _ptr(b.running_var, torch.float32, "running_var"), sc.data_ptr(), sh.data_ptr(), n, float(b.eps))
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    return {"table": table, "n": len(bns), "max": max(sizes), "pool": pool}, views


def bn_fold_run(plan):
    _chk(lib().rslo_bn_fold_many(_ptr(plan["table"]), plan["n"], plan["max"], _stream()), "rslo_bn_fold_many")


def pose_chain(t, q, state, count, rel_rows, traj):
    """One step of the streamed pose chain (rslo_pose_chain): t [3] / q [4] fp32 CUDA, state [7] fp64, count [1] int32,
    rel_rows [cap,7] fp32, traj [cap,7] fp64 -- row *count of both is written, then *count += 1."""
    _chk(lib().rslo_pose_chain(_ptr(t, torch.float32, "t"), _ptr(q, torch.float32, "q"), _ptr(state, torch.float64, "state"),
                               _ptr(count, torch.int32, "count"), _ptr(rel_rows, torch.float32, "rel_rows"),
                               _ptr(traj, torch.float64, "traj"), int(traj.shape[0]), _stream()), "rslo_pose_chain")


def conv2d_s2_supported(cin, cout, ksize):
    return bool(lib().rslo_conv2d_s2_supported(int(cin), int(cout), int(ksize)))


def conv2d_wsplit_k(w, transpose=False):
    """w [cout,cin,k,k] (k = 1 or 3) fp32 -> split-bf16 operands for conv2d_fwd_s2 (transpose=True: conv2d_dgrad_s2)."""
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    ws = torch.empty((3 * k * k * cin * cout,), dtype=torch.int16, device=w.device)
    _chk(lib().rslo_conv2d_wsplit_k(_ptr(w, torch.float32, "w"), cin, cout, k, 1 if transpose else 0, _ptr(ws), _stream()),
         "rslo_conv2d_wsplit_k")
    return ws


def conv2d_fwd_s2(x, ws, cout, ksize):
    """x [B,cin,H,W] contiguous fp32 -> [B,cout,Ho,Wo]: 3x3 / padding 1 or 1x1 / padding 0, stride 2, no bias."""
    B, cin, H, W = x.shape
    out = torch.empty((B, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    rc = lib().rslo_conv2d_fwd_s2(_ptr(x, torch.float32, "x"), ws.data_ptr(), B, cin, cout, H, W, ksize, out.data_ptr(),
                                  _stream())
    if rc:
        _chk(rc, "rslo_conv2d_fwd_s2")
    return out


def conv2d_dgrad_s2(dy, ws_t, cin, H, W, ksize, residual=None, inplace=False):
    """dy [B,cout,Ho,Wo] -> dx [B,cin,H,W] of the stride-2 layer; ws_t = the transpose=True operand.
    residual [B,cin,H,W]: added in the epilogue (rslo_conv2d_dgrad_s2_add); inplace (ksize 1): the gradient is added INTO
    residual, which is returned -- only the pixels (2y, 2x) are read and written."""
    B, cout = dy.shape[0], dy.shape[1]
    shape = (B, cin, H, W)
    if residual is not None and (tuple(residual.shape) != shape or not residual.is_contiguous()):
        raise ValueError("conv2d_dgrad_s2: residual must be a contiguous %s tensor" % (shape,))
    if inplace and (residual is None or ksize != 1):
        raise ValueError("conv2d_dgrad_s2: inplace needs a residual and ksize 1")
    dx = residual if inplace else torch.empty(shape, dtype=torch.float32, device=dy.device)
    rc = lib().rslo_conv2d_dgrad_s2_add(_ptr(dy, torch.float32, "dy"), ws_t.data_ptr(),
                                        _ptr(residual, torch.float32, "residual") if residual is not None else None,
                                        B, cin, cout, H, W, ksize, dx.data_ptr(), _stream())
    if rc:
        _chk(rc, "rslo_conv2d_dgrad_s2")
    return dx


def conv2d_fwd(x, ws, bias, cout, lp=False, residual=None):
    """x [B,cin,H,W] contiguous fp32, ws from conv2d_wsplit -> [B,cout,H,W] (3x3, stride 1, padding 1).
    lp: bf16 operands, fp32 accumulation (C4).  residual [B,cout,H,W]: added in the epilogue (rslo_conv2d_fwd_add)."""
    B, cin, H, W = x.shape
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    if residual is not None:
        if tuple(residual.shape) != tuple(out.shape) or not residual.is_contiguous():
            raise ValueError("conv2d_fwd: residual must be a contiguous %s tensor" % (tuple(out.shape),))
        fn = lib().rslo_conv2d_fwd_add_bf16 if lp else lib().rslo_conv2d_fwd_add
        rc = fn(_ptr(x, torch.float32, "x"), ws.data_ptr(), _dp(bias), _ptr(residual, torch.float32, "residual"), B, cin,
                cout, H, W, out.data_ptr(), _stream())
        if rc:
            _chk(rc, "rslo_conv2d_fwd_add")
        return out
    fn = lib().rslo_conv2d_fwd_bf16 if lp else lib().rslo_conv2d_fwd
    rc = fn(_ptr(x, torch.float32, "x"), ws.data_ptr(), _dp(bias), B, cin, cout, H, W, out.data_ptr(),
            _stream())
    if rc:
        _chk(rc, "rslo_conv2d_fwd")
    return out


def opl_from_nchw(x):
    """x [B,C,H,W] contiguous fp32 (C % 8 == 0) -> operand planes [B, C/8, 3, H, W, 8] bf16 bit patterns (int16):
    the exact hi / mid / lo split, one 16-byte piece per (pixel, channel octet, plane) -- what conv2d_fwd_p stages."""
    B, Cc, H, W = x.shape
    pl = torch.empty((B, Cc // 8, 3, H, W, 8), dtype=torch.int16, device=x.device)
    _chk(lib().rslo_opl_from_nchw(_ptr(x, torch.float32, "x"), B, Cc, H, W, pl.data_ptr(), _stream()), "rslo_opl_from_nchw")
    return pl


def conv2d_fwd_p_supported(cin, cout, H, W):
    return bool(lib().rslo_conv2d_fwd_p_supported(int(cin), int(cout), int(H), int(W)))


def conv2d_fwd_p(planes, ws, bias, cout, residual=None):
    """planes [B,cin/8,3,H,W,8] (opl_from_nchw or a BatchNorm apply kernel), ws from conv2d_wsplit -> [B,cout,H,W] fp32
    (3x3, stride 1, padding 1): the same bits as conv2d_fwd on the un-split tensor."""
    B, no, _, H, W, _ = planes.shape
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=planes.device)
    if residual is not None and (tuple(residual.shape) != tuple(out.shape) or not residual.is_contiguous()):
        raise ValueError("conv2d_fwd_p: residual must be a contiguous %s tensor" % (tuple(out.shape),))
    if not planes.is_contiguous() or planes.dtype != torch.int16:
        raise ValueError("conv2d_fwd_p: planes must be a contiguous int16 tensor")
    rc = lib().rslo_conv2d_fwd_p(planes.data_ptr(), ws.data_ptr(), _dp(bias),
                                 _ptr(residual, torch.float32, "residual") if residual is not None else None,
                                 B, no * 8, cout, H, W, out.data_ptr(), _stream())
    if rc:
        _chk(rc, "rslo_conv2d_fwd_p")
    return out


def conv1x1_supported(cin, cout):
    return bool(lib().rslo_conv1x1_supported(int(cin), int(cout)))


def conv1x1_fwd(x, w, bias):
    """x [B,cin,H,W], w [cout,cin,1,1] (cout <= 8), bias [cout] or None -> [B,cout,H,W]."""
    B, cin, H, W = x.shape
    cout = w.shape[0]
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    rc = lib().rslo_conv1x1_fwd(_ptr(x, torch.float32, "x"), _ptr(w, torch.float32, "w"), _dp(bias), B, cin, cout, H * W,
                                out.data_ptr(), _stream())
    if rc:
        _chk(rc, "rslo_conv1x1_fwd")
    return out


def conv1x1_dgrad(dy, w):
    B, cout, H, W = dy.shape
    cin = w.shape[1]
    dx = torch.empty((B, cin, H, W), dtype=torch.float32, device=dy.device)
    rc = lib().rslo_conv1x1_dgrad(_ptr(dy, torch.float32, "dy"), _ptr(w, torch.float32, "w"), B, cin, cout, H * W,
                                  dx.data_ptr(), _stream())
    if rc:
        _chk(rc, "rslo_conv1x1_dgrad")
    return dx


def conv1x1_wgrad(x, dy, want_bias=True):
    B, cin, H, W = x.shape
    cout = dy.shape[1]
    dev = x.device
    wsb = lib().rslo_conv1x1_wgrad_ws_bytes(B, cin, cout, H * W)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    dW = torch.empty((cout, cin, 1, 1), dtype=torch.float32, device=dev)
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if want_bias else None
    rc = lib().rslo_conv1x1_wgrad(_ptr(x, torch.float32, "x"), _ptr(dy, torch.float32, "dy"), B, cin, cout, H * W,
                                  dW.data_ptr(), _dp(db), ws.data_ptr(), wsb, _stream())
    if rc:
        _chk(rc, "rslo_conv1x1_wgrad")
    return dW, db


# --------------------------------------------------------------------------------------
# per-pair pose algebra
# --------------------------------------------------------------------------------------
def quat_to_rot(q):
    B = q.shape[0]
    R = torch.empty((B, 3, 3), dtype=torch.float32, device=q.device)
    _chk(lib().rslo_quat_to_rot(_ptr(q, torch.float32, "q"), B, _ptr(R), _stream()), "rslo_quat_to_rot")
    return R


def quat_to_rot_bwd(q, gR):
    B = q.shape[0]
    gq = torch.empty((B, 4), dtype=torch.float32, device=q.device)
    _chk(lib().rslo_quat_to_rot_bwd(_ptr(q, torch.float32, "q"), _ptr(gR, torch.float32, "gR"), B, _ptr(gq), _stream()),
         "rslo_quat_to_rot_bwd")
    return gq


def pose_targets(res_r, res_t, R_pred, T_pred, with_tq=False):
    """-> (q* [B,4] wxyz, t* [B,3]); with_tq: also the rows (t*, q*) [B,7] from the same launch."""
    B = res_r.shape[0]
    rot = torch.empty((B, 4), dtype=torch.float32, device=res_r.device)
    trans = torch.empty((B, 3), dtype=torch.float32, device=res_r.device)
    tq = torch.empty((B, 7), dtype=torch.float32, device=res_r.device) if with_tq else None
    _chk(lib().rslo_pose_targets_tq(_ptr(res_r, torch.float32, "res_r"), _ptr(res_t, torch.float32, "res_t"),
                                    _ptr(R_pred, torch.float32, "R_pred"), _ptr(T_pred, torch.float32, "T_pred"), B,
                                    _ptr(rot), _ptr(trans), _ptr(tq), _stream()), "rslo_pose_targets_tq")
    return (rot, trans, tq) if with_tq else (rot, trans)


# --------------------------------------------------------------------------------------
# place recognition (csrc/places.hip); the owning class is rslo_amd/places.py PlaceDB
# --------------------------------------------------------------------------------------
PLACE_HDR_ENTRIES = 4     # int64 words of a database's header: n_entries, dropped_full (include/rslo_hip.h)
PLACE_COUNTERS = ("n_points", "dropped_invalid", "dropped_range", "dropped_low")


def place_bytes(capacity, R, S):
    """rslo_place_bytes: bytes of a database of `capacity` entries of [R, S] descriptors; 0 for arguments out of range."""
    return int(lib().rslo_place_bytes(int(capacity), int(R), int(S)))


def place_reset(buf, capacity, R, S):
    """rslo_place_reset on the current stream: writes the header of an empty database."""
    ptr, nbytes = _map_buf(buf)
    _chk(lib().rslo_place_reset(ptr, nbytes, int(capacity), int(R), int(S), _stream()), "rslo_place_reset")


def place_describe(points, R, S, tables, z_offset, D, key, norm, counters):
    """rslo_place_describe: the Scan Context descriptor of one scan (fp32 CUDA [P, F >= 3], read in place) into D fp32
    [R, S], key int32 [R], norm float64 [S] and counters int64 [4], on the current stream.  tables: float64 CUDA
    [2*(S+1) + R+1] (places.tables).  No host read."""
    src, stride = _rows3(points, "points")
    if tables.numel() != 2 * (S + 1) + R + 1 or D.numel() != R * S or key.numel() != R or norm.numel() != S \
            or counters.numel() != 4:
        raise RsloHipError("place_describe: tables, D, key, norm or counters do not have the sizes of R = %d, S = %d" % (R, S))
    _chk(lib().rslo_place_describe(src, stride, int(points.shape[0]), int(R), int(S), _ptr(tables, torch.float64, "tables"),
                                   float(z_offset), _ptr(D, torch.float32, "D"), _ptr(key, torch.int32, "key"),
                                   _ptr(norm, torch.float64, "norm"), _ptr(counters, torch.int64, "counters"), _stream()),
         "rslo_place_describe")


def place_add(buf, capacity, R, S, D, key, norm):
    """rslo_place_add: append one descriptor on the current stream (a full database counts it in dropped_full)."""
    ptr, nbytes = _map_buf(buf)
    if D.numel() != R * S or key.numel() != R or norm.numel() != S:
        raise RsloHipError("place_add: D, key or norm do not have the sizes of R = %d, S = %d" % (R, S))
    _chk(lib().rslo_place_add(ptr, nbytes, int(capacity), int(R), int(S), _ptr(D, torch.float32, "D"),
                              _ptr(key, torch.int32, "key"), _ptr(norm, torch.float64, "norm"), _stream()), "rslo_place_add")


def place_query_ws(capacity, device):
    """a workspace for place_query on a database of `capacity` entries"""
    return torch.empty((max(int(lib().rslo_place_query_ws_bytes(int(capacity))), 8) // 8,), dtype=torch.int64, device=device)


def place_query(buf, capacity, R, S, D, key, norm, exclude_recent, num_candidates, top_k, out, ws):
    """rslo_place_query on the current stream: out float64 [top_k, 4] rows (entry, distance, shift, heading)."""
    ptr, nbytes = _map_buf(buf)
    if D.numel() != R * S or key.numel() != R or norm.numel() != S or out.numel() != 4 * int(top_k):
        raise RsloHipError("place_query: D, key, norm or out do not have the sizes of R = %d, S = %d, top_k = %d" % (R, S, top_k))
    _chk(lib().rslo_place_query(ptr, nbytes, int(capacity), int(R), int(S), _ptr(D, torch.float32, "D"),
                                _ptr(key, torch.int32, "key"), _ptr(norm, torch.float64, "norm"), int(exclude_recent),
                                int(num_candidates), int(top_k), _ptr(out, torch.float64, "out"),
                                _ptr(ws, torch.int64, "ws"), ws.numel() * 8, _stream()), "rslo_place_query")


# --------------------------------------------------------------------------------------
# pose graph (csrc/posegraph.hip); the owning class is rslo_amd/posegraph.py PoseGraph
# --------------------------------------------------------------------------------------
PG_EDGE_DOUBLES = 84      # doubles of an edge record (include/rslo_hip.h)
_D2 = C.c_double * 2


def posegraph_ws_bytes(N, L):
    """rslo_posegraph_ws_bytes: 0 for N outside 2..65536 or L outside 0..4096."""
    return int(lib().rslo_posegraph_ws_bytes(int(N), int(L)))


def _pg_graph(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, name):
    """the arguments every pose-graph call shares: (traj0, poses, N, chain pair, chain array, ij, Z, w, L)"""
    if traj0.dim() != 2 or traj0.shape[1] != 7 or poses.shape != traj0.shape:
        raise RsloHipError("%s: traj0 and poses must be [N, 7] float64" % name)
    N = int(traj0.shape[0])
    pair, arr = None, None
    if isinstance(chain_w, torch.Tensor):
        if tuple(chain_w.shape) != (N - 1, 2):
            raise RsloHipError("%s: a chain weight tensor must be [N-1, 2]" % name)
        arr = _ptr(chain_w, torch.float64, "chain_w")
    else:
        pair = _D2(float(chain_w[0]), float(chain_w[1]))
    L = 0 if loops_ij is None else int(loops_ij.shape[0])
    if L and (tuple(loops_ij.shape) != (L, 2) or tuple(loops_Z.shape) != (L, 7) or tuple(loops_w.shape) != (L, 2)):
        raise RsloHipError("%s: loops_ij [L, 2], loops_Z [L, 7] and loops_w [L, 2] must agree" % name)
    return (_ptr(traj0, torch.float64, "traj0"), _ptr(poses, torch.float64, "poses"), N, pair, arr,
            _ptr(loops_ij, torch.int32, "loops_ij") if L else None, _ptr(loops_Z, torch.float64, "loops_Z") if L else None,
            _ptr(loops_w, torch.float64, "loops_w") if L else None, L)


def posegraph_optimize(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, gn_iters, cg_iters, cg_tol, robust_scale, damping,
                       tol_t, tol_r, info, ws):
    """rslo_posegraph_optimize on the current stream: poses float64 CUDA [N, 7] updated in place, info [gn_iters, 8]."""
    g = _pg_graph(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, "posegraph_optimize")
    if 1 <= int(gn_iters) <= 32 and info.numel() != 8 * int(gn_iters):      # (a gn_iters out of range is the library's error)
        raise RsloHipError("posegraph_optimize: info must be [gn_iters, 8]")
    _chk(lib().rslo_posegraph_optimize(*g, int(gn_iters), int(cg_iters), float(cg_tol), float(robust_scale), float(damping),
                                       float(tol_t), float(tol_r), _ptr(info, torch.float64, "info"),
                                       _ptr(ws, torch.int64, "ws"), ws.numel() * 8, _stream()), "rslo_posegraph_optimize")


def posegraph_cost(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, robust_scale, out4, ws):
    """rslo_posegraph_cost: out4 float64 CUDA [4] = (cost, chain part, loops used, loops skipped)."""
    g = _pg_graph(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, "posegraph_cost")
    if out4.numel() != 4:
        raise RsloHipError("posegraph_cost: out4 must have 4 elements")
    _chk(lib().rslo_posegraph_cost(*g, float(robust_scale), _ptr(out4, torch.float64, "out4"), _ptr(ws, torch.int64, "ws"),
                                   ws.numel() * 8, _stream()), "rslo_posegraph_cost")


def posegraph_linearize(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, robust_scale, edges, g_out, sums4, ws):
    """rslo_posegraph_linearize: the edge records [(N-1+L), 84], the gradient [N, 6] and the four sums; the workspace
    keeps the linearisation for posegraph_matvec / posegraph_chain_solve."""
    g = _pg_graph(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, "posegraph_linearize")
    N, L = g[2], g[8]
    if (edges is not None and edges.numel() != (N - 1 + L) * PG_EDGE_DOUBLES) or \
            (g_out is not None and g_out.numel() != N * 6) or sums4.numel() != 4:
        raise RsloHipError("posegraph_linearize: edges, g or sums4 do not have the sizes of N = %d, L = %d" % (N, L))
    _chk(lib().rslo_posegraph_linearize(*g, float(robust_scale), _ptr(edges, torch.float64, "edges"),
                                        _ptr(g_out, torch.float64, "g"), _ptr(sums4, torch.float64, "sums4"),
                                        _ptr(ws, torch.int64, "ws"), ws.numel() * 8, _stream()), "rslo_posegraph_linearize")


def posegraph_matvec(x, y, N, L, damping, ws):
    """rslo_posegraph_matvec: y = H x, both float64 CUDA [N, 6], on the linearisation the workspace holds."""
    if x.numel() != N * 6 or y.numel() != N * 6:
        raise RsloHipError("posegraph_matvec: x and y must be [N, 6]")
    _chk(lib().rslo_posegraph_matvec(_ptr(x, torch.float64, "x"), _ptr(y, torch.float64, "y"), int(N), int(L), float(damping),
                                     _ptr(ws, torch.int64, "ws"), ws.numel() * 8, _stream()), "rslo_posegraph_matvec")


def posegraph_chain_solve(r, z, N, L, ws):
    """rslo_posegraph_chain_solve: z = M^-1 r, both float64 CUDA [N, 6], on the linearisation the workspace holds."""
    if r.numel() != N * 6 or z.numel() != N * 6:
        raise RsloHipError("posegraph_chain_solve: r and z must be [N, 6]")
    _chk(lib().rslo_posegraph_chain_solve(_ptr(r, torch.float64, "r"), _ptr(z, torch.float64, "z"), int(N), int(L),
                                          _ptr(ws, torch.int64, "ws"), ws.numel() * 8, _stream()),
         "rslo_posegraph_chain_solve")


def pose_between(A, B, out=None):
    """rslo_pose_between: out[k] = A[k]^-1 o B[k] for float64 CUDA [n, 7] rows, on the current stream."""
    if A.dim() != 2 or A.shape[1] != 7 or B.shape != A.shape:
        raise RsloHipError("pose_between: A and B must be [n, 7] float64")
    if out is None:
        out = torch.empty_like(A)
    elif out.shape != A.shape:
        raise RsloHipError("pose_between: out must be [n, 7]")
    _chk(lib().rslo_pose_between(_ptr(A, torch.float64, "A"), _ptr(B, torch.float64, "B"), int(A.shape[0]),
                                 _ptr(out, torch.float64, "out"), _stream()), "rslo_pose_between")
    return out


# --------------------------------------------------------------------------------------
# loop verification (csrc/loopverify.hip); the owning classes are rslo_amd/loops.py KeyframeStore / LoopVerifier
# --------------------------------------------------------------------------------------
KF_HDR_ENTRIES = 4        # int64 words of a store's header: n_entries, dropped_full (include/rslo_hip.h)
LOOP_OUT_COLS = 16


def keyframe_bytes(capacity, K):
    """rslo_keyframe_bytes: bytes of a store of `capacity` frames of K points; 0 for arguments out of range."""
    return int(lib().rslo_keyframe_bytes(int(capacity), int(K)))


def keyframe_reset(buf, capacity, K):
    """rslo_keyframe_reset on the current stream: writes the header of an empty store."""
    ptr, nbytes = _map_buf(buf)
    _chk(lib().rslo_keyframe_reset(ptr, nbytes, int(capacity), int(K), _stream()), "rslo_keyframe_reset")


def keyframe_prepare_ws(n_points, device):
    """a workspace for keyframe_prepare on scans of up to n_points points"""
    return torch.empty((max(int(lib().rslo_keyframe_prepare_ws_bytes(int(n_points))), 8) // 8 + 1,), dtype=torch.int64,
                       device=device)


def _frame(frame, info, K, name):
    if frame.numel() != 4 * int(K) or info.numel() != 4:
        raise RsloHipError("%s: frame must be [K, 4] float32 and frame_info [4] int32 for K = %d" % (name, K))
    return _ptr(frame, torch.float32, "frame"), _ptr(info, torch.int32, "frame_info")


def keyframe_prepare(points, K, voxel_size, min_z, max_range, frame, info, ws):
    """rslo_keyframe_prepare: gate, down-sample and select one scan (fp32 CUDA [P, F >= 3], read in place) into frame
    fp32 [K, 4] and frame_info int32 [4] = {count, Q, flags, gated}, on the current stream.  No host read."""
    src, stride = _rows3(points, "points")
    f, i = _frame(frame, info, K, "keyframe_prepare")
    _chk(lib().rslo_keyframe_prepare(src, stride, int(points.shape[0]), int(K), float(voxel_size), float(min_z),
                                     float(max_range), f, i, _ptr(ws, torch.int64, "ws"), ws.numel() * 8, _stream()),
         "rslo_keyframe_prepare")


def keyframe_add(buf, capacity, K, frame, info):
    """rslo_keyframe_add: append the staged frame on the current stream (a full store counts it in dropped_full)."""
    ptr, nbytes = _map_buf(buf)
    f, i = _frame(frame, info, K, "keyframe_add")
    _chk(lib().rslo_keyframe_add(ptr, nbytes, int(capacity), int(K), f, i, _stream()), "rslo_keyframe_add")


def loop_verify(buf, capacity, K, frame, info_q, cands, top_k, start, stages, max_distance, inlier_dist, min_overlap,
                max_rms, min_pairs, damping, out, info, matches):
    """rslo_loop_verify on the current stream: one workgroup per row of cands float64 [top_k, 4]; out float64
    [top_k, 16], info [top_k, sum of iters, 8] or None, matches int32 [top_k, K] or None, start [top_k, 7] or None.
    stages: host rows (max_dist, iters)."""
    ptr, nbytes = _map_buf(buf)
    f, i = _frame(frame, info_q, K, "loop_verify")
    top_k = int(top_k)
    flat = [float(v) for st in stages for v in st]
    n_stages = len(flat) // 2
    total = sum(int(st[1]) for st in stages) if n_stages else 0
    if cands.numel() != 4 * top_k or out.numel() != LOOP_OUT_COLS * top_k or (start is not None and start.numel() != 7 * top_k) \
            or (info is not None and 1 <= total <= 64 and info.numel() != top_k * total * 8) \
            or (matches is not None and matches.numel() != top_k * int(K)):
        raise RsloHipError("loop_verify: cands, start, out, info or matches do not have the sizes of top_k = %d, K = %d"
                           % (top_k, K))
    arr = (C.c_double * max(len(flat), 1))(*flat)
    _chk(lib().rslo_loop_verify(ptr, nbytes, int(capacity), int(K), f, i, _ptr(cands, torch.float64, "cands"), top_k,
                                _ptr(start, torch.float64, "start"), arr, n_stages, float(max_distance), float(inlier_dist),
                                float(min_overlap), float(max_rms), int(min_pairs), float(damping),
                                _ptr(out, torch.float64, "out"), _ptr(info, torch.float64, "info"),
                                _ptr(matches, torch.int32, "matches"), _stream()), "rslo_loop_verify")


def _edges(ij, Z, w, counters, name):
    E = int(ij.shape[0]) if ij.dim() == 2 else -1
    if tuple(ij.shape) != (E, 2) or tuple(Z.shape) != (E, 7) or tuple(w.shape) != (E, 2) or counters.numel() != 2:
        raise RsloHipError("%s: ij [E, 2], Z [E, 7], w [E, 2] and counters [2] must agree" % name)
    return (_ptr(ij, torch.int32, "ij"), _ptr(Z, torch.float64, "Z"), _ptr(w, torch.float64, "w"),
            _ptr(counters, torch.int64, "counters"), E)


def loop_edges_reset(ij, Z, w, counters):
    """rslo_loop_edges_reset: every row of the edge list becomes an unused one (i = j = -1), the counters zero."""
    _chk(lib().rslo_loop_edges_reset(*_edges(ij, Z, w, counters, "loop_edges_reset"), _stream()), "rslo_loop_edges_reset")


def loop_emit(out, top_k, buf, capacity, K, ij, Z, w, counters, w_t, w_r):
    """rslo_loop_emit: append the best accepted row of out float64 [top_k, 16] to the edge list, on the current stream."""
    ptr, nbytes = _map_buf(buf)
    if out.numel() != LOOP_OUT_COLS * int(top_k):
        raise RsloHipError("loop_emit: out must be [top_k, 16]")
    e = _edges(ij, Z, w, counters, "loop_emit")
    _chk(lib().rslo_loop_emit(_ptr(out, torch.float64, "out"), int(top_k), ptr, nbytes, int(capacity), int(K), *e,
                              float(w_t), float(w_r), _stream()), "rslo_loop_emit")

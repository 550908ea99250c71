"""ctypes binding of libape_hip.so (the C ABI declared in include/ape_hip.h).

There is NO CPU fallback: if the shared library is missing or a tensor is not on the GPU the call
raises.  torch is used only for device memory and streams (tensor.data_ptr(), current stream)."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("APE_HIP_LIB", os.path.join(_HERE, "libape_hip.so"))   # env override: kernel A/B experiments

_c = ctypes
_P, _I, _F, _L, _D = _c.c_void_p, _c.c_int, _c.c_float, _c.c_int64, _c.c_double

# symbol -> argtypes (restype is int unless listed in _RESTYPES); mirrors include/ape_hip.h one to one
SIGNATURES = {
    "ape_abi_version": [],
    "ape_last_error": [],
    "ape_knn_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "ape_conv2d_nhwc_f32": [_P, _P, _P, _P, _P, _P, _P],
    "ape_packed_weights_bf16_elems": [_I, _I],
    "ape_pack_weights_bf16": [_P, _P, _I, _I, _P],
    "ape_conv2d_nhwc_bf16": [_P, _P, _P, _P, _P, _P, _I, _P],
    "ape_conv_gemm_supported": [_P],
    "ape_conv_gemm_bf16": [_P, _P, _P, _P, _P, _P, _I, _I, _P],
    "ape_pack_weights_s32k": [_P, _P, _I, _I, _P],
    "ape_convert_s32": [_P, _P, _c.c_long, _I, _I, _P],
    "ape_point_feat_bf16": [_P] * 12 + [_c.c_long, _I, _I, _P],
    "ape_conv_gemm_s32_supported": [_P],
    "ape_conv_gemm_s32_debug": [_I],
    "ape_conv3x3_halo_s32_debug": [_I],
    "ape_conv_gemm_s32": [_P, _P, _P, _P, _I, _P, _I, _P, _P],
    "ape_conv_gemm_s32_per_image": [_P, _P, _c.c_long, _P, _P, _I, _P, _P],
    "ape_psp_fold_operands": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "ape_conv_gemm_bf16_fmt": [_P, _P, _P, _P, _P, _I, _P, _I, _I, _P],
    "ape_conv_gemm_splitk_workspace_bytes": [_P],
    "ape_conv_gemm_bf16_splitk": [_P, _P, _P, _P, _P, _P, _I, _P, _c.c_size_t, _P],
    "ape_conv_gemm_bf16_multi": [_I, _P, _P, _P, _P, _P, _I, _P],
    "ape_adaptive_avgpool_multi_nhwc_ld": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_upconv3x3_gather_ex": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P],
    "ape_upconv3x3_gather_strip_rows": [_I],
    "ape_upconv3x3_fused_supported": [_I, _I, _I, _I],
    "ape_upconv3x3_fused_debug": [_I],
    "ape_upconv3x3_fused_stamps": [_P],
    "ape_upconv3x3_fused_s32": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P],
    "ape_upconv3x3_fused_seghead_s32": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P, _P, _I, _P, _P, _I, _P],
    "ape_conv3x3_halo_s32_supported": [_P],
    "ape_conv3x3_halo_s32": [_P, _P, _P, _P, _I, _P, _I, _P, _P],
    "ape_conv3x3_halo_mx_supported": [_P],
    "ape_conv3x3_halo_mx": [_P, _P, _P, _P, _I, _P, _I, _P, _P],
    "ape_conv3x3_halo_mx_debug": [_I],
    "ape_s32_to_f16m6": [_P, _P, _c.c_long, _I, _P],
    "ape_stem_conv_pool_bf16": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "ape_stem_conv_pool_u8": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "ape_conv3x3_halo_supported": [_P],
    "ape_conv3x3_halo_bf16": [_P, _P, _P, _P, _P, _P, _I, _P],
    "ape_maxpool3x3s2_nhwc_f32": [_P, _P, _I, _I, _I, _I, _P],
    "ape_adaptive_avgpool_nhwc_f32": [_P, _P, _I, _I, _I, _I, _I, _P],
    "ape_adaptive_avgpool_multi_workspace_bytes": [_I, _I],
    "ape_bilinear_nhwc_f32": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "ape_psp_prior_sum_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "ape_upconv3x3_gather_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _P],
    "ape_gather_rows_f32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "ape_ups_patch_gather_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "ape_log_softmax_rows_f32": [_P, _P, _c.c_long, _I, _P],
    "ape_mean_rows_f32": [_P, _P, _I, _I, _I, _P],
    "ape_pad3to4_f32": [_P, _P, _c.c_long, _P],
    "ape_head_select_f32": [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "ape_pose_select_f32": [_P, _P, _P, _P, _P, _I, _I, _P],
    "ape_head_conf_argmax_f32": [_P, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _P],
    "ape_pose_from_row_f32": [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "ape_pose_compose_f64": [_P, _P, _I, _P, _I, _I, _P],
    "ape_pose_recentre_f32": [_P, _P, _P, _I, _I, _P],
    "ape_adds_dis_f32": [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    "ape_adds_dis_batched_f32": [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P],
    "ape_adds_select_f32": [_P, _P, _P, _P, _P, _P, _I, _F, _P, _P, _P],
    "ape_recentre_qt_f32": [_P, _P, _P, _I, _P],
    # the YCB toolbox's pose errors (csrc/pose_errors.hip)
    "ape_pose_errors_chunk": [],
    "ape_pose_errors_queries": [],
    "ape_pose_errors_lanes": [_c.c_long, _I],
    "ape_pose_errors_workspace_bytes": [_c.c_long, _I],
    "ape_pose_errors_f64": [_P, _P, _I, _c.c_long, _P, _P, _P, _P, _c.c_long, _I, _I, _P, _P, _c.c_size_t, _P],
    "ape_seg_argmax_f32": [_P, _I, _I, _P, _P, _c.c_long, _I, _P],
    "ape_seg_head_f32": [_P, _P, _P, _I, _P, _P, _c.c_long, _I, _P],
    "ape_seg_components_workspace_bytes": [_I, _I, _I, _I],
    "ape_conv3x3_halo_seghead_bf16": [_P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P],
    "ape_unet_conv3x3_supported": [_I, _I, _I, _I],
    "ape_unet_conv3x3_bf16": [_P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "ape_unet_conv3x3_seghead_bf16": [_P, _I, _I, _P, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "ape_nearest_upsample_nhwc_f32": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "ape_seg_components_scored": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_bgsub_features_f32": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "ape_conv2d_wgrad_workspace_bytes": [_P],
    "ape_conv2d_wgrad_nhwc_f32": [_P, _P, _P, _P, _P, _c.c_size_t, _P],
    "ape_act_bwd_f32": [_P, _P, _P, _c.c_long, _I, _F, _P],
    "ape_prelu_f32": [_P, _P, _c.c_long, _F, _P],
    "ape_prelu_dalpha_f32": [_P, _P, _P, _c.c_long, _P, _P],
    "ape_colsum_f32": [_P, _P, _c.c_long, _I, _I, _I, _P, _P],
    "ape_maxpool3x3s2_bwd_nhwc_f32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "ape_adaptive_avgpool_bwd_nhwc_f32": [_P, _P, _I, _I, _I, _I, _I, _P],
    "ape_bilinear_bwd_nhwc_f32": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "ape_log_softmax_bwd_rows_f32": [_P, _P, _P, _c.c_long, _I, _P],
    "ape_scatter_add_rows_f32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "ape_mean_rows_bwd_f32": [_P, _P, _I, _I, _I, _P],
    "ape_adds_grad_f32": [_P] * 9 + [_I, _I, _I, _I, _F, _P, _P, _P, _P],
    "ape_adam_step_f32": [_P, _P, _P, _P, _c.c_long, _F, _F, _F, _F, _I, _F, _P],
    "ape_adam_step_multi_f32": [_I, _P, _F, _F, _F, _F, _F, _P],
    "ape_pack_train_weights": [_I, _P, _c.c_long, _P],
    "ape_conv2d_wgrad_param_f32": [_P, _P, _P, _P, _I, _P, _c.c_size_t, _P],
    "ape_label_trust_counts": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    "ape_choose_points": [_P, _P, _P, _I, _I, _I, _I, _c.c_uint, _P, _c.c_long, _P, _P, _P],
    "ape_choose_points_dseed": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _c.c_long, _P, _P, _P],
    "ape_backproject_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _F, _F, _F, _P],
    "ape_preprocess_u8_nhwc4": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "ape_grid_nn1_f64": [_P, _P, _P, _P, _I, _D, _P, _I, _D, _P, _P, _P],
    "ape_knn_mean_dist_f64": [_P, _I, _I, _P, _P],
    "ape_icp_sums_f64": [_I, _P, _P, _P, _P, _P, _I, _P, _P, _c.c_size_t, _P],
    # blockIdx.y = cloud; per-cloud arguments as host arrays of pointers / sizes
    "ape_pc_batch_workspace_bytes": [_I, _c.c_long],
    "ape_surface_points_batch_f64": [_I, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P],
    "ape_voxel_down_sample_batch_f64": [_I, _P, _P, _D, _P, _P, _P, _c.c_size_t, _P],
    "ape_grid_build_batch_f64": [_I, _P, _P, _D, _P, _P, _P, _P, _P, _c.c_size_t, _P],
    "ape_grid_query_batch_f64": [_I, _I, _P, _P, _P, _P, _P, _D, _P, _P, _D, _I, _P, _P, _P, _P],
    "ape_select_points_batch_f64": [_I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P],
    "ape_moments_batch_f64": [_I, _P, _P, _P, _P, _c.c_size_t, _P],
    "ape_mahalanobis_batch_f64": [_I, _P, _P, _P, _P, _P],
    "ape_transform_points_batch_f64": [_I, _P, _P, _P, _P, _P],
    "ape_concat_points_batch_f64": [_I, _P, _P, _P, _P, _P, _P],
    "ape_icp_run_batch_f64": [_I, _I, _P, _P, _P, _P, _P, _D, _P, _P, _P, _P, _D, _D, _D, _I, _I, _I, _P, _P, _P, _P, _P, _c.c_size_t, _P],
    # global registration (csrc/registration.hip): per-pair arguments as host arrays of pointers / sizes, the pair's index in a grid dimension
    "ape_fpfh_batch_workspace_bytes": [_I, _P, _I],
    "ape_fpfh_batch_f64": [_I, _P, _P, _P, _P, _P, _D, _P, _P, _D, _I, _P, _P, _c.c_size_t, _P],
    "ape_feature_nn1_batch_workspace_bytes": [_I, _P, _P],
    "ape_feature_nn1_batch_f64": [_I, _P, _P, _P, _P, _P, _P, _c.c_size_t, _P],
    "ape_ransac_batch_workspace_bytes": [_I, _P, _I, _I],
    "ape_ransac_hypotheses_batch_f64": [_I, _P, _P, _P, _P, _P, _I, _P, _D, _D, _I, _I, _I, _P, _P, _P, _c.c_size_t, _P],
    "ape_ransac_validate_batch_f64": [_I, _P, _P, _P, _P, _P, _D, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _D, _P, _P, _P, _c.c_size_t, _P],
    # fast global registration (csrc/registration.hip, batched forms only: the one-pair call is a batch of one)
    "ape_fgr_mutual_batch": [_I, _P, _P, _P, _P, _P, _P, _P, _P],
    "ape_fgr_workspace_bytes": [_I, _I],
    "ape_fgr_tuples_batch_f64": [_I, _P, _P, _P, _P, _P, _P, _P, _P, _D, _I, _I, _I, _P, _P, _P, _c.c_size_t, _P],
    "ape_fgr_optimize_batch_f64": [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _D, _D, _I, _P, _P, _P],
    "ape_icp_polish_batch_f64": [_I, _P, _P, _I, _P, _P, _I, _I, _D, _P, _D, _D, _D, _I, _D, _P, _P, _P],
    "ape_icp_polish_plane_batch_f64": [_I, _P, _P, _I, _P, _P, _P, _I, _I, _D, _P, _D, _D, _D, _I, _D, _P, _P, _P],
    # segmentor training (csrc/segtrain.hip)
    "ape_bn_workspace_bytes": [_I],
    "ape_bn_train_fwd_f32": [_P] * 10 + [_c.c_long, _I, _F, _F, _I, _P, _c.c_size_t, _P],
    "ape_bn_train_bwd_f32": [_P] * 10 + [_c.c_long, _I, _P, _c.c_size_t, _P],
    "ape_upsample_nearest2x_bwd_f32": [_P, _I, _I, _P, _I, _I, _I, _I, _P],
    "ape_softmax_rows_f32": [_P, _P, _c.c_long, _I, _P],
    "ape_softmax_rows_bwd_f32": [_P, _P, _P, _c.c_long, _I, _P],
    "ape_jaccard_workspace_bytes": [_I, _I],
    "ape_jaccard_fwd_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _c.c_size_t, _P],
    "ape_jaccard_bwd_f32": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _c.c_size_t, _P],
    "ape_confusion_add": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "ape_sgd_step_multi_f32": [_I, _P, _F, _F, _F, _F, _I, _P],
    "ape_bgsub_train_workspace_bytes": [_I],
    "ape_bgsub_train_samples": [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _c.c_size_t, _P],
    # segmentor training samples (csrc/seg_train.hip): the extents of segmentation/utils.py:450-462 and ImageEnhance.Contrast's mean,
    # then dataset.py:98-112 with the transforms of utils.py:25-66 and CropAndZoom :361-487; the 'test' mode sample
    "ape_seg_train_workspace_bytes": [_I, _I],
    "ape_seg_train_extents_offset": [_I],
    "ape_seg_train_tables_offset": [_I],
    "ape_seg_train_stats": [_P, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_seg_train_samples": [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _c.c_size_t, _P],
    "ape_seg_plain_samples": [_P, _I, _I, _I, _P, _P, _P, _P, _P],
    # DenseFusion training samples (csrc/pose_train.hip): DenseFusion/datasets/myDatasetAugmented/dataset.py:158-326
    "ape_pose_train_extents_offset": [_I],
    "ape_pose_train_rows_offset": [_I],
    "ape_pose_train_tables_offset": [_I, _I],
    "ape_pose_train_sel_offset": [_I, _I],
    "ape_pose_train_workspace_bytes": [_I, _I, _I],
    "ape_pose_train_image_offset": [_I],
    "ape_pose_train_sample_bytes": [_I, _I, _I],
    "ape_pose_train_stats": [_P, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_pose_train_samples": [_P, _I, _I, _I, _I, _P, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P],
    # LineMOD samples (csrc/linemod.hip): DenseFusion/datasets/linemod/dataset.py:90-195; the job struct `ape_linemod_job` is mirrored next
    # to its one user, DenseFusion/datasets/linemod/augment.py
    "ape_linemod_box_workspace_bytes": [_I, _I, _I],
    "ape_linemod_boxes": [_P, _I, _I, _I, _P, _P, _c.c_size_t, _P],
    "ape_linemod_rows_offset": [_I],
    "ape_linemod_tables_offset": [_I, _I],
    "ape_linemod_sel_offset": [_I, _I],
    "ape_linemod_workspace_bytes": [_I, _I, _I],
    "ape_linemod_rows": [_P, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_linemod_samples": [_P, _I, _I, _I, _I, _P, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P],
    # YCB-Video samples (csrc/ycb.hip): DenseFusion/datasets/ycb/dataset.py:97-232; `ape_ycb_job` is mirrored next to its one user,
    # DenseFusion/datasets/ycb/augment.py
    "ape_ycb_overlap": [_P, _I, _I, _I, _P, _P],
    "ape_ycb_rows_offset": [_I],
    "ape_ycb_tables_offset": [_I, _I],
    "ape_ycb_sel_offset": [_I, _I],
    "ape_ycb_noise_offset": [_I, _I, _I],
    "ape_ycb_rows": [_P, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_ycb_samples": [_P, _I, _I, _I, _I, _P, _P, _P, _c.c_size_t, _P, _c.c_size_t, _P],
    # SegNet glue (csrc/segnet.hip): 2x2 max-pool with its winner codes, unpool, gather, cross-entropy
    "ape_maxpool2x2_idx_nhwc_f32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "ape_max_unpool2x2_nhwc_f32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "ape_gather2x2_nhwc_f32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "ape_cross_entropy_workspace_bytes": [_c.c_long],
    "ape_cross_entropy_f32": [_P, _I, _I, _P, _c.c_long, _F, _P, _P, _P, _c.c_size_t, _P],
    # SegNet training samples (csrc/segnet_samples.hip): vanilla_segmentation/data_controller.py:43-93; `ape_segnet_job` is mirrored next to
    # its one user, DenseFusion/vanilla_segmentation/augment.py
    "ape_segnet_samples_frames_offset": [_I],
    "ape_rgbd_gate_f64": [_P, _P, _P, _I, _I, _I, _P],
    "ape_rgbd_plane_fill_f64": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "ape_rgbd_box_f64": [_P, _P, _I, _I, _I, _I, _P],
    "ape_rgbd_score_f64": [_P, _P, _P, _P, _P, _I, _P, _D, _P, _P, _I, _I, _I, _P],
    "ape_rgbd_morph_f64": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "ape_rgbd_wrap_u8": [_P, _P, _c.c_long, _P],
    "ape_rgbd_cca_workspace_bytes": [_I, _I, _I],
    "ape_rgbd_component_stats": [_P, _P, _P, _P, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_rgbd_cca_round": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_segnet_samples_prepare": [_P, _I, _I, _I, _P, _c.c_size_t, _P],
    "ape_segnet_samples": [_P, _I, _I, _I, _P, _P, _P, _P, _P, _c.c_size_t, _P],
    # overlays (csrc/overlay.hip): the color_prediction images of pipeline/utils.py:471-476,576-585 and the review screens' :280-286,362
    "ape_overlay_stamp_counts_f64": [_P, _I, _P, _c.c_long, _P, _I, _P, _D, _D, _D, _D, _I, _P, _I, _I, _I, _I, _P],
    "ape_overlay_blend_u8": [_P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    # label-quality audit (csrc/label_audit.hip): compute_IoU's counts and the comparison image of experiments/gt_test.py:105-120,160-194
    "ape_label_pair_counts_u8": [_P, _I, _I, _I, _P, _I, _P, _P],
    "ape_label_pair_blend_u8": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _D, _D, _P, _P],
}


# The struct mirrors below are the ones tests/test_abi.py compares with the C compiler's layout.  They are not every mirror of the header:
# those of `ape_linemod_job`, of `ape_ycb_job` / `ape_ycb_jitter` / `ape_ycb_pair` and of `ape_segnet_job` live next to their one user
# (DenseFusion/datasets/{linemod,ycb}/augment.py, DenseFusion/vanilla_segmentation/augment.py) and get the same layout check in
# tests/test_linemod_host.py, tests/test_ycb_host.py and tests/test_segnet_samples_host.py.
class AdamJob(_c.Structure):
    """Mirror of `ape_adam_job` (include/ape_hip.h)."""
    _fields_ = [("param", _c.c_void_p), ("grad", _c.c_void_p), ("exp_avg", _c.c_void_p), ("exp_avg_sq", _c.c_void_p), ("n", _c.c_long),
                ("bc1", _c.c_float), ("bc2_sqrt", _c.c_float)]


class SgdJob(_c.Structure):
    """Mirror of `ape_sgd_job` (include/ape_hip.h)."""
    _fields_ = [("param", _c.c_void_p), ("grad", _c.c_void_p), ("momentum_buffer", _c.c_void_p), ("n", _c.c_long), ("first", _c.c_int32),
                ("reserved", _c.c_int32)]


class PackJob(_c.Structure):
    """Mirror of `ape_pack_job` (include/ape_hip.h)."""
    _fields_ = [("src", _c.c_void_p), ("dst_f32", _c.c_void_p), ("dst_bf16", _c.c_void_p), ("cout", _c.c_int32), ("cin", _c.c_int32),
                ("taps", _c.c_int32), ("transpose", _c.c_int32), ("src_ld", _c.c_int32), ("reserved", _c.c_int32)]


class ConvParams(_c.Structure):
    """Mirror of `ape_conv_params` (include/ape_hip.h)."""
    _fields_ = [(n, _c.c_int32) for n in ("B", "H", "W", "Cin", "ldx", "xoff", "Ho", "Wo", "Cout", "ldy", "yoff",
                                          "KH", "KW", "stride", "pad", "dil", "act")] + \
               [("alpha", _c.c_float), ("bias_bstride", _c.c_int32), ("ldr", _c.c_int32), ("roff", _c.c_int32), ("ups", _c.c_int32)]


class AugRotation(_c.Structure):
    """Mirror of `ape_aug_rotation` (include/ape_hip.h)."""
    _fields_ = [("a", _c.c_double * 6), ("fa", _c.c_int32 * 6), ("mode", _c.c_int32), ("reserved", _c.c_int32)]


class AugJitter(_c.Structure):
    """Mirror of `ape_aug_jitter` (include/ape_hip.h)."""
    _fields_ = [("n_ops", _c.c_int32), ("code", _c.c_int32 * 4), ("factor", _c.c_float * 4), ("shift", _c.c_int32 * 4)]


class BgsubTrainJob(_c.Structure):
    """Mirror of `ape_bgsub_train_job` (include/ape_hip.h)."""
    _fields_ = [("f_rgb", _c.c_void_p), ("b_rgb", _c.c_void_p), ("f_depth", _c.c_void_p), ("b_depth", _c.c_void_p), ("label", _c.c_void_p),
                ("rot", AugRotation), ("jit", AugJitter * 2), ("hflip", _c.c_int32), ("vflip", _c.c_int32)]


class SegTrainJob(_c.Structure):
    """Mirror of `ape_seg_train_job` (include/ape_hip.h)."""
    _fields_ = [("rgb", _c.c_void_p), ("label", _c.c_void_p), ("rot", AugRotation), ("jit", AugJitter), ("crop_x", _c.c_int32),
                ("crop_y", _c.c_int32), ("crop_side", _c.c_int32), ("class_id", _c.c_int32)]


class PoseTrainJob(_c.Structure):
    """Mirror of `ape_pose_train_job` (include/ape_hip.h)."""
    _fields_ = [("rgb", _c.c_void_p), ("depth", _c.c_void_p), ("label", _c.c_void_p), ("rot", AugRotation), ("add_t", _c.c_double * 3),
                ("out_off", _c.c_longlong), ("jit", AugJitter), ("rmin", _c.c_int32), ("rmax", _c.c_int32), ("cmin", _c.c_int32),
                ("cmax", _c.c_int32), ("ppx", _c.c_float), ("ppy", _c.c_float), ("fx", _c.c_float), ("fy", _c.c_float),
                ("depth_scale", _c.c_float), ("to_meter", _c.c_int32), ("add_noise", _c.c_int32)]


ACT_NONE, ACT_RELU, ACT_PRELU, ACT_SIGMOID = 0, 1, 2, 3
_RESTYPES = {"ape_last_error": _c.c_char_p, "ape_adaptive_avgpool_multi_workspace_bytes": _c.c_size_t, "ape_seg_components_workspace_bytes": _c.c_size_t,
             "ape_packed_weights_bf16_elems": _c.c_long, "ape_pc_batch_workspace_bytes": _c.c_size_t,
             "ape_conv2d_wgrad_workspace_bytes": _c.c_size_t, "ape_conv_gemm_splitk_workspace_bytes": _c.c_size_t,
             "ape_fpfh_batch_workspace_bytes": _c.c_size_t, "ape_feature_nn1_batch_workspace_bytes": _c.c_size_t,
             "ape_ransac_batch_workspace_bytes": _c.c_size_t, "ape_fgr_workspace_bytes": _c.c_size_t,
             "ape_bn_workspace_bytes": _c.c_size_t, "ape_jaccard_workspace_bytes": _c.c_size_t,
             "ape_bgsub_train_workspace_bytes": _c.c_size_t, "ape_seg_train_workspace_bytes": _c.c_size_t,
             "ape_seg_train_extents_offset": _c.c_size_t, "ape_seg_train_tables_offset": _c.c_size_t,
             "ape_pose_train_extents_offset": _c.c_size_t, "ape_pose_train_rows_offset": _c.c_size_t,
             "ape_pose_train_tables_offset": _c.c_size_t, "ape_pose_train_sel_offset": _c.c_size_t,
             "ape_pose_train_workspace_bytes": _c.c_size_t, "ape_pose_train_image_offset": _c.c_size_t,
             "ape_pose_train_sample_bytes": _c.c_size_t,
             "ape_linemod_box_workspace_bytes": _c.c_size_t, "ape_linemod_rows_offset": _c.c_size_t,
             "ape_linemod_tables_offset": _c.c_size_t, "ape_linemod_sel_offset": _c.c_size_t, "ape_linemod_workspace_bytes": _c.c_size_t,
             "ape_ycb_rows_offset": _c.c_size_t, "ape_ycb_tables_offset": _c.c_size_t, "ape_ycb_sel_offset": _c.c_size_t,
             "ape_ycb_noise_offset": _c.c_size_t, "ape_pose_errors_workspace_bytes": _c.c_size_t,
             "ape_cross_entropy_workspace_bytes": _c.c_size_t, "ape_segnet_samples_frames_offset": _c.c_size_t,
             "ape_rgbd_cca_workspace_bytes": _c.c_size_t}

_lib = None


ABI_VERSION = 23 # what ape_abi_version() of the library this table mirrors returns


class ApeError(RuntimeError):
    code = None      # the status an entry point returned, when that is what failed


def lib():
    """Load libape_hip.so once; raise loudly when it is absent (never fall back to a CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C autoposeestimation_amd/csrc` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
        h = ctypes.CDLL(LIB_PATH)
        h.ape_abi_version.restype = _c.c_int
        if h.ape_abi_version() != ABI_VERSION:
            raise ImportError("%s is ABI %d, this package expects ABI %d: a stale library -- rebuild it with "
                              "`python -c 'import __graft_entry__ as g; g.build()'`" % (LIB_PATH, h.ape_abi_version(), ABI_VERSION))
        for name, argtypes in SIGNATURES.items():
            fn = getattr(h, name)  # AttributeError here = header and library disagree
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, _c.c_int)
        _lib = h
    return _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def stream_ptr():
    """the HIP stream torch is currently enqueuing on (per thread, per device).  torch.cuda.current_stream() builds a Stream object
    through several Python layers (~12 us); the raw accessor is one C call -- at ~20 launches per registration / ~140 per frame batch
    this is a visible share of the host time"""
    if _raw_stream is not None:
        return _c.c_void_p(_raw_stream(_get_device()))
    return _c.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t, dtype=None):
    """Device pointer of a contiguous CUDA(HIP) tensor; refuses host tensors."""
    if t is None:
        return _c.c_void_p(0)
    if not t.is_cuda:
        raise ApeError("tensor is on %s; the HIP path needs device memory (no CPU fallback)" % t.device)
    if not t.is_contiguous():
        raise ApeError("tensor must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise ApeError("expected %s, got %s" % (dtype, t.dtype))
    return _c.c_void_p(t.data_ptr())


def _failed(what, rc):
    msg = lib().ape_last_error()
    err = ApeError("%s failed: code %d (%s)" % (what, rc, msg.decode() if msg else ""))
    err.code = rc
    return err


def check(rc, what):
    if rc != 0:
        raise _failed(what, rc)


class _Checked:
    """`call.ape_x(args)`: the status-returning entry point ape_x with its status checked -- raises ApeError (symbol, `.code`,
    ape_last_error) unless it returns APE_OK.  The checked form of a symbol is a ctypes function object of its own (the raw handle's
    `lib().ape_x` stays unchecked: tests and tools assert on its return code) whose `errcheck` does the test; it is built on first use and
    kept as an attribute.  Functions that return a value (*_supported, *_workspace_bytes, ...) are read through lib()."""

    def __getattr__(self, name):
        if name not in SIGNATURES or name in _RESTYPES or name.endswith(_QUERIES):
            raise AttributeError("%s is not a status-returning entry point of include/ape_hip.h" % name)
        fn = lib()[name]          # (item access makes a new function object; attribute access returns the cached raw one)
        fn.argtypes, fn.restype = SIGNATURES[name], _c.c_int

        def errcheck(rc, func, args):
            if rc:
                raise _failed(name, rc)
            return rc

        fn.errcheck = errcheck
        setattr(self, name, fn)
        return fn


_QUERIES = ("_supported", "_elems", "_debug", "_strip_rows", "ape_abi_version")
call = _Checked()

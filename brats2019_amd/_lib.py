"""ctypes binding of libresunet_hip.so (include/resunet_hip.h).  No torch types cross the ABI: tensors are
handed over as raw device pointers + extents, the stream as the hipStream_t integer of torch's current
stream.  The product path is HIP-only: if the library is missing or no GPU is usable, calls raise -- there
is no CPU fallback (the CPU restatement lives in oracle/ and is test infrastructure only)."""
from __future__ import annotations

import ctypes as C
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# RU_LIB_PATH: another build of the same library (A/B timing of kernel changes on one GPU box)
LIB_PATH = os.environ.get("RU_LIB_PATH") or os.path.join(_PKG, "lib", "libresunet_hip.so")

_lib = None
PRECISIONS = {"f32": 0, "bf16x3": 1}      # RU_PREC_F32 / RU_PREC_BF16X3
GRAD_PRECISIONS = {"bf16x3": 1, "bf16": 2}   # ru_unet_set_grad_precision: RU_PREC_BF16X3 / RU_PREC_BF16
FUSE_GN_BWD_STATS, FUSE_GN_BWD_APPLY, FUSE_SIDE_STREAM, FUSE_BATCH_WREDUCE, FUSE_TAIL_FINALIZE, FUSE_PW_DGRAD = 1, 2, 4, 8, 16, 32   # RU_FUSE_*

_vp, _f, _d, _i, _sz = C.c_void_p, C.c_float, C.c_double, C.c_int, C.c_size_t

# name -> (restype, argtypes); mirrors include/resunet_hip.h one to one
SIGNATURES = {
    "ru_last_error": (C.c_char_p, []),
    "ru_version": (_i, []),
    "ru_device_ok": (_i, []),
    "ru_conv3d_workspace_bytes": (_sz, [_i] * 7),
    "ru_conv3d_fwd": (_i, [_vp, _vp, _vp, _vp] + [_i] * 7 + [_vp, _sz, _vp]),
    "ru_conv3d_bwd_data": (_i, [_vp, _vp, _vp] + [_i] * 7 + [_vp, _sz, _vp]),
    "ru_conv3d_fwd_p": (_i, [_vp, _vp, _vp, _vp] + [_i] * 8 + [_vp, _sz, _vp]),
    "ru_conv3d_bwd_data_p": (_i, [_vp, _vp, _vp] + [_i] * 8 + [_vp, _sz, _vp]),
    "ru_conv3d_bwd_weight": (_i, [_vp, _vp, _vp, _vp] + [_i] * 7 + [_vp, _sz, _vp]),
    "ru_conv3d_bwd_weight_p": (_i, [_vp, _vp, _vp, _vp] + [_i] * 8 + [_vp, _sz, _vp]),
    "ru_conv3d_fwd_splitk_workspace_bytes": (_sz, [_i] * 7),
    "ru_conv3d_fwd_splitk": (_i, [_vp, _vp, _vp, _vp] + [_i] * 7 + [_vp, _sz, _vp]),
    "ru_conv3_f32_inst": (_i, [_i] * 6),
    "ru_wgrad3_inst": (_i, [_i] * 8 + [C.POINTER(_i)]),
    "ru_conv1_inst": (_i, [_i, _i, _i, _sz]),
    "ru_wgrad1_inst": (_i, [_i, _i, _i, _sz, C.POINTER(_i)]),
    "ru_groupnorm_workspace_bytes": (_sz, [_i, _i, _sz]),
    "ru_groupnorm_fwd": (_i, [_vp] * 7 + [_i, _i, _sz, _i, _f, _f, _vp, _sz, _vp]),
    "ru_groupnorm_bwd": (_i, [_vp] * 9 + [_i, _i, _sz, _i, _f, _vp, _sz, _vp]),
    "ru_leaky_relu_fwd": (_i, [_vp, _vp, _sz, _f, _vp]),
    "ru_leaky_relu_bwd": (_i, [_vp, _vp, _vp, _sz, _f, _vp]),
    "ru_upsample2x_trilinear_fwd": (_i, [_vp, _vp] + [_i] * 5 + [_vp]),
    "ru_upsample2x_trilinear_bwd": (_i, [_vp, _vp] + [_i] * 5 + [_vp]),
    "ru_sigmoid_fwd": (_i, [_vp, _vp, _sz, _vp]),
    "ru_criterion_workspace_bytes": (_sz, [_i, _i, _sz]),
    "ru_criterion_sums": (_i, [_vp, _vp, _vp, _i, _i, _sz, _f, _vp, _sz, _vp]),
    "ru_criterion_grad": (_i, [_vp, _vp, _vp, _d, _f, _f, _f, _f, _vp, _i, _i, _sz, _vp]),
    "ru_criterion_value": (_i, [C.POINTER(_d), _i, _d, _d, C.POINTER(_d), C.POINTER(_d)]),
    "ru_criterion_value_device": (_i, [_vp, _i, _d, _d, _d, _d, _vp, _vp]),
    "ru_crit_moments_workspace_bytes": (_sz, [_i, _i, _sz]),
    "ru_crit_moments": (_i, [_vp, _vp, _i, _i, _sz, C.c_uint, _vp, _vp, _sz, _vp]),
    "ru_crit_reduce": (_i, [_vp, _i, _i, _vp, _vp]),
    "ru_crit_eval": (_i, [_vp, _vp, _i, _i, _d, _d, _vp, _i, _vp, _vp, _vp]),
    "ru_crit_grad": (_i, [_vp, _vp, _vp, _vp, _i, _i, _sz, _i, _vp, _vp]),
    "ru_focal_workspace_bytes": (_sz, [_sz]),
    "ru_focal_sum": (_i, [_vp, _vp, _sz, _f, _f, _f, _vp, _vp, _sz, _vp]),
    "ru_focal_grad": (_i, [_vp, _vp, _sz, _f, _f, _f, _d, _vp, _vp, _vp]),
    "ru_tversky_eval": (_i, [_vp, _i, _i, _d, _d, _d, _d, _d, _vp, _vp, _vp]),
    "ru_topk_workspace_bytes": (_sz, [_sz]),
    "ru_topk_select": (_i, [_vp, _vp, _sz, C.c_ulonglong, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ru_topk_grad": (_i, [_vp, _vp, _vp, _vp, _sz, C.c_ulonglong, _f, _d, _vp, _vp, _vp]),
    "ru_signed_sqdist_workspace_bytes": (_sz, [_i] * 4),
    "ru_signed_sqdist": (_i, [_vp] + [_i] * 4 + [_vp, _vp, _sz, _vp]),
    "ru_boundary_workspace_bytes": (_sz, [_sz]),
    "ru_boundary_sum": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "ru_boundary_grad": (_i, [_vp, _sz, _f, _vp, _vp, _vp]),
    "ru_hddt_sum": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _vp, _vp, _sz, _vp]),
    "ru_hddt_grad": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _vp, _vp, _vp]),
    "ru_lesion_loss_workspace_bytes": (_sz, [_i] * 5),
    "ru_lesion_loss_state_bytes": (_sz, [_i] * 5 + [C.POINTER(_sz)]),
    "ru_lesion_loss_forward": (_i, [_vp, _vp] + [_i] * 6 + [C.c_longlong, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ru_lesion_loss_forward_upto": (_i, [_vp, _vp] + [_i] * 6 + [C.c_longlong, _vp, _vp, _vp, _vp, _vp, _sz, _i, _vp]),
    "ru_lesion_loss_grad": (_i, [_vp, _vp, _vp, _vp, _vp, _d, _vp, _vp] + [_i] * 5 + [_vp]),
    "ru_adam_amsgrad_step": (_i, [_vp] * 5 + [_sz] + [_f] * 5 + [_i, _vp]),
    "ru_adam_step": (_i, [_vp] * 5 + [_sz] + [_f] * 5 + [_i, _vp]),
    "ru_gradnorm_slots": (_sz, [_sz]),
    "ru_gradnorm_workspace_bytes": (_sz, [_sz, _sz]),
    "ru_gradnorm_partial": (_i, [_vp, _sz, _sz, _vp, _sz, _vp]),
    "ru_gradnorm_finalize": (_i, [_vp, _sz, _d, _vp, _vp, _vp]),
    "ru_scale_by": (_i, [_vp, _sz, _vp, _vp]),
    "ru_sgd_step": (_i, [_vp, _vp, _vp, _sz, _f, _f, _f, _f, _i, _i, _vp, _vp]),
    "ru_adamw_step": (_i, [_vp] * 5 + [_sz] + [_f] * 5 + [_i, _i, _vp, _vp]),
    "ru_ema_update": (_i, [_vp, _vp, _sz, _f, _vp]),
    "ru_swap_f32": (_i, [_vp, _vp, _sz, _vp]),
    "ru_unet_create": (_vp, [_i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i]),
    "ru_unet_destroy": (None, [_vp]),
    "ru_unet_set_precision": (_i, [_vp, _i]),
    "ru_unet_freeze_params": (_i, [_vp, _i]),
    "ru_unet_get_precision": (_i, [_vp]),
    "ru_unet_set_grad_precision": (_i, [_vp, _i]),
    "ru_unet_get_grad_precision": (_i, [_vp]),
    "ru_unet_set_fusion": (_i, [_vp, C.c_uint]),
    "ru_unet_probe": (_i, [_vp, _i]),
    "ru_unet_probe_read": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    "ru_unet_probe_read_families": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i), _i]),
    "ru_unet_param_count": (_i, [_vp]),
    "ru_unet_param_name": (C.c_char_p, [_vp, _i]),
    "ru_unet_param_ndim": (_i, [_vp, _i]),
    "ru_unet_param_dim": (_i, [_vp, _i, _i]),
    "ru_unet_param_offset": (_sz, [_vp, _i]),
    "ru_unet_param_total": (_sz, [_vp]),
    "ru_unet_param_is_dead": (_i, [_vp, _i]),
    "ru_unet_workspace_bytes": (_sz, [_vp] + [_i] * 5),
    "ru_unet_forward": (_i, [_vp, _vp, _vp, _vp] + [_i] * 5 + [_vp, _sz, _vp]),
    "ru_unet_backward": (_i, [_vp] * 6),
    "ru_unet_backward_criterion": (_i, [_vp, _vp, _vp, _vp, _d, _f, _f, _f, _f, _vp, _vp, _vp]),
    "ru_unet_gn_stats": (_i, [_vp, _i, _vp, _vp, _vp]),
    "ru_comm_unique_id": (_i, [_vp]),
    "ru_comm_init": (_i, [C.POINTER(_vp), _vp, _i, _i]),
    "ru_comm_destroy": (_i, [_vp]),
    "ru_comm_rank": (_i, [_vp]),
    "ru_comm_world": (_i, [_vp]),
    "ru_allreduce": (_i, [_vp, _vp, _sz, _i, _vp]),
    "ru_comm_group_begin": (_i, []),
    "ru_comm_group_end": (_i, []),
    "ru_tta_merge": (_i, [_vp, _i, C.c_uint, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "ru_compose_labels": (_i, [_vp, _vp, C.c_ulonglong, _vp, _sz, _vp]),
    "ru_dice_counts": (_i, [_vp, _vp, _vp, _i, _i, _sz, _vp]),
    "ru_dice_accumulate": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "ru_hausdorff_workspace_bytes": (_sz, [_i] * 6),
    "ru_hausdorff_sq": (_i, [_vp, _vp] + [_i] * 6 + [_vp, _vp, _sz, _vp]),
    "ru_hausdorff_accumulate": (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    "ru_label_confusion": (_i, [_vp, _vp, _i, _i, _i, _sz, _vp, _vp, _vp]),
    "ru_overlap_accumulate": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "ru_dice1d_accumulate": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "ru_rmse_accumulate": (_i, [_vp, _vp, _vp]),
    "ru_calib_histogram": (_i, [_vp, _vp, _i, _i, _i, _sz, _i, _vp, _vp, _vp, _vp, _vp]),
    "ru_calib_accumulate": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ru_calib_summary": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ru_threshold_regions": (_i, [_vp, _i, _sz, C.POINTER(_f), _vp, _vp, _vp]),
    "ru_surface_workspace_bytes": (_sz, [_i] * 6),
    "ru_surface_metrics": (_i, [_vp, _vp] + [_i] * 6 + [_d, _vp, _vp, _vp, _sz, _vp]),
    "ru_surface_accumulate": (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    "ru_lesion_workspace_bytes": (_sz, [_i] * 7),
    "ru_lesion_metrics": (_i, [_vp, _vp] + [_i] * 7 + [C.c_longlong, _d, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "ru_lesion_accumulate": (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    "ru_surface_distances": (_i, [_vp, _vp] + [_i] * 6 + [_d, C.POINTER(C.c_uint), _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ru_surface_extras_accumulate": (_i, [_vp, _vp] + [_i] * 5 + [_vp]),
    "ru_lesion_distances_workspace_bytes": (_sz, [_i] * 8),
    "ru_lesion_distances": (_i, [_vp, _vp] + [_i] * 7 + [C.c_longlong, _d, C.POINTER(C.c_uint), _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "ru_tile_gather": (_i, [_vp, _vp] + [_i] * 6 + [C.POINTER(_i), _i, _i, _i, _vp]),
    "ru_tile_scatter": (_i, [_vp, _vp] + [_i] * 6 + [C.POINTER(_i), _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_blend_accumulate": (_i, [_vp, _vp, _vp] + [_i] * 8 + [C.POINTER(_i), _i, C.POINTER(_i), _i, C.POINTER(_i), _i, _i, _i, _vp]),
    "ru_blend_finalize": (_i, [_vp, _vp, _vp] + [_i] * 8 + [C.POINTER(_i), _i, C.POINTER(_i), _i, C.POINTER(_i), _i, _vp]),
    "ru_case_bbox": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ru_case_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ru_case_stats": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp, _sz, _vp]),
    "ru_case_prepare": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i, C.c_uint, _vp]),
    "ru_tta_merge_box": (_i, [_vp, _i, C.c_uint, _vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_cc_workspace_bytes": (_sz, [_i, _i, _i]),
    "ru_cc_reject": (_i, [_vp, _i, _i, _i, _d, _vp, _sz, _vp]),
    "ru_paste_labels": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_postprocess_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ru_postprocess_regions": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong), C.c_uint, C.c_uint, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ru_ens_accumulate": (_i, [_vp, _i, C.c_uint, _vp, _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_ens_finalize": (_i, [_vp, _i, _vp, _vp, _vp, _i, _sz, _vp]),
    "ru_ens_accumulate_finalize": (_i, [_vp, _i, C.c_uint, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_ens_argmax": (_i, [_vp, _i, _vp, _i, _sz, _vp]),
    "ru_paste_probs": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_unc_accumulate": (_i, [_vp, _i, C.c_uint, _vp, _vp, _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_unc_accumulate_finalize": (_i, [_vp, _i, C.c_uint, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_unc_finalize": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _sz, _vp]),
    "ru_unc_histogram": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ru_unc_score": (_i, [_vp, C.POINTER(_i), _i, _vp, _vp, _vp]),
    "ru_paste_u8c": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), _vp]),
    "ru_zscore_workspace_bytes": (_sz, [_i, _sz]),
    "ru_zscore_stats": (_i, [_vp, _vp, _i, _sz, _vp, _sz, _vp]),
    "ru_augment_patch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "ru_augment_patch_soft": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "ru_augment_patch_affine": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "ru_case_probe": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ru_case_pack": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "ru_case_unpack": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ru_augment_batch_packed": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "ru_elastic_workspace_bytes": (_sz, [_i, _i, _i]),
    "ru_elastic_noise": (_i, [C.c_ulonglong, _i, _i, _i, _vp, _vp]),
    "ru_elastic_field": (_i, [_vp, _d, _d, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ru_elastic_warp": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "ru_intensity_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "ru_intensity_augment": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ru_carvemix_workspace_bytes": (_sz, [_i, _sz]),
    "ru_carvemix_threshold": (_i, [_vp, _i, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ru_carvemix_mix": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ru_layout_convert":(_i, [_vp, _vp, _i, _i, _sz, _i, _vp]),
    "ru_upsample2x_trilinear_fwd_l": (_i, [_vp, _vp] + [_i] * 5 + [_f, _vp]),
    "ru_upsample2x_trilinear_bwd_l": (_i, [_vp, _vp] + [_i] * 5 + [_vp]),
    "ru_conv3d_fwd_l": (_i, [_vp, _vp, _vp, _vp] + [_i] * 7 + [_vp, _sz, _vp]),
    "ru_conv3d_bwd_weight_l": (_i, [_vp, _vp, _vp] + [_i] * 7 + [_vp, _sz, _vp]),
    "ru_conv1_l_workspace_bytes": (_sz, [_i, _i, _i]),
    "ru_conv1_l": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _f, _vp, _f, _i, _i, _sz, _i, _i, _i, _i, _vp, _vp, _f, _vp, _sz,
                        C.POINTER(_i), C.POINTER(_i), _vp, _sz, _vp]),
    "ru_conv3_l_workspace_bytes": (_sz, [_i] * 7),
    "ru_conv3_l": (_i, [_vp, _vp, _vp, _vp] + [_i] * 8 + [_vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp, _vp, _f, _vp, _sz, C.POINTER(_i), C.POINTER(_i), _vp, _sz, _vp, _vp]),
    "ru_gn_finalize_l": (_i, [_vp, _i] + [_vp] * 7 + [_i, _i, _sz, _i, _f, _i, _vp]),
    "ru_gn_apply_l": (_i, [_vp] * 7 + [_i, _i, _sz, _f, _f, _vp]),
    "ru_gn_bwd_finalize_l": (_i, [_vp, _i] + [_vp] * 6 + [_i, _i, _sz, _i, _i, _vp]),
    "ru_gn_bwd_l_nblk": (_i, [_sz]),
    "ru_gn_bwd_l_workspace_bytes": (_sz, [_i, _i, _sz]),
    "ru_gn_bwd_l": (_i, [_vp] * 7 + [_f] + [_vp] * 5 + [_i, _i, _sz, _i, _i, _vp, _sz, _vp]),
    "ru_head_grad_l_workspace_bytes": (_sz, [_i, _i, _sz, _i]),
    "ru_head_grad_l": (_i, [_vp] * 4 + [_d, _f, _f, _f, _f] + [_vp] * 3 + [_i, _i, _sz, _i, _vp, _sz, _vp]),
    "ru_wgrad1_l_workspace_bytes": (_sz, [_i, _i, _i, _sz]),
    "ru_wgrad3_l_workspace_bytes": (_sz, [_i] * 7),
    "ru_wgrad3_l": (_i, [_vp, _vp, _vp] + [_i] * 8 + [_vp, _vp, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, C.POINTER(_i), _vp, _sz, _vp]),
    "ru_wgrad1_l": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _sz] + [_i] * 6 + [_vp, _i, _vp, _vp, _f, C.POINTER(_i), _vp, _sz, _vp]),
}


# ru_crit_* (include/resunet_hip.h): term kinds, moment indices, the term struct
CRIT_KINDS = {"Dice_loss_joint": 0, "BCE_Loss": 1, "MSE_Loss": 2, "CE_Loss": 3, "Dice1D": 4, "GDL_joint": 5, "sens_loss_joint": 6,
              "Dice_loss_separate": 7}
CRIT_MOMENTS, CRIT_MAX_TERMS = 7, 8
CRIT_MASK_LOGS, CRIT_MASK_ALL = (1 << 4) | (1 << 5), 0x7F
CRIT_M_D2 = 6

# ru_label_confusion / ru_overlap_accumulate (include/resunet_hip.h)
CONF_PROB, CONF_LABEL, OVERLAP_MAX_LABELS = 0, 1, 8
OVERLAP_MODES = {"itk": 0, "wt": 1, "validate": 2}

# ru_calib_* / ru_threshold_regions (include/resunet_hip.h)
CALIB_TARGET_REGIONS, CALIB_TARGET_LABELS = 0, 1
CALIB_MIN_NB, CALIB_MAX_NB, CALIB_DEFAULT_NB, CALIB_MAX_C = 16, 1024, 256, 8

# ru_unc_* (include/resunet_hip.h): measures, histogram extents [regions][levels][TP FP FN TN]
UNC_MEASURES = {"std": 0, "entropy": 1}
UNC_REGIONS, UNC_LEVELS, UNC_CLASSES = 3, 101, 4

# ru_surface_metrics / ru_surface_accumulate (include/resunet_hip.h)
SURFACE_PROB, SURFACE_LABEL, SURFACE_REGIONS, SURFACE_COUNTS = 0, 1, 3, 6
SURFACE_COLUMNS = {"dice": 0, "sensitivity": 1, "specificity": 2, "hd95": 3}

# ru_lesion_metrics / ru_lesion_accumulate (include/resunet_hip.h)
LESION_COUNTS, LESION_TABLE_COLUMNS, LESION_CHUNK = 6, 5, 8
LESION_COLUMNS = {"dice": 0, "hd95": 1}

# ru_surface_distances / ru_lesion_distances (include/resunet_hip.h): at most SURFACE_MAX_TOL tolerances per call.  For T tolerances the
# extras' rows are (NSD_0 .. NSD_T-1, ASSD, HD) and the lesion-wise summary's (LesionNSD_0 .. LesionNSD_T-1, LesionASSD).
SURFACE_MAX_TOL = 8


def surface_extras_columns(t):
    return dict([("nsd%d" % i, i) for i in range(t)] + [("assd", t), ("hd", t + 1)])


def lesion_extras_columns(t):
    return dict([("nsd%d" % i, i) for i in range(t)] + [("assd", t)])

# ru_postprocess_regions (include/resunet_hip.h)
POSTPROCESS_MASKS, POSTPROCESS_LABELS, POSTPROCESS_REGIONS, POSTPROCESS_STATS = 0, 1, 3, 6


# ru_intensity_augment (include/resunet_hip.h): stage bits and the per-channel parameter block
INT_BLUR, INT_LOWRES, INT_NOISE, INT_BRIGHTNESS, INT_CONTRAST, INT_GAMMA, INT_GAMMA_INVERT, INT_GAMMA_RETAIN = 1, 2, 4, 8, 16, 32, 64, 128
INT_MAXC, INT_MAX_RADIUS = 8, 8


# ru_augment_patch_affine (include/resunet_hip.h): thread mappings
AFFINE_MAPPINGS = {"default": 0, "row": 1, "brick": 2}


# packed cases and the batched gather (include/resunet_hip.h): RU_PACK_*, RU_AUG_*, ru_case_desc, ru_patch_desc
PACK_F32, PACK_U16 = 0, 1
PACK_KINDS = {"float32": PACK_F32, "uint16": PACK_U16}
AUG_ZOOM, AUG_AFFINE = 0, 1
AUG_BATCH_MAX = 8

# ru_carvemix_* (include/resunet_hip.h)
CARVE_SIDES = {"outer": 0, "inner": 1}       # RU_CARVE_OUTER / RU_CARVE_INNER
CARVE_BATCH_MAX, CARVE_MAX_VOXELS = 8, 1 << 27


class FinDesc(C.Structure):
    """ru_fin_desc (include/resunet_hip.h): what a kernel's in-launch tail finalizes, and where to"""
    _fields_ = [("kind", _i), ("G", _i), ("s2_sign", _i), ("keep_ticket", _i), ("eps", _f), ("nblk", _i), ("N", _i), ("C", _i),
                ("gamma", _vp), ("beta", _vp), ("mean", _vp), ("rstd", _vp), ("scale", _vp), ("shift", _vp), ("bst_k", _vp),
                ("coef", _vp), ("dgamma", _vp), ("dbeta", _vp)]


class CaseDesc(C.Structure):
    _fields_ = [("image", _vp), ("label", _vp), ("soft", _vp), ("kind", _i), ("C", _i), ("dims", _i * 3), ("box_lo", _i * 3), ("box_size", _i * 3),
                ("mean", _f * 8), ("inv_std", _f * 8)]


class PatchDesc(C.Structure):
    _fields_ = [("mode", _i), ("flags", _i), ("mapping", _i), ("crop_lo", _i * 3), ("scale", _d * 3), ("matrix", _d * 9), ("offset", _d * 3),
                ("gain", _f * 8), ("bias", _f * 8)]


class IntensityParams(C.Structure):
    _fields_ = [("mask", _i * 8), ("blur_sigma", _d * 8), ("lowres_zoom", _d * 8), ("noise_variance", _d * 8), ("noise_seed", C.c_ulonglong * 8),
                ("brightness", _d * 8), ("contrast", _d * 8), ("gamma", _d * 8)]


class CritTerm(C.Structure):
    _fields_ = [("kind", _i), ("weight", _d), ("priority", _d), ("bg_weight", _d)]


def load():
    """Load the shared library (once).  Raises RuntimeError with the build hint if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libresunet_hip.so not found at %s -- build it with `python -m brats2019_amd.build` "
            "(hipcc, gfx950).  There is no CPU fallback for this path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("RU_LIB_PATH") and not hasattr(lib, name):
            continue                 # A/B timing against an older build: entry points added since are simply absent
        fn = getattr(lib, name)      # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return load().ru_last_error().decode("utf-8", "replace")


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError("libresunet_hip: %s failed (%d): %s" % (what, rc, last_error()))


def require_gpu():
    """The hot path runs on an MI355X or not at all."""
    if not torch.cuda.is_available():
        raise RuntimeError("brats2019_amd: no ROCm GPU visible -- the ResUNet hot path is HIP-only (no CPU fallback)")
    load()


def ptr(t, allow_none=False):
    """Device pointer of a contiguous float32 (or float64 where noted) CUDA tensor."""
    if t is None:
        if allow_none:
            return None
        raise ValueError("null tensor")
    if not t.is_cuda:
        raise RuntimeError("brats2019_amd: expected a ROCm device tensor, got a %s tensor (HIP-only path)" % t.device)
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous (NCDHW)")
    return C.c_void_p(t.data_ptr())


def f32(t):
    if t.dtype != torch.float32:
        raise TypeError("expected float32, got %s" % t.dtype)
    return ptr(t)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)

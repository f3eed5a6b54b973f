"""ctypes binding of libmstg_hip.so (include/mstg_hip.h).  No fallback: without the library every op raises."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSTG_LIB") or os.path.join(HERE, "libmstg_hip.so")  # MSTG_LIB: A/B of two builds in one GPU call

ACT_NONE, ACT_RELU, ACT_LEAKY02, ACT_TANH, ACT_GELU = 0, 1, 2, 3, 4
LOSS_L1, LOSS_MSE = 0, 1


class ConvDesc(C.Structure):
    """mirror of mstg_conv_desc"""
    _fields_ = [(n, C.c_int32) for n in (
        "N", "H", "W", "Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad", "dil", "transposed",
        "x_nchw", "y_nchw", "x_ctot", "x_coff", "y_ctot", "y_coff", "act", "accumulate")]


class F16ConvDesc(C.Structure):
    """mirror of mstg_f16_conv_desc"""
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "N", "H", "W", "Cin", "Ho", "Wo", "Cout", "K", "stride", "pad", "dil", "src_nchw_f32", "dst_nchw", "act")]


class F16PlainDesc(C.Structure):
    """mirror of mstg_f16_plain_desc"""
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "N", "H", "W", "Cin", "Ho", "Wo", "Cout", "K", "src_nchw_f32", "dst_nchw", "act")]


class Style16ConvDesc(C.Structure):
    """mirror of mstg_style16_conv_desc"""
    _fields_ = [(n, C.c_int32) for n in (
        "dtype", "N", "H", "W", "Cin", "Cout", "src_nchw_f32", "dst_nchw_f32", "flip", "relu")]


STYLE16_F16, STYLE16_BF16 = 0, 1


class ImgDesc(C.Structure):
    """mirror of mstg_img_desc"""
    _fields_ = ([("src", C.c_void_p)] + [(n, C.c_int32) for n in (
        "src_h", "src_w", "box_y", "box_x", "box_h", "box_w", "rs_h", "rs_w", "filter", "win_y", "win_x", "win_h", "win_w",
        "dst_y", "dst_x", "fill", "ks_h", "ks_v", "y_first", "irows", "ipitch")] + [(n, C.c_int64) for n in (
            "kk_h", "bounds_h", "kk_v", "bounds_v", "inter_off", "out_off")] + [("grid", C.c_uint64)])


IMG_PASS_H, IMG_PASS_V_TENSOR, IMG_PASS_V_U8 = 0, 1, 2


class PairDesc(C.Structure):
    """mirror of mstg_pair_desc"""
    _fields_ = ([("a", C.c_void_p), ("b", C.c_void_p)] + [(n, C.c_int32) for n in ("ha", "wa", "hb", "wb", "tile0", "ntiles")] +
                [("table_v", C.c_int64), ("table_h", C.c_int64)])


PAIR_METRICS_LAUNCHES = 2  # MSTG_PAIR_METRICS_LAUNCHES

_vp, _fp, _sz, _i, _f = C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float
_dp = C.POINTER(ConvDesc)
_hp = C.POINTER(F16ConvDesc)
_pp = C.POINTER(F16PlainDesc)
_sp = C.POINTER(Style16ConvDesc)

# name -> (restype, argtypes); the test-suite checks that every symbol declared in include/mstg_hip.h is here
SIGNATURES = {
    "mstg_version": (C.c_char_p, []),
    "mstg_arch": (C.c_char_p, []),
    "mstg_last_error": (C.c_char_p, []),
    "mstg_env_refresh": (None, []),
    "mstg_prof_enable": (_i, [_i]),
    "mstg_prof_count": (_i, []),
    "mstg_prof_get": (_i, [_i, C.c_char_p, _sz, C.POINTER(C.c_float)]),
    "mstg_conv2d_kernel_name": (C.c_char_p, [_dp, _i]),
    "mstg_msblock_kernel_name": (C.c_char_p, [_i] * 6),
    "mstg_window_attn_kernel_name": (C.c_char_p, [_i] * 4),
    "mstg_conv2d_workspace_bytes": (_sz, [_dp]),
    "mstg_conv2d_fwd": (_i, [_dp, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_conv2d_dgrad": (_i, [_dp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_conv2d_dgrad_bsums_supported": (_i, [_dp]),
    "mstg_conv2d_dgrad_bsums_workspace_bytes": (_sz, [_dp]),
    "mstg_conv2d_dgrad_bsums": (_i, [_dp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _sz, _i, _vp]),
    "mstg_conv2d_fwd_cached": (_i, [_dp, _fp, _fp, _fp, _fp, _vp, _sz, _i, _vp]),
    "mstg_conv2d_fwd_norm_cached": (_i, [_dp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _sz, _i, _vp]),
    "mstg_conv2d_dgrad_cached": (_i, [_dp, _fp, _fp, _fp, _vp, _sz, _i, _vp]),
    "mstg_msblock_fwd_cached": (_i, [_fp] * 10 + [_i, _i, _i, _i, _vp, _sz, _i, _vp]),
    "mstg_msblock_dgrad_cached": (_i, [_fp] * 7 + [_i, _i, _i, _i, _vp, _sz, _i, _vp]),
    "mstg_conv2d_wgrad_workspace_bytes": (_sz, [_dp]),
    "mstg_conv2d_wgrad": (_i, [_dp, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_norm_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_norm_act_fwd": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_norm_act_bwd": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_norm_workspace_bytes_plan": (_sz, [_i, _i, _i, _i]),
    "mstg_norm_act_fwd_plan": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_norm_act_bwd_plan": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_conv2d_group_max": (_i, []),
    "mstg_conv2d_grouped_workspace_bytes": (_sz, [_dp, _i]),
    "mstg_conv2d_fwd_grouped": (_i, [_dp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mstg_conv2d_dgrad_grouped": (_i, [_dp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mstg_conv2d_grouped_kernel_name": (C.c_char_p, [_dp, _i]),
    "mstg_window_attn_core_fwd": (_i, [_fp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_window_attn_core_bwd": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_window_attn_ws_supported": (_i, [_i, _i]),
    "mstg_window_attn_ws_fwd": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "mstg_window_attn_ws_bwd": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "mstg_window_attn_fused_supported": (_i, [_i]),
    "mstg_window_attn_fwd": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_window_attn_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mstg_conv2d_wgrad_norm_supported": (_i, [_dp]),
    "mstg_conv2d_wgrad_norm": (_i, [_dp, _fp, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_conv2d_fwd_norm_supported": (_i, [_dp]),
    "mstg_conv2d_fwd_stats_pays": (_i, [_dp]),
    "mstg_conv2d_fwd_norm_workspace_bytes": (_sz, [_dp]),
    "mstg_conv2d_fwd_norm": (_i, [_dp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_window_attn_norm_fwd": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_window_attn_norm_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mstg_window_attn_norm_bwd": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_norm_apply_fwd": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_norm_stats": (_i, [_fp, _fp, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_norm_bwd_apply": (_i, [_fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _i, _vp]),
    "mstg_window_attn_norm_sums_split": (_i, []),
    "mstg_window_attn_bwd_direct": (_i, [_fp] * 11 + [_i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_window_attn_norm_bwd_direct": (_i, [_fp] * 12 + [_i, _fp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_window_attn_bwd": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_act_fwd": (_i, [_fp, _fp, _sz, _i, _vp]),
    "mstg_act_bwd": (_i, [_fp, _fp, _fp, _sz, _i, _vp]),
    "mstg_loss_workspace_bytes": (_sz, [_sz]),
    "mstg_loss_mean_fwd": (_i, [_fp, _fp, _f, _sz, _i, _fp, _vp, _sz, _vp]),
    "mstg_loss_mean_bwd": (_i, [_fp, _fp, _f, _sz, _i, _fp, _f, _fp, _fp, _vp]),
    "mstg_channel_sum_workspace_bytes": (_sz, [_sz, _i]),
    "mstg_channel_sum": (_i, [_fp, _sz, _i, _i, _i, _f, _fp, _vp, _sz, _vp]),
    "mstg_plane_sum_workspace_bytes": (_sz, [_i, _i, _sz]),
    "mstg_plane_sum": (_i, [_fp, _i, _i, _sz, _f, _fp, _vp, _sz, _vp]),
    "mstg_segment_mean_fwd": (_i, [_fp, _i, _sz, _i, _fp, _vp]),
    "mstg_segment_mean_bwd": (_i, [_fp, _i, _sz, _i, _fp, _vp]),
    "mstg_maxpool2x2_fwd": (_i, [_fp, _fp, _vp, _i, _i, _i, _i, _vp]),
    "mstg_maxpool2x2_bwd": (_i, [_fp, _vp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_gram_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_gram_fwd": (_i, [_fp, _fp, _i, _i, _i, _f, _vp, _sz, _vp]),
    "mstg_gram_bwd": (_i, [_fp, _fp, _fp, _i, _i, _i, _f, _vp]),
    "mstg_adam_step_flat": (_i, [_fp, _fp, _fp, _fp, _sz, _f, _f, _f, _f, _i, _vp, _vp]),
    "mstg_msblock_fused_supported": (_i, [_i]),
    "mstg_msblock_fwd_workspace_bytes": (_sz, [_i]),
    "mstg_msblock_fwd": (_i, [_fp] * 10 + [_i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_msblock_dgrad_workspace_bytes": (_sz, [_i]),
    "mstg_msblock_dgrad": (_i, [_fp] * 7 + [_i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_msblock_wgrad_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mstg_msblock_wgrad": (_i, [_fp] * 10 + [_i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_spectral_norm_workspace_bytes": (_sz, [_i, _i]),
    "mstg_spectral_norm_fwd": (_i, [_fp] * 7 + [_i, _i, _f, _i, _vp, _sz, _vp]),
    "mstg_spectral_norm_bwd": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_spectral_norm_group_max": (_i, []),
    "mstg_spectral_norm_group_workspace_bytes": (_sz, [_i, _vp, _vp]),
    "mstg_spectral_norm_group_fwd": (_i, [_i, _vp, _vp, _vp, _vp, _fp, _vp, _vp, _vp, _vp, _f, _i, _vp, _sz, _vp]),
    "mstg_spectral_norm_group_bwd": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mstg_f16_conv_plan_bytes": (_sz, [_hp]),
    "mstg_f16_conv_pack": (_i, [_hp] + [_fp] * 8 + [_vp, _sz, _vp]),
    "mstg_f16_conv_partial_bytes": (_sz, [_hp]),
    "mstg_f16_conv_fwd": (_i, [_hp, _vp, _vp, _fp, _vp, _fp, _vp, _sz, _vp]),
    "mstg_f16_conv_fwd_res": (_i, [_hp, _vp, _vp, _fp, _vp, _vp, _fp, _vp, _sz, _vp]),
    "mstg_f16_norm_residual": (_i, [_vp, _vp, _fp, _vp, _i, _i, _i, _vp]),
    "mstg_f16_attn_plan_bytes": (_sz, [_i]),
    "mstg_f16_attn_pack": (_i, [_fp, _fp, _fp, _fp, _i, _vp, _sz, _vp]),
    "mstg_f16_attn_fwd": (_i, [_vp, _fp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mstg_f16_plain_plan_bytes": (_sz, [_pp]),
    "mstg_f16_plain_pack": (_i, [_pp, _fp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_f16_plain_fwd": (_i, [_pp, _vp, _vp, _vp, _vp]),
    "mstg_f16_train_image_nhwc8": (_i, [_fp, _vp, _i, _i, _i, _vp]),
    "mstg_f16_train_bn_workspace_bytes": (_sz, [_sz, _i]),
    "mstg_f16_train_bn_fwd": (_i, [_vp, _fp, _fp, _sz, _i, _i, _f, _f, _fp, _fp, _fp, _fp, _vp, _vp, _sz, _vp]),
    "mstg_f16_train_bn_bwd": (_i, [_vp, _vp, _fp, _fp, _fp, _fp, _sz, _i, _i, _fp, _fp, _fp, _vp, _vp, _sz, _vp]),
    "mstg_f16_train_act_bwd": (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    "mstg_f16_train_loss_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_f16_train_head_loss_bwd": (_i, [_vp, _fp, _fp, _i, _i, _i, _fp, _fp, _vp, _vp, _sz, _vp]),
    "mstg_f16_train_wgrad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "mstg_f16_train_wgrad": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _fp, _fp, _vp, _sz, _vp]),
    "mstg_f16_train_bias_grad": (_i, [_vp, _sz, _i, _i, _fp, _fp, _vp, _sz, _vp]),
    "mstg_f16_train_scale_update": (_i, [_fp, _fp, _vp, _vp]),
    "mstg_f16_train_adam": (_i, [_fp, _fp, _fp, _fp, _sz, _f, _f, _f, _f, _i, _vp, _vp]),
    "mstg_style16_conv_plan_bytes": (_sz, [_sp]),
    "mstg_style16_conv_kernel_name": (C.c_char_p, [_sp]),
    "mstg_style16_conv_pack": (_i, [_sp, _fp, _fp, _vp, _sz, _vp]),
    "mstg_style16_conv_fwd": (_i, [_sp, _vp, _vp, _vp, _vp, _vp]),
    "mstg_style16_maxpool_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mstg_style16_maxpool_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mstg_style16_gram_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_style16_gram_fwd": (_i, [_vp, _fp, _i, _i, _i, _f, _vp, _sz, _vp]),
    "mstg_style16_gram_bwd_workspace_bytes": (_sz, [_i, _i]),
    "mstg_style16_gram_bwd": (_i, [_vp, _fp, _vp, _vp, _i, _i, _i, _f, _vp, _sz, _vp]),
    "mstg_f16_linear_plan_bytes": (_sz, [_i, _i]),
    "mstg_f16_linear_pack": (_i, [_fp, _fp, _i, _i, _vp, _sz, _vp]),
    "mstg_f16_linear_fwd": (_i, [_vp, _vp, _fp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mstg_f16_ln_mod_fwd": (_i, [_vp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _i, _i, _i, _f, _vp]),
    "mstg_f16_token_mean_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_f16_token_mean": (_i, [_vp, _fp, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_f16_flash_attn_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "mstg_f16_attn_cast_qkv": (_i, [_fp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mstg_f16_flash_attn_train_fwd": (_i, [_vp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_f16_flash_attn_train_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mstg_f16_flash_attn_train_bwd": (_i, [_vp, _vp, _fp, _fp, _fp, _vp, _sz, _i, _i, _i, _i, _vp]),
    "mstg_add": (_i, [_fp, _fp, _fp, _sz, _vp]),
    "mstg_weighted_sum_fwd": (_i, [C.POINTER(C.c_void_p), C.POINTER(C.c_float), _i, _i, _fp, _vp]),
    "mstg_weighted_sum_bwd": (_i, [_fp, C.POINTER(C.c_float), _i, _fp, _vp]),
    "mstg_masked_l1_mean_fwd": (_i, [_fp, _fp, _fp, _sz, _fp, _vp, _sz, _vp]),
    "mstg_masked_l1_mean_bwd": (_i, [_fp, _fp, _fp, _sz, _fp, _fp, _vp]),
    "mstg_clip_grad_norm": (_i, [_fp, _sz, _f, _fp, _vp, _sz, _vp]),
    "mstg_structure_map": (_i, [_fp, _fp, _i, _i, _i, _vp]),
    "mstg_ln_mod_fwd": (_i, [_fp] * 7 + [_i, _i, _i, _f, _vp]),
    "mstg_ln_mod_bwd_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_ln_mod_bwd": (_i, [_fp] * 11 + [_i, _i, _i, _i, _vp, _sz, _vp]),
    "mstg_flash_attn_fwd": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_flash_attn_bwd": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp]),
    "mstg_resample_ksize": (_i, [_i, _i, _i]),
    "mstg_resample_coeffs": (_i, [_i, _i, _i, _vp, _vp]),
    "mstg_resample_h_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mstg_resample_v_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "mstg_paste_u8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "mstg_u8_to_tensor": (_i, [_vp, _i, _i, _i, _i, _i, _i, _fp, _fp, _fp, C.c_ulonglong, _i, _vp]),
    "mstg_tensor_to_u8": (_i, [_fp, _i, _i, _vp, _vp]),
    "mstg_blend_u8": (_i, [_vp, _vp, C.c_double, C.c_double, _vp, _vp, _i, _i, _vp]),
    "mstg_img_batch_validate": (_i, [_vp, _i, _vp, _sz, _sz, _i, _sz]),
    "mstg_img_batch_tiles": (_i, [_vp, _i, _vp, _sz, _i, _i, _vp, _sz]),
    "mstg_img_batch_resample_h": (_i, [_vp, _i, _vp, _sz, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "mstg_img_batch_resample_v_tensor": (_i, [_vp, _i, _vp, _sz, _vp, _vp, _i, _vp, _vp, _sz, _i, _fp, _fp, _fp, _vp, _i, _vp]),
    "mstg_img_batch_resample_v_u8": (_i, [_vp, _i, _vp, _sz, _vp, _vp, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "mstg_img_batch_tensor_to_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "mstg_image_metrics_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_image_metrics_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mstg_cv_resize_coeffs": (_i, [_i, _i, _i, _vp, _vp]),
    "mstg_cv_resize_linear_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "mstg_pair_metrics_validate": (_i, [_vp, _i, _vp, _sz]),
    "mstg_pair_metrics_workspace_bytes": (_sz, [_vp, _i]),
    "mstg_pair_metrics_tiles": (_i, [_vp, _i, _vp, _sz]),
    "mstg_pair_metrics_u8": (_i, [_vp, _i, _vp, _sz, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "mstg_local_style_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_local_style_prepare": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mstg_local_style_hysteresis": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mstg_local_style_weights": (_i, [_vp, _vp, _vp, _i, _i, _i, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp]),
    "mstg_local_style_weight_map": (_i, [_vp, _i, _i, _i, C.c_double, C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "mstg_local_style_finish": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "mstg_local_style_enhanced_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_local_style_enhanced": (_i, [_vp, _vp, _i, _i, _i, C.c_double, C.c_double, C.c_double, _i, _i, _vp, _vp, _sz, _vp]),
    "mstg_bilateral_tables": (_i, [_i, C.c_double, C.c_double, _vp]),
    "mstg_standard_color_lut": (_i, [_i, _vp]),
    "mstg_median3_u8": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mstg_bilateral_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mstg_lut_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "mstg_gaussian_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "mstg_standard_finish_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_standard_finish": (_i, [_vp, _vp, _i, _i, _i, C.c_double, C.c_double, _i, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "mstg_gaussian_kernel_f64": (_i, [_i, C.c_double, _vp]),
    "mstg_app_sky_mask": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mstg_app_edge_weight": (_i, [_vp, _i, _i, _i, _vp, C.c_double, _vp, _vp]),
    "mstg_app_chain": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, C.c_double, C.c_double, _vp, _vp, _vp]),
    "mstg_app_local_style_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_app_local_style_finish": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp,
                                         _sz, _vp]),
    "mstg_lab_tables": (_i, [_vp]),
    "mstg_bilateral_wide_tables": (_i, [_i, C.c_double, C.c_double, _vp]),
    "mstg_color_block_mask": (_i, [_vp, _i, _i, _i, _vp, _f, _i, _vp, _vp, _sz, _vp]),
    "mstg_color_correct_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mstg_bilateral_wide_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mstg_detail_blend_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, C.c_double, C.c_double, C.c_double, _vp, _vp, _sz, _vp]),
    "mstg_color_block_fix_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mstg_color_block_fix": (_i, [_vp, _vp, _i, _i, _i, _vp, _f, _i, _i, _i, _vp, _vp, _i, C.c_double, C.c_double, C.c_double, _vp, _vp,
                                  _sz, _vp]),
    "mstg_segment_blend_map_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "mstg_segment_blend_map": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mstg_gaussian_reflect_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mstg_blend_map_f32_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "mstg_clahe_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_clahe_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mstg_hsv_enhance_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mstg_sharpen3_u8": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mstg_enhanced_style_finish_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_enhanced_style_finish": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "mstg_felzenszwalb_u8": (_i, [_vp, _i, _i, C.c_double, C.c_double, _i, _vp]),
    "mstg_slic_grid": (_i, [_i, _i, _i, _vp, _vp, _vp]),
    "mstg_slic_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mstg_slic_u8": (_i, [_vp, _i, _i, _i, _i, C.c_double, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mstg_slic_assign_u8": (_i, [_vp, _i, _i, _i, _i, C.c_double, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mstg_connect_labels_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_connect_labels": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "mstg_quickshift_workspace_bytes": (_sz, [_i, _i, _i, C.c_double]),
    "mstg_quickshift_density_u8": (_i, [_vp, _i, _i, _i, C.c_double, C.c_double, _vp, _vp, _vp]),
    "mstg_quickshift_parents_u8": (_i, [_vp, _vp, _i, _i, _i, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp]),
    "mstg_quickshift_u8": (_i, [_vp, _i, _i, _i, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mstg_lab_inverse_tables": (_i, [_vp]),
    "mstg_gaussian_sigma_taps": (_i, [C.c_double, _vp, _vp]),
    "mstg_lab_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "mstg_lab2rgb_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "mstg_gaussian_sigma_u8": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "mstg_hsv_gain_u8": (_i, [_vp, _i, _i, _i, _f, _f, _vp, _vp]),
    "mstg_kmeans_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_kmeans_u8": (_i, [_vp, _i, _i, _i, _i, _i, _i, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mstg_region_blend_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "mstg_region_blend_gain_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _f, _f, _vp, _vp]),
    "mstg_fuse_scales_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _f, _vp, _vp]),
    "mstg_contrast_enhanced_finish_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_contrast_enhanced_finish": (_i, [_vp, _i, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _sz, _vp]),
    "mstg_detail_enhanced_finish": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f, _vp, _vp, _sz, _vp]),
    "mstg_frechet_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_frechet_distance": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "mstg_singular_values_workspace_bytes": (_sz, [_i, _i]),
    "mstg_singular_values": (_i, [_vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "mstg_gamma_u8": (_i, [_vp, _i, _i, _i, _i, C.c_double, _vp, _vp]),
    "mstg_equalize_luma_workspace_bytes": (_sz, [_i, _i, _i]),
    "mstg_equalize_luma_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
}

FRECHET_MAX_SAMPLES, FRECHET_MAX_SWEEPS = 256, 44  # MSTG_FRECHET_MAX_SAMPLES, MSTG_FRECHET_MAX_SWEEPS
APP_EDGE_KSIZE = 21  # MSTG_APP_EDGE_KSIZE
LOCAL_STYLE_MAX_PIXELS = 147456  # MSTG_LOCAL_STYLE_MAX_PIXELS
BILATERAL_COLOR_WEIGHTS, BILATERAL_MAX_TAPS = 768, 49  # MSTG_BILATERAL_COLOR_WEIGHTS, MSTG_BILATERAL_MAX_TAPS
LAB_TABLE_U16 = 3340  # MSTG_LAB_TABLE_U16
BILATERAL_WIDE_MAX_RADIUS = 90  # MSTG_BILATERAL_WIDE_MAX_RADIUS
BILATERAL_WIDE_TABLE_FLOATS = 768 + 90 * 90 + 1  # MSTG_BILATERAL_WIDE_TABLE_FLOATS
SEGMENT_SUMS, SEGMENT_MAX_PIXELS, SEGMENT_TILE_SLOTS = 11, 1 << 20, 128  # MSTG_SEGMENT_SUMS, _MAX_PIXELS, _TILE_SLOTS
CLAHE_TILES = 8  # MSTG_CLAHE_TILES
SLIC_MAX_CENTRES, SLIC_SUMS = 4096, 6  # MSTG_SLIC_MAX_CENTRES, MSTG_SLIC_SUMS
QUICKSHIFT_MAX_RADIUS = 15  # MSTG_QUICKSHIFT_MAX_RADIUS
LAB_INV_TABLE_U16, GAUSSIAN_SIGMA_MAX_KSIZE = 15696, 31  # MSTG_LAB_INV_TABLE_U16, MSTG_GAUSSIAN_SIGMA_MAX_KSIZE
KMEANS_MAX_K, KMEANS_MAX_ATTEMPTS, KMEANS_MAX_ITERS, FUSE_MAX_SCALES = 16, 16, 100, 8  # MSTG_KMEANS_MAX_*, MSTG_FUSE_MAX_SCALES
STANDARD_MODEL_TYPES = {"photo_to_monet": 0, "monet_to_photo": 1}  # MSTG_STANDARD_PHOTO_TO_MONET, MSTG_STANDARD_MONET_TO_PHOTO

_lib = None


def load() -> C.CDLL:
    """Load the HIP library once.  Raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m mstg_hip.build` (or __graft_entry__.build()). "
                "This package has no CPU or eager-PyTorch fallback.")
        # torch first: it ships its own libamdhip64 / libhsa-runtime64, and this library must bind to THAT runtime (the one that owns
        # torch's device memory and streams).  Loaded before torch, this library pulls in /opt/rocm's copy, the process then holds two
        # HIP runtimes and every launch from here fails with "no ROCm-capable device is detected".
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().mstg_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed with code {rc}: {msg}")

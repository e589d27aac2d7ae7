"""ctypes binding of libunet_hip.so (the C ABI declared in include/unet_hip.h).

The library is built in-tree by `build()` (hipcc, --offload-arch=gfx950) and is
the ONLY compute path of this package: there is no CPU or eager-PyTorch
fallback.  `lib()` raises if the shared object is missing.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# UNET_HIP_LIB selects an alternative in-tree build (A/B experiments of kernel variants)
LIB_PATH = os.environ.get("UNET_HIP_LIB") or os.path.join(_HERE, "libunet_hip.so")
CSRC = os.path.join(_HERE, "csrc")

ABI_VERSION = 11     # UNET_ABI_VERSION of include/unet_hip.h this binding was written against

_c = ctypes
_p = _c.c_void_p
_i = _c.c_int
_f = _c.c_float
_sz = _c.c_size_t
_i64 = _c.c_int64



class ActSrc(ctypes.Structure):
    """`unet_act_src` of include/unet_hip.h: an operand activated on load."""
    _fields_ = [("x", _p), ("C", _i), ("alpha", _p), ("beta", _p)]


_ps = _c.POINTER(ActSrc)


class BwdStats(ctypes.Structure):
    """`unet_bwd_stats` of include/unet_hip.h: the layer whose InstanceNorm-backward reductions a
    data-gradient epilogue emits."""
    _fields_ = [("y", _p), ("mean", _p), ("rstd", _p), ("gamma", _p), ("beta", _p), ("mask", _p),
                ("slope", _f), ("partial", _p), ("partial_bytes", _sz), ("tiles_out", _i)]


_pbs = _c.POINTER(BwdStats)

# name -> (restype, argtypes); mirrors include/unet_hip.h one to one
SIGNATURES = {
    "unet_last_error": (_c.c_char_p, []),
    "unet_abi_version": (_i, []),
    "unet_device_count": (_i, []),
    "unet_debug_set_chunk_limit": (_i, [_i64]),
    "unet_debug_record_launches": (_i, [_i]),
    "unet_debug_recorded_launches": (_sz, [_p, _sz]),
    "unet_nchw_to_nhwc": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "unet_nhwc_to_nchw": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "unet_pack_conv3x3_weights": (_i, [_p, _p, _p, _i, _i, _p]),
    "unet_conv3x3_fwd": (_i, [_p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "unet_conv3x3_bwd_data": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "unet_conv3x3_fwd_bf16": (_i, [_p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "unet_conv3x3_bwd_data_bf16": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "unet_conv1x1_fwd": (_i, [_p, _i, _p, _i, _p, _p, _p, _i, _i, _i, _i, _p]),
    "unet_conv1x1_bwd_data": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p]),
    "unet_conv1x1_bwd_weight": (_i, [_p, _i, _p, _p, _i, _i, _p, _sz, _i, _i, _i, _i, _p]),
    "unet_transpose2d": (_i, [_p, _p, _i, _i, _p]),
    "unet_conv3x3_bwd_weight_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "unet_conv3x3_bwd_weight": (_i, [_p, _i, _p, _p, _i, _i, _p, _p, _sz, _i, _i, _i, _i, _i, _p]),
    "unet_conv3x3_bwd_weight_bf16": (_i, [_p, _i, _p, _p, _i, _i, _p, _p, _sz, _i, _i, _i, _i, _i,
                                          _p]),
    "unet_pack_conv3x3_weights_bf16x3": (_i, [_p, _p, _p, _i, _i, _p]),
    "unet_pack_conv3x3_weights_batched": (_i, [_p, _i, _i, _p]),
    "unet_conv3x3_fwd_bf16x3": (_i, [_p, _i, _p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "unet_conv3x3_bwd_data_bf16x3": (_i, [_p, _p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "unet_conv3x3_bwd_weight_bf16x3": (_i, [_p, _i, _p, _p, _i, _i, _p, _p, _sz, _i, _i, _i, _i, _i,
                                          _p]),
    "unet_instnorm_workspace_bytes": (_sz, [_i, _i, _i]),
    "unet_instnorm_stats": (_i, [_p, _p, _p, _f, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_instnorm_lrelu_drop_fwd": (_i, [_p, _p, _p, _p, _f, _p, _i, _i, _i, _p]),
    "unet_instnorm_lrelu_drop_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p, _sz,
                                          _i, _i, _i, _p]),
    "unet_upsample2x_fwd": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "unet_resize_bilinear_fwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "unet_resize_bilinear_bwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "unet_upsample2x_bwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "unet_head1x1_fwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "unet_head1x1_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "unet_head1x1_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _i, _p]),
    "unet_dice_wce_loss_workspace_bytes": (_sz, [_i, _i, _i]),
    "unet_dice_wce_loss_fwd_bwd": (_i, [_p, _p, _p, _p, _p, _sz, _i, _i, _i, _f, _f, _f, _i, _i,
                                        _p, _f, _p]),
    "unet_dice_wce_loss_shard_stats": (_i, [_p, _p, _p, _p, _sz, _i, _i, _i, _f, _i, _p]),
    "unet_dice_wce_loss_shard_apply": (_i, [_p, _p, _p, _i, _p, _p, _p, _sz, _i, _i, _i, _f, _f, _f,
                                            _i, _i, _p, _f, _p]),
    "unet_wgrad_defer_begin": (_i, []),
    "unet_wgrad_defer_pending": (_i, []),
    "unet_wgrad_defer_flush": (_i, [_p]),
    "unet_wgrad_defer_end": (_i, [_p]),
    "unet_dice_wce_loss_grad": (_i, [_p, _p, _p, _sz, _p, _p, _i, _i, _i, _i, _p]),
    "unet_argmax_dice_counts": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "unet_eval_confusion": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "unet_eval_maps": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "unet_render_seg_panels": (_i, [_p, _i, _p, _p, _i, _p, _p, _i, _c.c_uint64, _p, _i, _i, _i, _p]),
    "unet_render_recon_panels": (_i, [_p, _i, _p, _p, _p, _p, _i, _i, _i, _p]),
    "unet_letterbox_u8": (_i, [_p, _sz, _p, _i, _i, _i, _p, _p, _p, _p]),
    "unet_byte_histogram_u8": (_i, [_p, _sz, _p, _i, _p, _p]),
    "unet_augment_params_per_sample": (_i, []),
    "unet_augment_u8": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "unet_augment_warp_params_per_sample": (_i, []),
    "unet_augment_warp_u8": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "unet_elastic_field": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "unet_augment_post_params_per_sample": (_i, []),
    "unet_augment_post_workspace_bytes": (_sz, [_i]),
    "unet_augment_post_u8": (_i, [_p, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_augment_post_hist": (_i, [_p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_augment_post_apply": (_i, [_p, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_augment_light_params_per_sample": (_i, []),
    "unet_augment_light_workspace_bytes": (_sz, [_i]),
    "unet_augment_light_u8": (_i, [_p, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_augment_light_stats": (_i, [_p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_augment_light_apply": (_i, [_p, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_gradcam_workspace_bytes": (_sz, [_i, _i, _i]),
    "unet_gradcam_weights": (_i, [_p, _i, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_gradcam_map": (_i, [_ps, _i, _f, _p, _p, _p, _sz, _i, _i, _p]),
    "unet_gradcam_heatmap": (_i, [_p, _p, _sz, _p, _i, _i, _i, _i, _i, _p]),
    "unet_preprocess_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _c.POINTER(_f), _c.POINTER(_f), _p]),
    "unet_sgd_nesterov_step": (_i, [_p, _p, _p, _i64, _f, _f, _f, _i, _f, _p]),
    "unet_sgd_nesterov_step_dev": (_i, [_p, _p, _p, _i64, _p, _i, _p]),
    "unet_conv_in_fwd_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "unet_conv_in_fwd": (_i, [_ps, _ps, _f, _p, _p, _i, _i, _p, _p, _sz, _c.POINTER(_i), _i, _i, _i,
                              _i, _p]),
    "unet_conv_in_fwd_bf16x3": (_i, [_ps, _ps, _f, _p, _p, _p, _i, _i, _p, _p, _sz, _c.POINTER(_i), _i,
                                     _i, _i, _i, _p]),
    "unet_conv_up_in_fwd_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "unet_conv_up_in_fwd": (_i, [_ps, _ps, _f, _p, _p, _p, _p, _sz, _c.POINTER(_i), _i, _i, _i, _i,
                                 _p]),
    "unet_conv_in_stats_finalize": (_i, [_p, _p, _sz, _i, _p, _p, _f, _p, _p, _p, _p, _p, _i, _i, _i,
                                         _p]),
    "unet_stem_u8_fwd": (_i, [_p, _c.POINTER(_f), _c.POINTER(_f), _p, _p, _p, _p, _sz,
                              _c.POINTER(_i), _i, _i, _i, _i, _p]),
    "unet_stem_u8_bwd_weight": (_i, [_p, _c.POINTER(_f), _c.POINTER(_f), _p, _p, _p, _sz, _i, _i,
                                     _i, _i, _p]),
    "unet_conv_in_bwd_weight": (_i, [_ps, _f, _p, _p, _i, _i, _i, _i, _p, _sz, _i, _i, _i, _i, _p]),
    "unet_conv_in_bwd_weight_bf16x3": (_i, [_ps, _f, _p, _p, _i, _i, _i, _i, _p, _sz, _i, _i, _i, _i,
                                            _p]),
    "unet_upsample2x_in_fwd": (_i, [_ps, _f, _p, _i, _i, _i, _p]),
    "unet_conv3x3_bwd_data_bs": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, _pbs, _p]),
    "unet_conv_wino_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "unet_set_c32_winograd": (_i, [_i]),
    "unet_conv_c32_is_winograd": (_i, [_i, _i, _i, _i, _i, _i]),
    "unet_conv_up_c32_is_winograd": (_i, [_i, _i, _i, _i, _i, _i]),
    "unet_wino_weight_floats": (_sz, [_i, _i]),
    "unet_pack_wino_weights": (_i, [_p, _p, _p, _i, _i, _p]),
    "unet_pack_wino_weights_batched": (_i, [_p, _i, _i, _p]),
    "unet_conv_in_fwd_wino": (_i, [_ps, _ps, _f, _p, _p, _p, _p, _sz, _c.POINTER(_i), _i, _i, _i,
                                   _i, _p]),
    "unet_conv3x3_bwd_weight_is_winograd": (_i, [_i, _i, _i, _i, _i, _i]),
    "unet_conv_up_wino_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "unet_conv_up_in_fwd_wino": (_i, [_ps, _ps, _f, _p, _p, _p, _p, _sz, _c.POINTER(_i), _i, _i,
                                      _i, _i, _p]),
    "unet_conv3x3_bwd_data_bs_wino": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _pbs, _p]),
    "unet_conv3x3_bwd_data_bs_b16": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, _pbs, _p]),
    "unet_conv3x3_bwd_data_bs_b16_wb": (_i, [_p, _p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, _pbs,
                                             _p]),
    "unet_conv3x3_bwd_data_bs_bf16x3": (_i, [_p, _p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, _pbs,
                                             _p]),
    "unet_conv3x3_up_bwd_data_bs": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _pbs, _p]),
    "unet_instnorm_lrelu_drop_bwd_partials": (_i, [_p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p,
                                                   _p, _i, _p, _sz, _i, _i, _i, _p]),
    "unet_instnorm_lrelu_drop_bwd_partials_b16": (_i, [_p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p,
                                                       _p, _i, _p, _sz, _i, _i, _i, _p]),
    "unet_conv_in_fwd_b16": (_i, [_ps, _ps, _f, _p, _p, _i, _i, _p, _p, _sz, _c.POINTER(_i), _i, _i,
                                  _i, _i, _p]),
    "unet_conv_in_fwd_b16_wb": (_i, [_ps, _ps, _f, _p, _p, _p, _i, _i, _p, _p, _sz, _c.POINTER(_i),
                                     _i, _i, _i, _i, _p]),
    "unet_conv_in_stats_finalize_b16": (_i, [_p, _p, _sz, _i, _p, _p, _f, _p, _p, _p, _p, _p, _i, _i,
                                             _i, _p]),
    "unet_conv_in_bwd_weight_b16": (_i, [_ps, _f, _p, _p, _i, _i, _i, _i, _p, _sz, _i, _i, _i, _i,
                                         _p]),
    "unet_conv3x3_bwd_data_b16": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "unet_instnorm_lrelu_drop_bwd_b16": (_i, [_p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _p, _p,
                                              _sz, _i, _i, _i, _p]),
    "unet_upsample2x_in_fwd_b16": (_i, [_ps, _f, _p, _i, _i, _i, _p]),
    "unet_upsample2x_bwd_taps_b16": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "unet_conv3x3_up_bwd_weight_b16": (_i, [_ps, _f, _p, _p, _i, _i, _p, _sz, _i, _i, _i, _i, _p]),
    "unet_conv_up_in_fwd_b16_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "unet_conv_up_in_fwd_b16": (_i, [_ps, _ps, _f, _p, _p, _p, _p, _p, _sz, _c.POINTER(_i), _i, _i, _i,
                                     _i, _p]),
    "unet_conv3x3_up_bwd_data_b16": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p]),
    "unet_conv3x3_up_bwd_data_bs_b16": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _pbs, _p]),
    "unet_conv3x3_up_bwd_data_bs_b16_wb": (_i, [_p, _p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _pbs,
                                           _p]),
    "unet_head1x1_in_fwd_b16": (_i, [_ps, _f, _p, _p, _p, _i, _i, _i, _p]),
    "unet_head1x1_in_bwd_b16": (_i, [_ps, _f, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_upsample2x_bwd_taps": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "unet_conv3x3_up_bwd_weight_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "unet_conv3x3_up_bwd_weight": (_i, [_ps, _f, _p, _p, _i, _i, _p, _sz, _i, _i, _i, _i, _p]),
    "unet_conv3x3_up_bwd_data": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p]),
    "unet_head1x1_in_fwd": (_i, [_ps, _f, _p, _p, _p, _i, _i, _i, _p]),
    "unet_head1x1_in_bwd": (_i, [_ps, _f, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_head1x1_in_bwd_bs": (_i, [_ps, _f, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _pbs, _p]),
    "unet_head1x1_in_bwd_bs_b16": (_i, [_ps, _f, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _pbs, _p]),
    "unet_stem_in_bwd_weight_fold_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "unet_stem_in_bwd_weight_fold": (_i, [_p, _p, _c.POINTER(_f), _c.POINTER(_f), _p, _p, _p, _p, _p,
                                          _p, _p, _f, _p, _i, _p, _p, _p, _p, _p, _sz, _i, _i, _i,
                                          _i, _p]),
    "unet_conv_in_bwd_weight_fold32_supported": (_i, [_i, _i, _i, _i, _i]),
    "unet_conv_in_bwd_weight_fold32_workspace_bytes": (_sz, [_i, _i, _i]),
    "unet_conv_in_bwd_weight_fold32": (_i, [_ps, _f, _p, _p, _p, _p, _p, _p, _p, _f, _p, _i, _p, _i,
                                            _i, _p, _p, _p, _p, _sz, _i, _i, _i, _p]),
    "unet_instnorm_bwd_merge_partials": (_i, [_p, _i, _p, _p, _i, _i, _i, _p]),
    "unet_head1x1_in_bwd_fold_workspace_bytes": (_sz, [_i, _i, _i]),
    "unet_head1x1_in_bwd_fold": (_i, [_ps, _f, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i,
                                      _pbs, _p]),
    "unet_recon3x3_fwd": (_i, [_ps, _i, _f, _p, _p, _p, _i, _i, _i, _i, _p]),
    "unet_recon3x3_bwd_workspace_bytes": (_sz, [_i, _i, _i]),
    "unet_recon3x3_bwd": (_i, [_ps, _i, _f, _p, _p, _p, _p, _p, _p, _p, _sz, _i, _i, _i, _i, _pbs,
                               _p]),
    "unet_mse_loss_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "unet_mse_loss_fwd": (_i, [_p, _p, _i, _p, _p, _p, _sz, _i, _i, _i, _i, _p]),
    "unet_mse_loss_grad": (_i, [_p, _p, _i, _p, _p, _i, _i, _i, _i, _p]),
    "unet_adam_step": (_i, [_p, _p, _p, _p, _i64, _p, _i, _p]),
    "unet_ssim_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "unet_ssim_fwd": (_i, [_p, _p, _i, _c.POINTER(_f), _f, _f, _p, _p, _p, _c.c_double,
                           _c.c_double, _p, _sz, _i, _i, _i, _i, _p]),
    "unet_ssim_grad": (_i, [_p, _p, _i, _c.POINTER(_f), _f, _f, _p, _i, _c.c_double, _c.c_double,
                            _p, _i, _i, _i, _i, _p]),
    "unet_perceptual_prep": (_i, [_p, _p, _i, _c.POINTER(_f), _c.POINTER(_f), _p, _i, _i, _i, _p]),
    "unet_relu_maxpool2x2_fwd": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "unet_feature_mse_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "unet_feature_mse_fwd": (_i, [_p, _p, _p, _sz, _i, _i, _i, _i, _p]),
    "unet_perceptual_relu_bwd": (_i, [_p, _p, _f, _p, _p, _p, _i, _i, _i, _i, _p]),
    "unet_perceptual_stem_bwd_data": (_i, [_p, _p, _c.POINTER(_f), _p, _i, _i, _i, _i, _p]),
    "unet_vit_patchify": (_i, [_p, _i, _c.POINTER(_f), _c.POINTER(_f), _p, _i, _i, _i, _i, _i, _i,
                               _p]),
    "unet_vit_gemm_bf16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "unet_vit_tokens_ln": (_i, [_p, _p, _p, _p, _p, _f, _p, _i, _i, _i, _p]),
    "unet_vit_layernorm": (_i, [_p, _p, _p, _f, _p, _i, _i, _p]),
    "unet_vit_attention": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "unet_vit_head": (_i, [_p, _p, _p, _f, _p, _p, _i, _i, _i, _i, _i, _p]),
    "unet_stem_u8_fwd_b16": (_i, [_p, _c.POINTER(_f), _c.POINTER(_f), _p, _p, _p, _p, _sz,
                                  _c.POINTER(_i), _i, _i, _i, _i, _p]),
    "unet_stem_u8_bwd_weight_b16": (_i, [_p, _c.POINTER(_f), _c.POINTER(_f), _p, _p, _p, _sz, _i,
                                         _i, _i, _i, _p]),
}
# the uint8-target twins take the arguments of their int64 forms
for _name in ("unet_dice_wce_loss_fwd_bwd", "unet_dice_wce_loss_grad",
              "unet_dice_wce_loss_shard_stats", "unet_dice_wce_loss_shard_apply",
              "unet_argmax_dice_counts"):
    SIGNATURES[_name + "_u8"] = SIGNATURES[_name]
del _name

_lib = None


class UNetHipError(RuntimeError):
    pass


def build(verbose=False):
    """Compile libunet_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    jobs = str(min(8, os.cpu_count() or 1))
    proc = subprocess.run(["make", "-C", CSRC, "-j", jobs], capture_output=True, text=True)
    if verbose or proc.returncode != 0:
        print(proc.stdout)
        print(proc.stderr)
    if proc.returncode != 0:
        raise UNetHipError("building libunet_hip.so failed (see output above)")
    return LIB_PATH


def lib():
    """Load (once) and return the ctypes handle; raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UNetHipError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU / eager fallback for the HIP path)")
    # torch must be imported first so its bundled libamdhip64.so.7 (same soname) is the
    # one HIP runtime of the process: streams and device pointers are then shared.
    import torch  # noqa: F401
    handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if handle.unet_abi_version() != ABI_VERSION:
        raise UNetHipError("libunet_hip.so ABI version mismatch; rebuild")
    _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().unet_last_error()
        raise UNetHipError(f"libunet_hip error {rc}: {msg.decode() if msg else '?'}")

"""ctypes binding of include/vipcup_hip.h.  Loads the in-tree libvipcup_hip.so and fails loudly if it
is absent (there is deliberately no CPU fallback)."""
import ctypes as C
import os

# torch must load ITS libamdhip64 first: libvipcup_hip.so then binds to that same runtime instance (same
# SONAME), so device pointers and streams are shared.  Loaded the other way round the process ends up with
# two HIP runtimes and every launch fails with "no ROCm-capable device".
import torch  # noqa: F401  (side effect: HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VIP_LIB_PATH") or os.path.join(_HERE, "libvipcup_hip.so")   # VIP_LIB_PATH: kernel A/B builds

_lib = None


class VipError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    """mirror of vip_conv_desc (include/vipcup_hip.h)"""
    _fields_ = [(n, C.c_int) for n in (
        "B", "H", "W", "Cin", "Cout", "kh", "kw", "sh", "sw", "pt", "pl", "Ho", "Wo", "groups",
        "ldx", "cin_off", "ldy", "cout_off", "ldr", "res_off", "ldw", "act_pre", "act_post")]


class JpegDesc(C.Structure):
    """mirror of vip_jpeg_desc (include/vipcup_hip.h)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32),
                ("hsamp", C.c_int32 * 3), ("vsamp", C.c_int32 * 3),
                ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3),
                ("coef_off", C.c_int64 * 3), ("qt", (C.c_uint16 * 64) * 3), ("rgb_coded", C.c_int32)]


class PngDesc(C.Structure):
    """mirror of vip_png_desc (include/vipcup_hip.h)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bit_depth", C.c_int32), ("color_type", C.c_int32),
                ("interlace", C.c_int32), ("channels", C.c_int32), ("bpp", C.c_int32), ("palette_size", C.c_int32),
                ("stream_off", C.c_int64), ("pass_off", C.c_int64 * 7), ("pass_w", C.c_int32 * 7), ("pass_h", C.c_int32 * 7),
                ("palette", (C.c_uint8 * 3) * 256)]


class WebpDesc(C.Structure):
    """mirror of vip_webp_desc (include/vipcup_hip.h)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("has_alpha", C.c_int32), ("coded_width", C.c_int32),
                ("n_transforms", C.c_int32), ("stats", C.c_int32), ("type", C.c_int32 * 4), ("bits", C.c_int32 * 4),
                ("xsize", C.c_int32 * 4), ("stream_off", C.c_int64), ("data_off", C.c_int64 * 4), ("argb_off", C.c_int64)]


class Vp8Mb(C.Structure):
    """mirror of vip_vp8_mb (include/vipcup_hip.h)"""
    _fields_ = [("ymode", C.c_uint8), ("uvmode", C.c_uint8), ("flevel", C.c_uint8), ("ilevel", C.c_uint8), ("hev", C.c_uint8),
                ("inner", C.c_uint8), ("segment", C.c_uint8), ("skip", C.c_uint8), ("bmodes", C.c_uint8 * 16), ("nz", C.c_uint32),
                ("dc_only", C.c_uint32), ("coef_idx", C.c_uint32), ("reserved", C.c_uint32)]


class Vp8Desc(C.Structure):
    """mirror of vip_vp8_desc (include/vipcup_hip.h)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("mb_w", C.c_int32), ("mb_h", C.c_int32), ("has_alpha", C.c_int32),
                ("filter_type", C.c_int32), ("stats", C.c_int64), ("stream_off", C.c_int64), ("mb_off", C.c_int64),
                ("coef_off", C.c_int64), ("coef_blocks", C.c_int64), ("plane_off", C.c_int64)]


class Vp8EncParams(C.Structure):
    """mirror of vip_vp8_enc_params (include/vipcup_hip.h)"""
    _fields_ = [("quality", C.c_int32), ("base_q", C.c_int32), ("y1", C.c_int32 * 2), ("y2", C.c_int32 * 2), ("uv", C.c_int32 * 2),
                ("filter_level", C.c_int32), ("flevel", C.c_int32), ("ilevel", C.c_int32), ("hev", C.c_int32), ("i4_bias", C.c_int32),
                ("reserved", C.c_int32), ("y1_inv", C.c_uint32 * 2), ("y2_inv", C.c_uint32 * 2), ("uv_inv", C.c_uint32 * 2)]


_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> (restype, argtypes); every symbol include/vipcup_hip.h declares
SIGNATURES = {
    "vip_version": (_i, []),
    "vip_last_error": (C.c_char_p, []),
    "vip_conv2d_nhwc_f16": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp]),
    "vip_conv2d_gated_nhwc_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp]),
    "vip_conv2d_hilo_nhwc_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp]),
    "vip_conv2d_out_gated_nhwc_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp]),
    "vip_conv2d_out_gated_variant": (_i, [C.POINTER(ConvDesc), _i, C.c_char_p, _sz]),
    "vip_conv2d_out_gated2_nhwc_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(ConvDesc), _vp]),
    "vip_conv2d_out_gated2_variant": (_i, [C.POINTER(ConvDesc), _i, _i, C.c_char_p, _sz]),
    "vip_gemm_bias_act_f16": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 9 + [_vp]),
    "vip_ln_gemm_supported": (_i, [_i, _i, _i, _i]),
    "vip_ln_gemm_bias_act_f16": (_i, [_vp, _vp, _vp, _f] + [_vp] * 4 + [_i] * 9 + [_vp]),
    "vip_mlp_fused_supported": (_i, [_i, _i, _i, _i]),
    "vip_mlp_fused_plan": (_i, [_i] * 4 + [C.POINTER(_i)] * 2),
    "vip_mlp_fused_f16": (_i, [_vp, _vp, _vp, _f] + [_vp] * 6 + [_i] * 9 + [_vp]),
    "vip_se_gate_f16": (_i, [_vp] * 6 + [_i] * 11 + [_vp]),
    "vip_se_gate_hilo_f16": (_i, [_vp] * 7 + [_i] * 11 + [_vp]),
    "vip_gemm_split_f16": (_i, [_vp, _vp, _vp, _vp] + [_i] * 6 + [_vp]),
    "vip_gemm_split2_f16": (_i, [_vp, _vp, _vp, _vp] + [_i] * 5 + [_vp]),
    "vip_gemm_split2_hilo_f16": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 5 + [_vp]),
    "vip_dwconv2d_nhwc_f16": (_i, [_vp, _vp, _vp, _vp] + [_i] * 11 + [_vp]),
    "vip_dwconv2d_pool_parts": (_i, [_i] * 8),
    "vip_dwconv2d_tile_plan": (C.c_long, [_i] * 9 + [C.POINTER(_i)] * 2),
    "vip_dwconv2d_pool_nhwc_f16": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 12 + [_vp]),
    "vip_se_gate_pooled_f16": (_i, [_vp, _i] + [_vp] * 5 + [_i] * 10 + [_vp]),
    "vip_layernorm_f16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "vip_pool2d_nhwc_f16": (_i, [_vp, _vp] + [_i] * 13 + [_vp]),
    "vip_global_avgpool_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vip_global_avgpool_split_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vip_gap_dense_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vip_experiments_built": (_i, []),
    "vip_gcvit_attn_block_supported": (_i, [_i, _i, _i]),
    "vip_gcvit_attn_block_f16": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp] + [_i] * 6 + [_f, _vp]),
    "vip_mbconv_expand_dw_supported": (_i, [_i, _i, _i, _i]),
    "vip_mbconv_expand_dw_f16": (_i, [_vp] * 7 + [_i] * 14 + [_vp]),
    "vip_head_prob_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "vip_head_act_f32": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "vip_prob_to_score_f32": (_i, [_vp, _vp, _i, _i, _vp]),
    "vip_ensemble_mean_f32": (_i, [_vp, _vp, _i, _i, C.c_long, _vp]),
    "vip_gap_ln_dense_f32": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vip_scale_add_act_f16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "vip_scale_add_act2_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vip_scale_add_act3_f16": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vip_mul_f16": (_i, [_vp, _vp, _vp, C.c_long] + [_i] * 7 + [_vp]),
    "vip_radix_combine_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "vip_radix_combine2_f16": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "vip_window_attn_fwd_f16": (_i, [_vp, _vp, _vp, _vp] + [_i] * 7 + [_f, _vp]),
    "vip_mhsa_fwd_f16": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "vip_jpeg_probe_h": (_i, [_vp, _sz, _vp, _vp]),
    "vip_jpeg_entropy_decode_h": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp, _i]),
    "vip_jpeg_idct_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    "vip_jpeg_quality_tables_h": (_i, [_i, _vp, _vp]),
    "vip_jpeg_encode_layout_h": (_i, [_i, _i, _i, _i, _vp, _vp]),
    "vip_jpeg_fdct_quant_u8": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp]),
    "vip_resample_coeffs_h": (_i, [_i, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "vip_resample_tile_shape": (_i, [_vp, _vp, _vp]),
    "vip_resample_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp]),
    "vip_blur_weights_h": (_i, [C.c_double, _i, _vp, _sz]),
    "vip_blur_gauss_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _vp]),
    "vip_median_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    "vip_sharpen_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    "vip_warp_affine_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "vip_colour_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "vip_noise_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, C.c_int64, C.c_uint32, _vp, _vp, _i, _vp]),
    "vip_noise_rgb_u8_placed": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, C.c_int64, C.c_uint32, _vp, _vp, _i, _i, _vp]),
    "vip_tone_hist_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "vip_tone_lut_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "vip_tone_apply_rgb_u8": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    "vip_tone_apply_rgb_u8_placed": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "vip_png_probe_h": (_i, [_vp, _sz, _vp, _vp]),
    "vip_png_inflate_h": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp, _i]),
    "vip_png_unfilter_rgb_u8": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp]),
    "vip_webp_probe_h": (_i, [_vp, _sz, _vp, _vp]),
    "vip_webp_entropy_h": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp, _i]),
    "vip_webp_inverse_rgb_u8": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp]),
    "vip_vp8_probe_h": (_i, [_vp, _sz, _vp, _vp]),
    "vip_vp8_entropy_h": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp, _i]),
    "vip_vp8_scratch_bytes": (_i, [_vp, _i, _vp]),
    "vip_vp8_reconstruct_rgb_u8": (_i, [_vp, _sz, _vp, _i, _vp, _sz, _vp, _i, _i, _vp]),
    "vip_vp8_default_stages": (_i, []),
    "vip_vp8_reconstruct_stages_rgb_u8": (_i, [_vp, _sz, _vp, _i, _vp, _sz, _vp, _i, _i, _i, _vp]),
    "vip_vp8_encode_params_h": (_i, [_i, _vp]),
    "vip_vp8_encode_layout_h": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "vip_vp8_encode_rgb_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "vip_bicubic_table_f32": (_i, [_vp]),
    "vip_resize_bicubic_norm_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "vip_tile_resize_bicubic_norm_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "vip_tile_resize_bicubic_norm_s32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "vip_tile_aggregate_f32": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "vip_image_mean_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "vip_occlude_resize_bicubic_norm_f16": (_i, [_vp] * 5 + [_i] * 4 + [_vp, _i, _i, _i, _vp]),
    "vip_occlude_resize_bicubic_norm_s32": (_i, [_vp] * 5 + [_i] * 4 + [_vp, _i, _i, _i, _vp]),
    "vip_occlusion_cells_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "vip_occlusion_map": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "vip_tta_augment_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "vip_vit_tokens_f16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    # STRICT precision path (fp32 storage, fp32 arithmetic): csrc/strict_conv.hip, csrc/strict_ops.hip
    "vip_conv2d_nhwc_s32": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp]),
    "vip_conv2d_nhwc_s32x": (_i, [_vp, _vp, _i, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp]),
    "vip_conv2d_nhwc_s32x2": (_i, [_vp, _vp, _i, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp]),
    "vip_dwconv2d_nhwc_s32": (_i, [_vp, _vp, _vp, _vp] + [_i] * 11 + [_vp]),
    "vip_layernorm_s32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "vip_pool2d_nhwc_s32": (_i, [_vp, _vp] + [_i] * 13 + [_vp]),
    "vip_global_avgpool_s32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vip_scale_add_act_s32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vip_radix_combine_s32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "vip_mul_s32": (_i, [_vp, _vp, _vp, C.c_long] + [_i] * 7 + [_vp]),
    "vip_vit_tokens_s32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "vip_gap_ln_dense_s32": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _i, _i, C.c_long, _i, _vp]),
    "vip_window_attn_fwd_s32": (_i, [_vp, _vp, _vp, _vp] + [_i] * 7 + [_f, _vp]),
    "vip_mhsa_fwd_s32": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "vip_resize_bicubic_norm_s32": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "vip_tta_augment_s32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    # STRICT precision path, packed (hi, lo) fp16 storage: csrc/conv_h2.hip, csrc/strict_ops.hip
    "vip_pack_h2": (_i, [_vp, _vp, C.c_long, _vp, _vp]),
    "vip_unpack_h2": (_i, [_vp, _vp, C.c_long, _vp]),
    "vip_conv2d_nhwc_h2": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _f, _vp, _vp]),
    "vip_conv2d_gated_nhwc_h2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _f, _vp, _vp]),
    "vip_conv2d_kernel_name_h2": (_i, [C.POINTER(ConvDesc), _i, C.c_char_p, _sz]),
    "vip_conv2d_kernel_variant_h2": (_i, [C.POINTER(ConvDesc), _i, C.c_char_p, _sz]),
    "vip_dwconv2d_nhwc_h2": (_i, [_vp, _vp, _vp, _vp] + [_i] * 11 + [_vp, _vp]),
    "vip_dwconv2d_tile_plan_h2": (C.c_long, [_i] * 10 + [C.POINTER(_i)] * 2),
    "vip_mlp_fused_supported_h2": (_i, [_i] * 4),
    "vip_mlp_fused_plan_h2": (_i, [_i] * 4 + [C.POINTER(_i)] * 2),
    "vip_mlp_fused_h2": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _f, _vp, _vp, _f, _vp, _vp] + [_i] * 9 + [_vp, _vp]),
    "vip_dw_filter_quad_major": (_i, [_vp, _vp, _i, _i, _vp]),
    "vip_dwconv2d_s1_supported_h2": (_i, [_i] * 7),
    "vip_dwconv2d_s1_plan_h2": (C.c_long, [_i] * 7 + [C.POINTER(_i)] * 2),
    "vip_dwconv2d_s1_h2": (_i, [_vp, _vp, _vp, _vp] + [_i] * 10 + [_vp, _vp]),
    "vip_dwconv2d_s1_pool_parts_h2": (_i, [_i] * 7),
    "vip_dwconv2d_s1_pool_h2": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 11 + [_vp, _vp]),
    "vip_se_gate_pooled_h2": (_i, [_vp, _i, _vp, _vp, _f, _vp, _vp, _f, _vp] + [_i] * 9 + [_vp, _vp]),
    "vip_se_gate_h2": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _f, _vp] + [_i] * 10 + [_vp, _vp]),
    "vip_layernorm_h2": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp]),
    "vip_pool2d_nhwc_h2": (_i, [_vp, _vp] + [_i] * 13 + [_vp, _vp]),
    "vip_global_avgpool_h2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "vip_scale_add_act_h2": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "vip_radix_combine_h2": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "vip_mul_h2": (_i, [_vp, _vp, _vp, C.c_long] + [_i] * 7 + [_vp, _vp]),
    "vip_vit_tokens_h2": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "vip_gap_ln_dense_h2": (_i, [_vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _i, _i, C.c_long, _i, _vp]),
    "vip_window_attn_fwd_h2": (_i, [_vp, _vp, _vp, _vp] + [_i] * 7 + [_f, _vp, _vp]),
    "vip_mhsa_fwd_h2": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _vp]),
    # evidence maps (Grad-CAM): csrc/cam.hip
    "vip_cam_f32": (_i, [_vp, _vp, _vp, _f] + [_vp] * 5 + [_i] * 4 + [C.c_long, _i, _i, _i, _vp]),
    "vip_cam_s32": (_i, [_vp, _vp, _vp, _f] + [_vp] * 5 + [_i] * 4 + [C.c_long, _i, _i, _i, _vp]),
    "vip_cam_h2": (_i, [_vp, _vp, _vp, _f] + [_vp] * 5 + [_i] * 4 + [C.c_long, _i, _i, _i, _vp]),
    "vip_cam_compose_f32": (_i, [_vp] * 5 + [_i, _vp, _i, _i, _i, _vp, _i, _vp]),
    "vip_cam_overlay_u8": (_i, [_vp, _vp, _vp, _f, _i, _i, _i, _vp, _vp]),
    # HorNet global-local filter: csrc/global_filter.hip
    "vip_global_local_filter_supported": (_i, [_i, _i, _i]),
    "vip_global_local_filter_plan": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "vip_global_local_filter_nhwc_f16": (_i, [_vp] * 4 + [_i] * 4 + [_vp]),
    "vip_global_local_filter_nhwc_s32": (_i, [_vp] * 4 + [_i] * 4 + [_vp]),
    "vip_global_local_filter_nhwc_h2": (_i, [_vp] * 4 + [_i] * 4 + [_vp, _vp]),
    # Swin V2 shifted cosine window attention: csrc/swin_attn.hip
    "vip_swin_attn_supported": (_i, [_i] * 4),
    "vip_swin_attn_plan": (_i, [_i] * 6 + [C.POINTER(_i)] * 3),
    "vip_swin_attn_fwd_f16": (_i, [_vp] * 5 + [_i] * 7 + [_vp]),
    "vip_swin_attn_fwd_s32": (_i, [_vp] * 5 + [_i] * 7 + [_vp]),
    "vip_swin_attn_fwd_h2": (_i, [_vp] * 5 + [_i] * 7 + [_vp, _vp]),
    # neighbourhood attention: csrc/nat_attn.hip
    "vip_nat_attn_plan": (_i, [_i] * 5 + [C.POINTER(_i)] * 3),
    "vip_nat_attn_fwd_f16": (_i, [_vp] * 4 + [_i] * 6 + [_vp]),
    "vip_nat_attn_fwd_s32": (_i, [_vp] * 4 + [_i] * 6 + [_vp]),
    "vip_nat_attn_fwd_h2": (_i, [_vp] * 4 + [_i] * 6 + [_vp, _vp]),
    "vip_conv2d_kernel_name": (_i, [C.POINTER(ConvDesc), _i, _i, _i, C.c_char_p, _sz]),
    "vip_conv2d_kernel_variant": (_i, [C.POINTER(ConvDesc), _i, _i, _i, C.c_char_p, _sz]),
    "vip_workspace_bytes": (_sz, [_i, C.POINTER(C.c_int64), _i]),
    "vip_microbench_copy": (_i, [_vp, _vp, _sz, _vp]),
    "vip_microbench_copy_variant": (_i, [_vp, _vp, _sz, _i, _vp]),
    "vip_microbench_mfma_f16": (_i, [_vp, _i, C.POINTER(C.c_double), _vp]),
}


def lib():
    """Return the loaded library (loading it on first use)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VipError(
                f"{LIB_PATH} not found: build it with `python vip-cup-2022_amd/build.py` "
                "(or __graft_entry__.build()); vipcup_amd has no CPU fallback")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().vip_last_error().decode("utf-8", "replace")
        raise VipError(f"{what} failed with vip_status {status}: {msg}")

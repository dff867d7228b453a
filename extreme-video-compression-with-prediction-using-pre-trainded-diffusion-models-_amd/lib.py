"""ctypes bindings to the two C-ABI libraries (include/evc_hip.h, include/evc_rans.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every kernel launch goes
through the C ABI with raw pointers.  There is NO fallback path -- a missing library or a non-gfx950
device raises ``EvcLibraryError`` so a silent eager/CPU substitute can never pass a GPU test.
"""
import ctypes
import math
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_longlong, c_uint, c_uint8, c_ulonglong, c_void_p

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_SO = os.path.join(HERE, "lib", "libevc_hip.so")
if os.environ.get("EVC_HIP_SO"):       # A/B builds of the kernel library (tools/ab_lib.sh); in-tree paths only
    HIP_SO = os.path.abspath(os.environ["EVC_HIP_SO"])
RANS_SO = os.path.join(HERE, "lib", "libevc_rans.so")

ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2
# How the convolution multiplies (include/evc_hip.h EVC_ARITH_*).  All are fp32 convolutions with fp32 accumulation:
#   F32     v_mfma_f32_32x32x2_f32, exact products;
#   BF16X6  every fp32 operand split exactly into three bf16 values, six cross products on the bf16 matrix cores;
#   F16X3   operands scaled into fp16's range and split 2-way (2^-22 relative), three cross products on the fp16 matrix
#           cores -- only valid where the operand is O(1) (GroupNorm-normalised / activated inputs).
# Measured error vs fp64 on MI355X: F16X3 < BF16X6 < F32 chain (profiles/r02_split_numerics.log).  The packed weights
# carry the choice in their dtype (float32 / bfloat16 / float16).  EVC_CONV_ARITH=f32|bf16x6|f16x3 sets the policy:
# "f16x3" (default) = F16X3 for convolutions whose input is normalised (``bounded_arith``), BF16X6 for the rest.
ARITH_F32, ARITH_BF16X6, ARITH_F16X3 = 0, 1, 2
_ARITH_NAMES = {"f32": ARITH_F32, "bf16x6": ARITH_BF16X6, "f16x3": ARITH_F16X3}
_ARITH_DTYPES = {ARITH_F32: torch.float32, ARITH_BF16X6: torch.bfloat16, ARITH_F16X3: torch.float16}


def _arith_policy():
    name = os.environ.get("EVC_CONV_ARITH", "f16x3").lower()
    if name not in _ARITH_NAMES:
        raise ValueError(f"EVC_CONV_ARITH must be one of {sorted(_ARITH_NAMES)}, got {name!r}")
    return _ARITH_NAMES[name]


def default_arith():
    """Arithmetic for convolutions whose operand range is unknown (raw residual streams, ELIC): never F16X3."""
    a = _arith_policy()
    return ARITH_BF16X6 if a == ARITH_F16X3 else a


def bounded_arith():
    """Arithmetic for convolutions whose input is GroupNorm-normalised / activated, i.e. O(1)."""
    return _arith_policy()


class EvcLibraryError(RuntimeError):
    pass


class EvcKernelError(RuntimeError):
    pass


class ConvArgs(ctypes.Structure):
    """Mirror of ``evc_conv_args`` (include/evc_hip.h)."""
    _fields_ = [("src0", c_void_p), ("src1", c_void_p), ("C0", c_int), ("C1", c_int),
                ("ld0", c_int), ("ld1", c_int),
                ("coef_a", c_void_p), ("coef_s", c_void_p), ("act_in", c_int),
                ("w_packed", c_void_p), ("bias", c_void_p), ("res", c_void_p), ("ld_res", c_int),
                ("out_scale", c_float), ("act_out", c_int),
                ("out", c_void_p), ("ld_out", c_int),
                ("B", c_int), ("H", c_int), ("W", c_int), ("Co", c_int), ("KH", c_int), ("KW", c_int),
                ("splits", c_int), ("stats_out", c_void_p), ("arith", c_int), ("in_bound", c_void_p),
                ("x2_src0", c_void_p), ("x2_src1", c_void_p), ("x2_C0", c_int), ("x2_C1", c_int), ("x2_ld0", c_int),
                ("x2_ld1", c_int), ("x2_w_packed", c_void_p), ("x2_bound", c_void_p), ("invariant", c_int)]


class ConvPlan(ctypes.Structure):
    """Mirror of ``evc_conv_plan`` (include/evc_hip.h): what ``evc_conv_plan_query`` reports."""
    _fields_ = [("kernel", ctypes.c_char * 96), ("tile_m", c_int), ("tile_n", c_int), ("splits", c_int),
                ("steps_per_split", c_int), ("cut_chunk", c_int), ("tail_tiles", c_int), ("tail_splits", c_int),
                ("stats_runs", c_int), ("fused_1x1", c_int)]


class NinArgs(ctypes.Structure):
    """Mirror of ``evc_nin_args`` (include/evc_hip.h)."""
    _fields_ = [("x", c_void_p), ("x1", c_void_p), ("Ci", c_int), ("Co", c_int), ("coef_a", c_void_p), ("coef_s", c_void_p),
                ("in_bound", c_void_p), ("w_packed", c_void_p), ("arith", c_int), ("bias", c_void_p), ("res", c_void_p),
                ("out_scale", c_float), ("act_out", c_int), ("out", c_void_p), ("stats_out", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("tile", c_int)]


class NinPlan(ctypes.Structure):
    """Mirror of ``evc_nin_plan`` (include/evc_hip.h): what ``evc_nin_gemm_plan_query`` reports."""
    _fields_ = [("kernel", ctypes.c_char * 64), ("tile_m", c_int), ("tile_n", c_int), ("stages", c_int), ("stats_runs", c_int)]


class SmallConvArgs(ctypes.Structure):
    """Mirror of ``evc_small_conv_args`` (include/evc_hip.h)."""
    _fields_ = [("src0", c_void_p), ("src1", c_void_p), ("C0", c_int), ("C1", c_int),
                ("coef_a", c_void_p), ("coef_s", c_void_p), ("act_in", c_int), ("in_bound", c_void_p),
                ("w_packed", c_void_p), ("arith", c_int), ("bias", c_void_p), ("res", c_void_p),
                ("out_scale", c_float), ("act_out", c_int), ("out", c_void_p), ("stats_out", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("Co", c_int), ("KH", c_int), ("KW", c_int),
                ("x2_w_packed", c_void_p), ("invariant", c_int), ("variant", c_int)]


class SmallConvPlan(ctypes.Structure):
    """Mirror of ``evc_small_conv_plan`` (include/evc_hip.h): what ``evc_small_conv_plan_query`` reports."""
    _fields_ = [("kernel", ctypes.c_char * 64), ("variant", c_int), ("tile_m", c_int), ("tile_n", c_int), ("groups", c_int),
                ("chunks", c_int), ("rounds", c_int), ("stats_runs", c_int)]


class AttentionPlan(ctypes.Structure):
    """Mirror of ``evc_attention_plan`` (include/evc_hip.h): what ``evc_attention_plan_query`` reports."""
    _fields_ = [("kernel", ctypes.c_char * 64), ("waves", c_int), ("kparts", c_int), ("tiles_per_part", c_int),
                ("kv_planes", c_int), ("merge", c_int), ("short_seq", c_int),
                ("lds_bytes", c_longlong), ("parts_bytes", c_longlong), ("ws_bytes", c_longlong)]


# name -> (restype, argtypes); exactly the symbols declared in include/evc_hip.h
HIP_SYMBOLS = {
    "evc_version": (c_char_p, []),
    "evc_arch": (c_char_p, []),
    "evc_device_ok": (c_int, []),
    "evc_clock_probe": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "evc_im2col_nchw_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 9 + [c_void_p, c_void_p, c_void_p]),
    "evc_maxpool3s2_nhwc_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_lpips_layer_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_maxpool2d_nhwc_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p]),
    "evc_lpips_map_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "evc_lpips_map_mean_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "evc_lpips_upsample_add_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    "evc_i3d_stem_im2col_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 17 + [c_void_p]),
    "evc_maxpool3d_same_nthwc_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 11 + [c_void_p]),
    "evc_i3d_head_f32": (c_int, [c_void_p] * 4 + [c_int] * 6 + [c_void_p]),
    "evc_upfirdn2d_f32": (c_int, [c_void_p, c_void_p, POINTER(c_float)] + [c_int] * 13 + [c_void_p]),
    "evc_upfirdn2d_nhwc_f32": (c_int, [c_void_p, c_void_p, POINTER(c_float)] + [c_int] * 10 +
                               [c_void_p, c_void_p, c_int, c_void_p]),
    "evc_pack_nchw_to_nhwc_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                          c_void_p]),
    "evc_nhwc_to_nchw_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_chan_stats_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_gn_coeffs_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                  c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "evc_gn_coeffs_bound_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                        c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "evc_moments_bound_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "evc_gn_coeffs_site_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                       c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_int, c_void_p]),
    "evc_gn_coeffs_bound_site_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                             c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "evc_moments_bound_site_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                           c_int, c_void_p]),
    "evc_invariant_plan_revision": (c_int, []),
    "evc_conv_plan_query": (c_int, [POINTER(ConvArgs), POINTER(ConvPlan)]),
    "evc_gn_coeffs_bound_sample_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                               c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "evc_moments_bound_sample_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                             c_int, c_void_p]),
    "evc_attention_invariant_workspace_bytes": (c_longlong, [c_int, c_int, c_int, c_int]),
    "evc_attention_invariant_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                            c_float, c_void_p, c_void_p, c_void_p]),
    "evc_attention_f16x3_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_float, c_void_p, c_void_p, c_void_p]),
    "evc_deconv5x5s2_phase_weights_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_conv5x5s2_phase_weights_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "evc_depth_to_space2_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_space_to_depth2_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_deconv5x5s2_workspace_bytes": (c_longlong, [c_int, c_int, c_int, c_int]),
    "evc_deconv5x5s2_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    "evc_conv5x5s2_workspace_bytes": (c_longlong, [c_int, c_int, c_int, c_int]),
    "evc_conv5x5s2_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    "evc_gdn_workspace_bytes": (c_longlong, [c_int, c_int, c_int, c_int]),
    "evc_gdn_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                            c_int, c_void_p]),
    "evc_affine_act_nhwc_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_int, c_void_p]),
    "evc_conv_co_pad": (c_int, [c_int]),
    "evc_conv_packed_floats": (c_longlong, [c_int, c_int, c_int, c_int]),
    "evc_conv_pack_weights_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_conv_packed_bytes": (c_longlong, [c_int, c_int, c_int, c_int, c_int]),
    "evc_conv_pack_weights": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_conv_set_option": (c_int, [c_char_p, c_int]),
    "evc_spade_act_nhwc_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                       c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "evc_conv_choose_splits": (c_int, [POINTER(ConvArgs)]),
    "evc_conv_kernel_name": (c_int, [POINTER(ConvArgs), c_char_p, c_int]),
    "evc_conv_fused_1x1_supported": (c_int, [POINTER(ConvArgs)]),
    "evc_conv_stats_splits": (c_int, [POINTER(ConvArgs)]),
    "evc_conv_workspace_bytes": (c_longlong, [POINTER(ConvArgs)]),
    "evc_conv2d_nhwc_f32": (c_int, [POINTER(ConvArgs), c_void_p, c_void_p]),
    "evc_conv2d_nhwc_profiled_f32": (c_int, [POINTER(ConvArgs), c_void_p, c_void_p, c_void_p, c_void_p]),
    "evc_nin_gemm_supported": (c_int, [POINTER(NinArgs)]),
    "evc_nin_gemm_plan_query": (c_int, [POINTER(NinArgs), POINTER(NinPlan)]),
    "evc_nin_gemm_f32": (c_int, [POINTER(NinArgs), c_void_p]),
    "evc_small_conv_supported": (c_int, [POINTER(SmallConvArgs)]),
    "evc_small_conv_plan_query": (c_int, [POINTER(SmallConvArgs), POINTER(SmallConvPlan)]),
    "evc_small_conv_f32": (c_int, [POINTER(SmallConvArgs), c_void_p]),
    "evc_attention_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                  c_float, c_void_p]),
    "evc_attention_workspace_bytes": (c_longlong, [c_int, c_int, c_int, c_int]),
    "evc_attention_set_option": (c_int, [c_char_p, c_int]),
    "evc_attention_plan_query": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(AttentionPlan)]),
    "evc_attention_ws_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                     c_float, c_void_p, c_void_p]),
    "evc_frame_group_norm_f32": (c_int, [c_void_p] * 4 + [c_int] * 5 + [c_float, c_void_p]),
    "evc_frame_attention_f32": (c_int, [c_void_p, c_int, c_void_p, c_int] + [c_int] * 5 + [c_float, c_void_p]),
    "evc_frame_mix_f32": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_longlong, c_void_p]),
    "evc_frame_taps_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    "evc_ddpm_step_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_longlong] + [c_float] * 5 + [c_int, c_void_p]),
    "evc_ddim_step_f32": (c_int, [c_void_p, c_void_p, c_longlong] + [c_float] * 4 + [c_int, c_void_p]),
    "evc_axpy_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_longlong, c_float, c_void_p]),
    "evc_pndm_transfer_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_longlong, c_float, c_float, c_float, c_int,
                                      c_void_p]),
    "evc_lincomb4_f32": (c_int, [c_void_p] * 5 + [c_longlong] + [c_float] * 4 + [c_void_p]),
    "evc_scale_clamp_f32": (c_int, [c_void_p, c_void_p, c_longlong, c_float, c_float, c_int, c_float, c_float,
                                    c_void_p]),
    "evc_gate_residual_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_void_p]),
    "evc_elic_gather_params_f32": (c_int, [c_void_p] + [c_int] * 8 + [c_void_p, c_int, c_void_p, c_void_p,
                                                                       c_void_p]),
    "evc_elic_scatter_symbols_f32": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 7 + [c_void_p]),
    "evc_elic_quantize_f32": (c_int, [c_void_p, c_int, c_int, c_void_p] + [c_int] * 5 + [c_void_p, c_void_p]),
    "evc_elic_rate_pass_f32": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_void_p]),
    "evc_bottleneck_rate_f32": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p] * 5),
    "evc_noise_normal_f32": (c_int, [c_void_p, c_void_p, c_int, c_longlong, c_ulonglong, c_uint, c_int, c_void_p]),
    "evc_yuv420_to_rgb": (c_int, [c_void_p] + [c_longlong] * 6 + [c_int] * 5 + [c_void_p, c_int, c_void_p]),
    "evc_rgb_to_yuv420": (c_int, [c_void_p, c_void_p] + [c_longlong] * 6 + [c_int] * 4 + [c_void_p, c_void_p]),
    "evc_resample_h_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_longlong, c_longlong, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                  c_void_p]),
    "evc_resample_v_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_longlong, c_longlong, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                  c_void_p]),
    "evc_tile_grid_check": (c_int, [c_int] * 6 + [c_void_p, c_void_p, c_int]),
    "evc_tile_gather_u8": (c_int, [c_void_p] + [c_int] * 6 + [c_void_p] * 6),
    "evc_tile_blend_f32": (c_int, [c_void_p] + [c_int] * 6 + [c_void_p] * 6),
    "evc_tile_gather_f32": (c_int, [c_void_p] + [c_int] * 7 + [c_void_p] * 6),
    "evc_ssim_workspace_bytes": (c_longlong, [c_int, c_int, c_int]),
    "evc_ssim_planes_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_double, c_double, c_void_p, c_void_p,
                                    c_void_p]),
    "evc_msssim_workspace_bytes": (c_longlong, [c_int, c_int, c_int, c_int]),
    "evc_msssim_levels_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_double, c_double, c_void_p,
                                      c_void_p, c_void_p]),
    "evc_frame_sqerr_f64": (c_int, [c_void_p, c_void_p, c_int, c_longlong, c_void_p, c_void_p]),
    "evc_inception_stem_im2col_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p]),
    "evc_im2col_nhwc_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 11 + [c_void_p]),
    "evc_pool3x3s1p1_nhwc_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    "evc_spatial_mean_nhwc_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p]),
    "evc_knn_radius_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p]),
    "evc_manifold_hits_f32": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p]),
}

RANS_SYMBOLS = {
    "evc_rans_version": (c_char_p, []),
    "evc_rans_max_encoded_bytes": (c_longlong, [c_longlong]),
    "evc_rans_encode_with_indexes": (c_longlong, [POINTER(c_int32), POINTER(c_int32), c_longlong, POINTER(c_int32),
                                                  c_int, POINTER(c_int32), POINTER(c_int32), c_int,
                                                  POINTER(c_uint8), c_longlong]),
    "evc_rans_decode_with_indexes": (c_int, [POINTER(c_uint8), c_longlong, POINTER(c_int32), c_longlong,
                                             POINTER(c_int32), c_int, POINTER(c_int32), POINTER(c_int32), c_int,
                                             POINTER(c_int32)]),
    "evc_pmf_to_quantized_cdf": (c_int, [POINTER(c_float), c_int, c_int, POINTER(c_int32)]),
}

_hip = None
_rans = None


def _load(path, symbols, what):
    if not os.path.exists(path):
        raise EvcLibraryError(f"{what} not built: {path} is missing. Run `python -c \"import __graft_entry__ as g; "
                              f"g.build()\"` (needs hipcc / g++). There is no fallback path.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in symbols.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise EvcLibraryError(f"{path} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    return lib


def hip_lib(require_device=True):
    """The HIP kernel library.  ``require_device=False`` is only for symbol/export checks on CPU boxes."""
    global _hip
    if _hip is None:
        _hip = _load(HIP_SO, HIP_SYMBOLS, "libevc_hip.so")
        # A/B switches of the convolution dispatch (same-box comparisons: tools/ab_*.sh): EVC_CONV_OPTIONS="tail_split=0,..."
        for item in filter(None, os.environ.get("EVC_CONV_OPTIONS", "").split(",")):
            name, _, value = item.partition("=")
            if _hip.evc_conv_set_option(name.strip().encode(), int(value or 1)) != 0:
                raise ValueError(f"EVC_CONV_OPTIONS: unknown convolution option {name!r}")
    if require_device:
        if not torch.cuda.is_available():
            raise EvcLibraryError("no HIP device visible: the evc_amd compute path is gfx950-only (no CPU fallback)")
        if not getattr(hip_lib, "_checked", False):
            if _hip.evc_device_ok() != 1:
                raise EvcLibraryError("current HIP device is not gfx950 (MI355X); libevc_hip.so has no code for it")
            hip_lib._checked = True
    return _hip


def rans_lib():
    global _rans
    if _rans is None:
        _rans = _load(RANS_SO, RANS_SYMBOLS, "libevc_rans.so")
    return _rans


def _check(rc, name):
    if rc != 0:
        raise EvcKernelError(f"{name} failed with code {rc} "
                             "(-1 invalid argument, -2 unsupported, -3 launch failure)")


def stream_ptr():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-contiguous tensor required"
    return c_void_p(t.data_ptr())


def fptr(t, dtype=torch.float32):
    assert t is None or t.dtype == dtype, (t.dtype, dtype)
    return ptr(t)


# ----------------------------------------------------------------------------------------------
# thin, shape-checked wrappers (one per C entry point that the host code uses)
# ----------------------------------------------------------------------------------------------

def upfirdn2d_nchw(x, kernel, up=1, down=1, pad=(0, 0)):
    """Drop-in for reference ``upfirdn2d(input, kernel, up, down, pad)`` (models/better/op/upfirdn2d.py:13)."""
    L = hip_lib()
    assert x.dim() == 4 and x.dtype == torch.float32
    x = x.contiguous()
    n, c, h, w = x.shape
    k = np.ascontiguousarray(np.asarray(kernel.detach().cpu() if torch.is_tensor(kernel) else kernel,
                                        dtype=np.float32))
    kh, kw = k.shape
    oh = (h * up + pad[0] + pad[1] - kh) // down + 1
    ow = (w * up + pad[0] + pad[1] - kw) // down + 1
    out = torch.empty((n, c, oh, ow), device=x.device, dtype=torch.float32)
    _check(L.evc_upfirdn2d_f32(fptr(x), fptr(out), k.ctypes.data_as(POINTER(c_float)), n * c, h, w, kh, kw, up, up,
                               down, down, pad[0], pad[1], pad[0], pad[1], stream_ptr()), "evc_upfirdn2d_f32")
    return out


def upfirdn2d_nhwc(x, kernel, up, down, pad, coef=None, act=ACT_NONE, out=None):
    L = hip_lib()
    B, H, W, C = x.shape
    k = np.ascontiguousarray(np.asarray(kernel, dtype=np.float32))
    kh, kw = k.shape
    oh = (H * up + pad[0] + pad[1] - kh) // down + 1
    ow = (W * up + pad[0] + pad[1] - kw) // down + 1
    if out is None:
        out = torch.empty((B, oh, ow, C), device=x.device, dtype=torch.float32)
    ca, cs = coef if coef is not None else (None, None)
    _check(L.evc_upfirdn2d_nhwc_f32(fptr(x), fptr(out), k.ctypes.data_as(POINTER(c_float)), B, H, W, C, kh, kw, up,
                                    down, pad[0], pad[1], fptr(ca), fptr(cs), act, stream_ptr()),
           "evc_upfirdn2d_nhwc_f32")
    return out


def pack_nchw_to_nhwc(x0, x1, cpad, out=None):
    L = hip_lib()
    B, C0, H, W = x0.shape
    C1 = 0 if x1 is None else x1.shape[1]
    if out is None:
        out = torch.empty((B, H, W, cpad), device=x0.device, dtype=torch.float32)
    _check(L.evc_pack_nchw_to_nhwc_f32(fptr(x0.contiguous()), C0, fptr(None if x1 is None else x1.contiguous()), C1,
                                       fptr(out), cpad, B, H, W, stream_ptr()), "evc_pack_nchw_to_nhwc_f32")
    return out


def nhwc_to_nchw(x, C, out=None):
    L = hip_lib()
    B, H, W, ld = x.shape
    if out is None:
        out = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    _check(L.evc_nhwc_to_nchw_f32(fptr(x), ld, fptr(out), B, C, H, W, stream_ptr()), "evc_nhwc_to_nchw_f32")
    return out


# ---- batch-invariant mode (include/evc_hip.h) ---------------------------------------------------------------------
# Every wrapper below that plans by batch takes ``invariant=``: True asks the library for the batch-invariant plan of that
# call.  Per call, here as in the C ABI: there is no process-wide or ambient switch, a caller passes the flag on every call
# (``ScoreNet`` does through its ``_conv`` / ``_gn`` / ... helpers).
def invariant_plan_revision():
    """Integer bumped whenever a change alters the bits of batch-invariant mode (job streams carry it)."""
    return int(hip_lib(require_device=False).evc_invariant_plan_revision())


def stats_splits(B, HW, invariant=False):
    """Number of pixel ranges per image for evc_chan_stats_f32: enough blocks to fill the chip while every
    block still streams >= 64 pixels; ``invariant``: from HW only."""
    return max(1, min(HW // 64, 128 if invariant else (1024 + B - 1) // B))


def chan_stats(x, invariant=False):
    """x: (B, H, W, C) -> partial moments (B, nsplit, C, 2).  ``invariant``: pixel ranges from H*W only."""
    L = hip_lib()
    B, H, W, C = x.shape
    ns = stats_splits(B, H * W, bool(invariant))
    part = torch.empty((B, ns, C, 2), device=x.device, dtype=torch.float32)
    _check(L.evc_chan_stats_f32(fptr(x), fptr(part), B, H * W, C, ns, stream_ptr()), "evc_chan_stats_f32")
    return part


# Sticky range-event word of the fp16-split arithmetic (include/evc_hip.h EVC_RANGE_*), one per device: the coefficient /
# bound kernels OR bits into it when a tensor holds a NaN / inf or when a GroupNorm-ed operand may leave fp16's range.
RANGE_NONFINITE, RANGE_F16_OPERAND = 1, 2
_range_words = {}


def _events(device):
    w = _range_words.get(device.index)
    if w is None:
        w = _range_words[device.index] = torch.zeros(1, dtype=torch.int32, device=device)
    return w


def range_events(device=None, reset=False):
    """Bits raised so far on ``device`` (default: current): 0 = every fp16-split operand was provably in range and
    every tensor finite.  Synchronises the device.  RANGE_F16_OPERAND set means a trained checkpoint drives a normalised
    activation towards fp16's limit: run that model with EVC_CONV_ARITH=bf16x6 (exact 3-way bf16 split, no range limit),
    or let the decoder move only the layers that raised it to that split (EVC_RANGE_RECOVERY=layer, ``site_events``)."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    w = _range_words.get(idx)
    if w is None:
        return 0
    v = int(w.item())
    if reset:
        w.zero_()
    return v


class Site:
    """Where a coefficient / bound call reports its range events besides the device word: word ``index`` of a network's
    site arena ``words`` (``site_word_arena``).  ``quiet``: report to the site word only -- the network already moved that
    site's consumers off the fp16 split, so the global word stays reserved for the sites that still matter."""
    __slots__ = ("words", "index", "quiet")

    def __init__(self, words, index, quiet=False):
        self.words, self.index, self.quiet = words, int(index), bool(quiet)


def site_word_arena(n, device):
    """One zeroed int32 range-event word per event site of a network (include/evc_hip.h evc_*_site_f32).  Kept apart from
    the per-forward bound arena: it is only cleared on demand (``site_events(net, reset=True)``)."""
    return torch.zeros(max(1, int(n)), dtype=torch.int32, device=device)


def site_events(net, reset=False):
    """{site: EVC_RANGE_* bits} of the non-zero words of ``net``'s site arena, read with ONE device-to-host copy
    (synchronises the device); ``reset`` zeroes the arena afterwards."""
    w = net.site_words
    v = w.cpu().tolist()
    if reset:
        w.zero_()
    return {i: b for i, b in enumerate(v) if b}


def _site_args(site, device):
    """(events, site_events, index) pointers of a coefficient / bound call."""
    if site is None:
        return _word(_events(device)), None, 0
    assert site.words.is_cuda and site.words.dtype == torch.int32 and 0 <= site.index < site.words.numel()
    return (None if site.quiet else _word(_events(device))), c_void_p(site.words.data_ptr()), site.index


def raise_range_events(bits, device=None):
    """OR ``bits`` back into ``device``'s range-event word (a caller that cleared it to look at one piece of work restores
    what was there before)."""
    if bits:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        w = _events(dev)
        w.bitwise_or_(int(bits))


def im2col_nchw(x, KH, KW, stride, pad, ld_out, shift=None, scale=None):
    """x: (N, C, H, W) -> (N, Ho, Wo, ld_out) patch rows in (c, ky, kx) order, zero-filled beyond C*KH*KW; optional
    (x - shift[c]) / scale[c] before the zero padding (include/evc_hip.h)."""
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    out = torch.empty((N, Ho, Wo, ld_out), device=x.device, dtype=torch.float32)
    _check(hip_lib().evc_im2col_nchw_f32(fptr(x), fptr(out), N, C, H, W, KH, KW, stride, pad, ld_out, ptr(shift), ptr(scale),
                                         stream_ptr()), "evc_im2col_nchw_f32")
    return out


def maxpool3s2_nhwc(x):
    N, H, W, C = x.shape
    out = torch.empty((N, (H - 3) // 2 + 1, (W - 3) // 2 + 1, C), device=x.device, dtype=torch.float32)
    _check(hip_lib().evc_maxpool3s2_nhwc_f32(fptr(x), fptr(out), N, H, W, C, stream_ptr()), "evc_maxpool3s2_nhwc_f32")
    return out


def lpips_layer(f0, f1, lin_w, dist, accumulate):
    """dist[n] (+)= spatial mean of lin_w . (unit-normalised f0 - unit-normalised f1)^2; f0, f1: (N, H, W, C)."""
    N, H, W, C = f0.shape
    assert f1.shape == f0.shape and lin_w.numel() == C and dist.numel() == N
    _check(hip_lib().evc_lpips_layer_f32(fptr(f0), fptr(f1), fptr(lin_w), fptr(dist), N, H * W, C, int(bool(accumulate)),
                                         stream_ptr()), "evc_lpips_layer_f32")
    return dist


def pool_out_size(size, k, stride, ceil_mode):
    """torch's pooling output size without padding: in ceil mode the last window must start inside the input."""
    num = size - k + (stride - 1 if ceil_mode else 0)
    if num < 0:
        raise ValueError(f"max pool {k} stride {stride} of a side of {size}: no output")
    o = num // stride + 1
    return o - 1 if ceil_mode and (o - 1) * stride >= size else o


def maxpool2d_nhwc(x, k, stride, ceil_mode=False):
    """MaxPool2d(k, stride, ceil_mode=...) without padding, k in {2, 3}; x: (N, H, W, C), C % 4 == 0 (include/evc_hip.h)."""
    N, H, W, C = x.shape
    out = torch.empty((N, pool_out_size(H, k, stride, ceil_mode), pool_out_size(W, k, stride, ceil_mode), C), device=x.device,
                      dtype=torch.float32)
    _check(hip_lib().evc_maxpool2d_nhwc_f32(fptr(x), fptr(out), N, H, W, C, k, stride, int(bool(ceil_mode)), stream_ptr()),
           "evc_maxpool2d_nhwc_f32")
    return out


def lpips_map(f0, f1, lin_w, out=None):
    """(N, H, W) per-pixel distances of one tap: lin_w . (unit-normalised f0 - unit-normalised f1)^2; f0, f1: (N, H, W, C)."""
    N, H, W, C = f0.shape
    assert f1.shape == f0.shape and lin_w.numel() == C
    if out is None:
        out = torch.empty((N, H, W), device=f0.device, dtype=torch.float32)
    assert out.numel() == N * H * W
    _check(hip_lib().evc_lpips_map_f32(fptr(f0), fptr(f1), fptr(lin_w), fptr(out), N, H * W, C, stream_ptr()), "evc_lpips_map_f32")
    return out


def lpips_map_mean(m, dist, accumulate):
    """dist[n] (+)= mean of m[n]; m: (N, H, W) or (N, HW)."""
    N = m.shape[0]
    assert dist.numel() == N
    _check(hip_lib().evc_lpips_map_mean_f32(fptr(m), fptr(dist), N, m.numel() // N, int(bool(accumulate)), stream_ptr()),
           "evc_lpips_map_mean_f32")
    return dist


def lpips_upsample_add(m, out, accumulate):
    """out[n] (+)= bilinear(m[n], size=out.shape[1:], align_corners=False); m: (N, h, w), out: (N, H, W)."""
    N, h, w = m.shape
    assert out.shape[0] == N and out.dim() == 3
    _check(hip_lib().evc_lpips_upsample_add_f32(fptr(m), fptr(out), N, h, w, out.shape[1], out.shape[2], int(bool(accumulate)),
                                                stream_ptr()), "evc_lpips_upsample_add_f32")
    return out


def same_pad(size, k, s):
    """TensorFlow "same" padding of I3D (include/evc_hip.h): (front, back)."""
    p = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return p // 2, p - p // 2


def i3d_stem_im2col(x, Hr, Wr, R, k, s, f_begin, out):
    """x: (B, T, C, H, W) clips in [0, 1] -> ``out`` (nf, Ho, Wo, ld_out): rows of output frames f_begin .. f_begin + nf - 1 of
    the k^3 stride-s first I3D convolution over the resized (Hr x Wr), centre-cropped (R x R), [-1, 1]-scaled, same-padded clip."""
    B, T, C, H, W = x.shape
    nf, Ho, Wo, ld = out.shape
    To = (T + sum(same_pad(T, k, s)) - k) // s + 1
    assert (Ho, Wo) == ((R + sum(same_pad(R, k, s)) - k) // s + 1,) * 2 and f_begin + nf <= B * To
    _check(hip_lib().evc_i3d_stem_im2col_f32(fptr(x), fptr(out), B, T, C, H, W, Hr, Wr, R, k, k, k, s, s, s, f_begin, nf, ld,
                                             stream_ptr()), "evc_i3d_stem_im2col_f32")
    return out


def maxpool3d_same_nthwc(x, T, kernel, stride):
    """MaxPool3dSamePadding on (B*T, H, W, C) NTHWC activations -> (B*To, Ho, Wo, C); zero padding, as the reference pads."""
    BT, H, W, C = x.shape
    assert BT % T == 0
    B = BT // T
    To, Ho, Wo = ((n + sum(same_pad(n, k, s)) - k) // s + 1 for n, k, s in zip((T, H, W), kernel, stride))
    out = torch.empty((B * To, Ho, Wo, C), device=x.device, dtype=torch.float32)
    _check(hip_lib().evc_maxpool3d_same_nthwc_f32(fptr(x), fptr(out), B, T, H, W, C, *kernel, *stride, stream_ptr()),
           "evc_maxpool3d_same_nthwc_f32")
    return out


def i3d_head(x, T, w, bias, kt):
    """x: (B*T, H, W, C) -> (B, Co): AvgPool3d((kt, H, W), stride 1), 1x1x1 logits unit w (Co, C) + bias, mean over windows."""
    BT, H, W, C = x.shape
    assert BT % T == 0 and w.shape[1] == C
    out = torch.empty((BT // T, w.shape[0]), device=x.device, dtype=torch.float32)
    _check(hip_lib().evc_i3d_head_f32(fptr(x), fptr(w), fptr(bias), fptr(out), BT // T, T, H * W, C, w.shape[0], kt,
                                      stream_ptr()), "evc_i3d_head_f32")
    return out


INCEPTION_RES, INCEPTION_STEM_OUT = 299, 149      # the resize target and the side of Conv2d_1a_3x3's output
POOL_AVG, POOL_MAX = 0, 1                         # include/evc_hip.h EVC_POOL_*


def inception_stem_im2col(x, f_begin, out):
    """x: (N, 3, H, W) images in [0, 1] -> ``out`` (nf, 149, 149, ld_out): the patch rows of Conv2d_1a_3x3 (3x3, stride 2) over
    2 * bilinear(x, 299 x 299) - 1 for the images f_begin .. f_begin + nf - 1, (c, ky, kx) order, zeros from column 27."""
    N, C, H, W = x.shape
    nf, Ho, Wo, ld = out.shape
    assert (Ho, Wo) == (INCEPTION_STEM_OUT, INCEPTION_STEM_OUT) and f_begin + nf <= N
    _check(hip_lib().evc_inception_stem_im2col_f32(fptr(x), fptr(out), N, C, H, W, f_begin, nf, ld, stream_ptr()),
           "evc_inception_stem_im2col_f32")
    return out


def im2col_nhwc(x, KH, KW, stride=(1, 1), pad=(0, 0), ld_out=None, out=None):
    """x: (N, H, W, C) -> (N, Ho, Wo, ld_out) patch rows in (ky, kx, c) order, zeros beyond KH*KW*C (include/evc_hip.h)."""
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad[0] - KH) // stride[0] + 1, (W + 2 * pad[1] - KW) // stride[1] + 1
    ld = KH * KW * C if ld_out is None else ld_out
    if Ho < 1 or Wo < 1:
        raise ValueError(f"im2col_nhwc: a {KH} x {KW} window with padding {tuple(pad)} does not fit {H} x {W}")
    if out is None:
        out = torch.empty((N, Ho, Wo, ld), device=x.device, dtype=torch.float32)
    assert tuple(out.shape) == (N, Ho, Wo, ld)
    _check(hip_lib().evc_im2col_nhwc_f32(fptr(x), fptr(out), N, H, W, C, KH, KW, stride[0], stride[1], pad[0], pad[1], ld,
                                         stream_ptr()), "evc_im2col_nhwc_f32")
    return out


def pool3x3s1p1_nhwc(x, mode):
    """3x3 stride-1 padding-1 pool of (N, H, W, C): POOL_AVG = avg_pool2d(count_include_pad=False), POOL_MAX = max_pool2d."""
    N, H, W, C = x.shape
    out = torch.empty_like(x)
    _check(hip_lib().evc_pool3x3s1p1_nhwc_f32(fptr(x), fptr(out), N, H, W, C, mode, stream_ptr()), "evc_pool3x3s1p1_nhwc_f32")
    return out


def spatial_mean_nhwc(x):
    """(N, H, W, C) or (N, HW, C) -> (N, C): the mean over the pixels, summation order a function of HW only."""
    N, C = x.shape[0], x.shape[-1]
    out = torch.empty((N, C), device=x.device, dtype=torch.float32)
    _check(hip_lib().evc_spatial_mean_nhwc_f32(fptr(x), fptr(out), N, x.numel() // max(N * C, 1), C, stream_ptr()),
           "evc_spatial_mean_nhwc_f32")
    return out


def knn_radius(x, k):
    """x: (n, d) float32 -> (n,) float64: the squared distance of every row to its (k + 1)-th nearest row, itself included."""
    n, d = x.shape
    out = torch.empty((n,), device=x.device, dtype=torch.float64)
    _check(hip_lib().evc_knn_radius_f32(fptr(x), fptr(out, torch.float64), n, d, k, stream_ptr()), "evc_knn_radius_f32")
    return out


def manifold_hits(y, x, radius2):
    """(m,) int32 flags: row i of y (m, d) lies within squared distance radius2[j] of some row j of x (n, d)."""
    m, d = y.shape
    n = x.shape[0]
    assert x.shape[1] == d and radius2.numel() == n
    out = torch.empty((m,), device=y.device, dtype=torch.int32)
    _check(hip_lib().evc_manifold_hits_f32(fptr(y), fptr(x), fptr(radius2, torch.float64), fptr(out, torch.int32), m, n, d,
                                           stream_ptr()), "evc_manifold_hits_f32")
    return out


class ClockProbe:
    """Shader clock held by the chip while other streams work, measured by a one-wave idle kernel on its own stream
    (``evc_clock_probe``): start it, enqueue the work to be characterised, call ``stop()`` (a stream-ordered write behind that
    work on the CURRENT stream: the probe ends with it, or after ``max_us`` at the latest), then read ``ghz()``."""

    def __init__(self, max_us, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.out = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))          # the two zero-fills above
        _check(hip_lib().evc_clock_probe(self.out.data_ptr(), int(max_us), self.flag.data_ptr(), self.stream.cuda_stream),
               "evc_clock_probe")

    def stop(self):
        self.flag.fill_(1)

    def ghz(self):
        self.stream.synchronize()
        ticks, ref = (int(v) for v in self.out.tolist())
        return ticks / ref * 0.1 if ref else None

    def seconds(self):
        return int(self.out[1]) / 1e8


def gpu_power_w(device=None):
    """Average package power (W) of ``device`` from sysfs (hwmon power1_average of the card with the device's PCI address), or
    None where that is not readable.  Read-only; the figure is the driver's ~1 s moving average."""
    import glob as _glob
    try:
        pr = torch.cuda.get_device_properties(torch.cuda.current_device() if device is None else torch.device(device).index)
        addr = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}."
        for card in _glob.glob("/sys/class/drm/card*/device"):
            if addr in os.path.realpath(card):
                for f in _glob.glob(card + "/hwmon/hwmon*/power1_average") + _glob.glob(card + "/hwmon/hwmon*/power1_input"):
                    return int(open(f).read()) / 1e6
    except Exception:
        return None
    return None


def gn_coeffs(parts, HW, groups, eps, mode=0, gamma=None, beta=None, ss=None, row=None, bound=None, site=None,
              invariant=False):
    """parts: one or two partial-moment tensors (virtual concat). Returns (coef_a, coef_s), each (B, C).
    ``bound``: optional one-element int32 tensor (zeroed by the caller) raised to the bit pattern of the tensors'
    element bound S (|x| <= sqrt(S)) -- what ``conv2d_nhwc(..., in_bound=)`` takes.  ``site``: a ``Site`` that also
    receives this call's range events."""
    L = hip_lib()
    p0 = parts[0]
    p1 = parts[1] if len(parts) > 1 else None
    B, ns0, C0, _ = p0.shape
    ns1, C1 = (p1.shape[1], p1.shape[2]) if p1 is not None else (0, 0)
    C = C0 + C1
    ca = torch.empty((B, C), device=p0.device, dtype=torch.float32)
    cs = torch.empty((B, C), device=p0.device, dtype=torch.float32)
    ss_ld = 0 if ss is None else ss.stride(0)
    ssp = c_void_p(ss.data_ptr()) if ss is not None else None
    if bool(invariant) and bound is not None:        # one bound word per sample
        ev, sw, si = _site_args(site, p0.device)
        _check(L.evc_gn_coeffs_bound_sample_f32(fptr(p0), ns0, C0, fptr(p1), ns1, C1, B, HW, groups, eps, mode, fptr(gamma),
                                                fptr(beta), ssp, ss_ld, fptr(row, torch.int32), fptr(ca), fptr(cs),
                                                _word(bound, B), ev, sw, si, stream_ptr()),
               "evc_gn_coeffs_bound_sample_f32")
        return ca, cs
    if site is None:
        _check(L.evc_gn_coeffs_bound_f32(fptr(p0), ns0, C0, fptr(p1), ns1, C1, B, HW, groups, eps, mode, fptr(gamma),
                                         fptr(beta), ssp, ss_ld, fptr(row, torch.int32), fptr(ca), fptr(cs), _word(bound),
                                         _word(_events(p0.device)), stream_ptr()),
               "evc_gn_coeffs_bound_f32")
    else:
        _check(L.evc_gn_coeffs_bound_site_f32(fptr(p0), ns0, C0, fptr(p1), ns1, C1, B, HW, groups, eps, mode, fptr(gamma),
                                              fptr(beta), ssp, ss_ld, fptr(row, torch.int32), fptr(ca), fptr(cs),
                                              _word(bound), *_site_args(site, p0.device), stream_ptr()),
               "evc_gn_coeffs_bound_site_f32")
    return ca, cs


def _word(t, n=1):
    """Device pointer of an n-element int32 tensor (or view), None when absent."""
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.int32 and t.numel() == n and t.is_contiguous()
    return c_void_p(t.data_ptr())


def moments_bound(part, c_begin, c_count, bound, site=None, invariant=False):
    """Raise ``bound[z]`` to the element bound of channels [c_begin + z*c_count, + c_count) of a moments tensor
    (B, ns, C, 2), for z < bound.numel().  ``site``: as in ``gn_coeffs``."""
    B, ns, C, _ = part.shape
    n = bound.numel()
    if bool(invariant):                              # bound: (B, n_ranges) words, sample-major
        assert n % B == 0
        ev, sw, si = _site_args(site, part.device)
        _check(hip_lib().evc_moments_bound_sample_f32(fptr(part), ns, C, c_begin, c_count, n // B, B, _word(bound, n),
                                                      ev, sw, si, stream_ptr()), "evc_moments_bound_sample_f32")
        return
    if site is not None:
        _check(hip_lib().evc_moments_bound_site_f32(fptr(part), ns, C, c_begin, c_count, n, B, _word(bound, n),
                                                    *_site_args(site, part.device), stream_ptr()),
               "evc_moments_bound_site_f32")
        return
    _check(hip_lib().evc_moments_bound_f32(fptr(part), ns, C, c_begin, c_count, n, B, _word(bound, n),
                                           _word(_events(part.device)), stream_ptr()),
           "evc_moments_bound_f32")


def affine_act(x, coef, act, out=None, coef_col=0):
    """y = act(x * a + s).  ``out`` may be a ``Cols`` slice of a wider buffer; ``coef_col`` selects the channel
    offset inside wider (B, Ctot) coefficient tensors (both let a concat be activated piecewise)."""
    L = hip_lib()
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    po, Cout, ldo, _ = _src(out)
    assert Cout == C
    ca, cs = coef if coef is not None else (None, None)
    ldc = 0 if ca is None else ca.shape[-1]
    pa = None if ca is None else c_void_p(ca.data_ptr() + 4 * coef_col)
    ps = None if cs is None else c_void_p(cs.data_ptr() + 4 * coef_col)
    _check(L.evc_affine_act_nhwc_f32(fptr(x), po, pa, ps, act, B, H * W, C, ldc, ldo, stream_ptr()),
           "evc_affine_act_nhwc_f32")
    return out.t if isinstance(out, Cols) else out


def spade_act(x, coef, maps, ctot, col=0, ss=None, row=None, act=ACT_SILU, out=None):
    """SPADE act-norm of one part of a (virtual) concat: ``x`` (B, H, W, C) contiguous; ``coef`` = (a, s), each (B, ctot);
    ``maps`` (B, H, W, 2*ctot) = [1 + gamma | beta]; ``ss`` the AdaGN table slice (rows, 2*ctot) = [scale | shift] (None:
    no time embedding); ``col`` the part's channel offset inside the concat; ``out`` a tensor or ``Cols`` slice."""
    L = hip_lib()
    B, H, W, C = x.shape
    assert x.is_contiguous() and maps.is_contiguous() and maps.shape == (B, H, W, 2 * ctot) and col + C <= ctot
    if out is None:
        out = torch.empty_like(x)
    po, Cout, ldo, _ = _src(out)
    assert Cout == C
    ca, cs = coef
    assert ca.shape == (B, ctot) and cs.shape == (B, ctot)
    off = lambda t, c: c_void_p(t.data_ptr() + 4 * c)
    ps = psh = None
    ld_ss = 0
    if ss is not None:
        assert ss.shape[1] == 2 * ctot and ss.stride(1) == 1
        ps, psh, ld_ss = off(ss, col), off(ss, ctot + col), ss.stride(0)
    _check(L.evc_spade_act_nhwc_f32(fptr(x), po, off(ca, col), off(cs, col), ctot, off(maps, col), off(maps, ctot + col),
                                    2 * ctot, ps, psh, ld_ss, fptr(row, torch.int32), act, B, H * W, C, ldo, stream_ptr()),
           "evc_spade_act_nhwc_f32")
    return out.t if isinstance(out, Cols) else out


def conv_pack_weights(w, arith=None):
    """w: (Co, Ci, KH, KW) device float32 with Ci % 16 == 0 -> packed flat tensor: float32 for ARITH_F32, bfloat16
    (three planes) for ARITH_BF16X6, float16 (header + two planes) for ARITH_F16X3; ``conv2d_nhwc`` picks the kernel
    from that dtype."""
    L = hip_lib()
    arith = default_arith() if arith is None else arith
    w = w.contiguous()
    Co, Ci, KH, KW = w.shape
    nbytes = L.evc_conv_packed_bytes(Co, Ci, KH, KW, arith)
    if nbytes < 0:
        raise EvcKernelError(f"evc_conv_packed_bytes rejected the arguments ({nbytes})")
    if arith not in _ARITH_DTYPES:
        raise EvcKernelError(f"unknown convolution arithmetic {arith}")
    dt = _ARITH_DTYPES[arith]
    packed = torch.empty((nbytes // dt.itemsize,), device=w.device, dtype=dt)
    _check(L.evc_conv_pack_weights(fptr(w), ptr(packed), Co, Ci, KH, KW, arith, stream_ptr()), "evc_conv_pack_weights")
    return packed


def conv_set_option(name, value):
    """Dispatch switches of the convolution ("wide_tiles", "row_reuse", "tail_split", "wide256"): include/evc_hip.h."""
    _check(hip_lib(require_device=False).evc_conv_set_option(name.encode(), int(value)), "evc_conv_set_option")


def packed_arith(w_packed):
    return {torch.bfloat16: ARITH_BF16X6, torch.float16: ARITH_F16X3}.get(w_packed.dtype, ARITH_F32)


_ws_cache = {}

# Optional launch profiler (bench.py roofline leg): when a list is installed here every conv launch is
# bracketed by HIP events recorded on the stream the kernel runs on.
CONV_PROFILE = None


def conv_variant(Co):
    """Which conv_igemm_kernel<TN> instantiation serves an output width (mirrors pick_tn in conv_igemm.hip)."""
    # A restatement of the C function pick_tn(evc_conv_co_pad(Co)) (csrc/conv_igemm.hip), kept only because bench.py reads
    # ``variant`` from the profile records; the kernel a launch really runs is the record's ``kernel`` (evc_conv_kernel_name).
    cp = (Co + 63) // 64 * 64
    return 3 if cp % 192 == 0 else (2 if cp % 128 == 0 else 1)


def _workspace(nbytes, device):
    """Split-K workspace.  Eager launches: one grow-only buffer per (device, stream), reused stream-ordered.
    Inside a HIP-graph capture every graph must own its buffer (all captures share one capture stream, and
    graphs replayed concurrently on different streams would otherwise race on it): allocate from the graph pool."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(((nbytes + 3) // 4,), device=device, dtype=torch.float32)
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    cur = _ws_cache.get(key)
    if cur is None or cur.numel() * 4 < nbytes:
        cur = torch.empty(((nbytes + 3) // 4,), device=device, dtype=torch.float32)
        _ws_cache[key] = cur
    return cur


class Cols:
    """A channel slice [c0, c0 + C) of a contiguous NHWC tensor, usable as a conv source or destination."""
    __slots__ = ("t", "c0", "C")

    def __init__(self, t, c0, C):
        assert t.is_contiguous() and 0 <= c0 and c0 + C <= t.shape[-1] and c0 % 4 == 0
        self.t, self.c0, self.C = t, c0, C


def _src(s):
    """-> (pointer, channels, row stride, shape[:3])"""
    if s is None:
        return None, 0, 0, None
    if isinstance(s, Cols):
        return c_void_p(s.t.data_ptr() + 4 * s.c0), s.C, s.t.shape[-1], s.t.shape[:3]
    return ptr(s), s.shape[-1], s.shape[-1], s.shape[:3]


def conv_query_args(B, H, W, C0, C1, Co, KH, KW, arith, coef=False, act_in=ACT_NONE, splits=0, x2_ci=0, invariant=False):
    """``ConvArgs`` for the planner queries below (no launch, works without a GPU): shapes, arithmetic, on-load mode
    (``coef``: GroupNorm coefficients, ``act_in``), forced splits, channels of a fused 1x1 operand, the batch-invariant flag.
    The queries read shapes and which pointers are set, never memory, so every pointer is a non-null dummy."""
    d = c_void_p(16)
    a = ConvArgs(src0=d, src1=d if C1 else None, C0=C0, C1=C1, coef_a=d if coef else None, coef_s=d if coef else None,
                 act_in=act_in, w_packed=d, out_scale=1.0, act_out=ACT_NONE, out=d, ld_out=Co, B=B, H=H, W=W, Co=Co, KH=KH,
                 KW=KW, splits=splits, arith=arith, invariant=int(bool(invariant)))
    if x2_ci:
        a.x2_src0, a.x2_C0, a.x2_w_packed, a.x2_bound = d, x2_ci, d, d
    return a


def conv_fused_1x1_supported(B, H, W, Ci, Co, arith, splits=0, invariant=False):
    """Whether a 3x3 convolution of this shape may carry a fused 1x1 operand (``conv2d_nhwc(..., x2=)``): C query.  It
    needs the f16x3 row-reuse kernel, i.e. 128-pixel tiles: very small grids, for which 64-pixel tiles are chosen, do not."""
    a = conv_query_args(B, H, W, Ci, 0, Co, 3, 3, arith, splits=splits, invariant=invariant)
    return bool(hip_lib(require_device=False).evc_conv_fused_1x1_supported(ctypes.byref(a)))


def conv_plan(B, H, W, C0, C1, Co, K, arith, coef=False, act_in=ACT_NONE, x2_ci=0, invariant=False, splits=0):
    """The whole plan of a convolution without a launch (``evc_conv_plan_query``; works without a GPU): a dict of the kernel
    instance, tile, K split (count, steps per split, cut), K-split tail, fused-moment runs and whether a fused 1x1 operand
    is accepted.  ``coef`` / ``act_in``: the on-load mode (GroupNorm coefficients, activation); ``x2_ci``: channels of a
    fused 1x1 operand (f16x3 only).  The C query refuses a fused operand the plan cannot carry, as the launch does; the
    answer is then the plan of the launch without it (``fused_1x1`` False), which is what the network launches instead."""
    L = hip_lib(require_device=False)
    out = ConvPlan()
    a = conv_query_args(B, H, W, C0, C1, Co, K, K, arith, coef, act_in, splits, x2_ci, invariant)
    rc = L.evc_conv_plan_query(ctypes.byref(a), ctypes.byref(out))
    if rc != 0 and x2_ci:
        a = conv_query_args(B, H, W, C0, C1, Co, K, K, arith, coef, act_in, splits, 0, invariant)
        rc = L.evc_conv_plan_query(ctypes.byref(a), ctypes.byref(out))
    _check(rc, "evc_conv_plan_query")
    return dict(kernel=out.kernel.decode(), tile=(out.tile_m, out.tile_n), splits=out.splits,
                steps_per_split=out.steps_per_split, cut_chunk=out.cut_chunk, tail_tiles=out.tail_tiles,
                tail_splits=out.tail_splits, stats_runs=out.stats_runs, fused_1x1=bool(out.fused_1x1))


def conv_accepts(B, H, W, Ci, Co, KH, KW, arith, invariant=False):
    """Whether ``conv2d_nhwc`` takes a plain KH x KW "same" convolution of this shape: ``evc_conv_plan_query`` and
    ``evc_conv_workspace_bytes`` both answer without an error code (no launch, works without a GPU).  A caller with another
    route for the layer (``im2col_nhwc`` + 1x1) asks this first."""
    lib = hip_lib(require_device=False)
    a = conv_query_args(B, H, W, Ci, 0, Co, KH, KW, arith, invariant=invariant)
    return lib.evc_conv_plan_query(ctypes.byref(a), ctypes.byref(ConvPlan())) == 0 and \
        lib.evc_conv_workspace_bytes(ctypes.byref(a)) >= 0


def conv2d_nhwc(src0, w_packed, Co, KH, KW, bias=None, src1=None, coef=None, act_in=ACT_NONE, res=None,
                out_scale=1.0, act_out=ACT_NONE, out=None, splits=0, want_stats=False, in_bound=None, x2=None,
                invariant=False):
    """out = act_out((conv(act_in(cat[src0,src1]*a+s), w) + bias + res) * out_scale); tensors are NHWC.
    ``src0`` / ``src1`` / ``out`` may be ``Cols`` channel slices of wider tensors.
    ``x2 = (x2_src0, x2_src1 or None, w2_packed, bound)``: a fused 1x1 operand -- conv1x1(cat[x2_src0, x2_src1], w2) is
    accumulated into the same output (include/evc_hip.h); ``bias`` must then be the sum of both convolutions' biases.
    ``want_stats=True`` returns ``(out, stats)``: per-channel moments of ``out`` in ``chan_stats`` layout, produced
    by the conv epilogue when the shape allows it, else by a separate ``evc_chan_stats_f32`` pass.
    ``invariant``: the batch-invariant plan; ``in_bound`` / the bound of ``x2`` then hold one word per sample."""
    L = hip_lib()
    inv = bool(invariant)
    p0, C0, ld0, shp = _src(src0)
    p1, C1, ld1, shp1 = _src(src1)
    assert shp1 is None or tuple(shp1) == tuple(shp)
    B, H, W = shp
    dev = (src0.t if isinstance(src0, Cols) else src0).device
    if out is None:
        out = torch.empty((B, H, W, Co), device=dev, dtype=torch.float32)
    po, Cout, ldo, shpo = _src(out)
    assert tuple(shpo) == (B, H, W) and Cout >= Co
    ca, cs = coef if coef is not None else (None, None)
    a = ConvArgs(p0, p1, C0, C1, ld0, ld1, ptr(ca), ptr(cs), act_in, ptr(w_packed), ptr(bias), ptr(res),
                 0 if res is None else res.shape[-1], float(out_scale), act_out, po, ldo,
                 B, H, W, Co, KH, KW, splits, None, packed_arith(w_packed), _word(in_bound, B if inv else 1))
    a.invariant = int(inv)
    x2_ci = 0
    if x2 is not None:
        q0, qC0, qld0, qshp = _src(x2[0])
        q1, qC1, qld1, _ = _src(x2[1])
        assert tuple(qshp) == (B, H, W) and x2[2].dtype == torch.float16
        a.x2_src0, a.x2_src1, a.x2_C0, a.x2_C1, a.x2_ld0, a.x2_ld1 = q0, q1, qC0, qC1, qld0, qld1
        a.x2_w_packed, a.x2_bound = ptr(x2[2]), _word(x2[3], B if inv else 1)
        x2_ci = qC0 + qC1
    stats = None
    if want_stats:
        ns = L.evc_conv_stats_splits(ctypes.byref(a))
        if ns > 0:
            stats = torch.empty((B, ns, Co, 2), device=dev, dtype=torch.float32)
            a.stats_out = ptr(stats)
    nbytes = L.evc_conv_workspace_bytes(ctypes.byref(a))
    if nbytes < 0:
        raise EvcKernelError(f"evc_conv_workspace_bytes rejected the arguments ({nbytes})")
    ws = _workspace(nbytes, dev) if nbytes > 0 else None
    if CONV_PROFILE is not None:
        # e0 .. ec: the convolution kernel alone (recorded inside the C call, before the split-K combine); e0 .. e1: with it
        st = torch.cuda.current_stream()
        e0, ec, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(st); ec.record(st)          # (a torch event owns a hipEvent_t only once it has been recorded)
        _check(L.evc_conv2d_nhwc_profiled_f32(ctypes.byref(a), ptr(ws), stream_ptr(), c_void_p(e0.cuda_event),
                                              c_void_p(ec.cuda_event)), "evc_conv2d_nhwc_profiled_f32")
        e1.record(st)
        kbuf = ctypes.create_string_buffer(96)
        L.evc_conv_kernel_name(ctypes.byref(a), kbuf, 96)
        CONV_PROFILE.append(dict(variant=conv_variant(Co), split=nbytes > 0, e0=e0, ec=ec, e1=e1, arith=a.arith,
                                 kernel=kbuf.value.decode(),
                                 flops=2.0 * B * H * W * Co * (KH * KW * (C0 + C1) + x2_ci),
                                 shape=(B, H, W, C0 + C1, Co, KH),
                                 call=dict(B=B, H=H, W=W, C0=C0, C1=C1, Co=Co, K=KH, coef=coef is not None, act_in=act_in,
                                           res=res is not None, out_scale=float(out_scale), bias=bias is not None,
                                           bound=in_bound is not None, arith=a.arith, ld_out=ldo,
                                           stats=bool(want_stats), x2=x2_ci, invariant=inv)))
    else:
        _check(L.evc_conv2d_nhwc_f32(ctypes.byref(a), ptr(ws), stream_ptr()), "evc_conv2d_nhwc_f32")
    result = out.t if isinstance(out, Cols) else out
    if want_stats:
        return result, (stats if stats is not None else chan_stats(result, invariant=inv))
    return result


def conv_fused_stats_splits(B, H, W, Ci, Co, KH, KW, splits=0, arith=None):
    """HW/64 or HW/32 when ``conv2d_nhwc(..., want_stats=True)`` gets its moments from the conv epilogue / split-K
    combine for this shape, 0 when it falls back to a separate ``evc_chan_stats_f32`` pass (C query, no launch)."""
    a = conv_query_args(B, H, W, Ci, 0, Co, KH, KW, default_arith() if arith is None else arith, splits=splits)
    return hip_lib(require_device=False).evc_conv_stats_splits(ctypes.byref(a))


def conv_workspace_bytes(B, H, W, Ci, Co, KH, KW, splits=0, arith=None):
    """Bytes of split-K slabs ``conv2d_nhwc`` takes for this shape: 0 for an unsplit grid, splits x output for split-K,
    tail splits x tail rows when only the last partial round of tiles is split (C query, no launch)."""
    a = conv_query_args(B, H, W, Ci, 0, Co, KH, KW, default_arith() if arith is None else arith, splits=splits)
    return hip_lib(require_device=False).evc_conv_workspace_bytes(ctypes.byref(a))


# ---- NIN projections of the attention blocks as a plain GEMM (csrc/nin_gemm.hip): a separate operation, not a convolution
# plan -- ``conv2d_nhwc`` never launches it.  A caller asks ``nin_gemm_supported`` and keeps ``conv2d_nhwc`` where it says no.
# Optional launch log: when a list is installed here every ``nin_gemm`` call appends its shape and plan.
NIN_PROFILE = None


def nin_query_args(B, H, W, Ci, Co, arith=ARITH_F16X3, coef=False, bound=None, two_sources=False, act_out=ACT_NONE, tile=0):
    """``NinArgs`` for the queries below (no launch, works without a GPU): they read shapes and which pointers are set, never
    memory, so every pointer is a non-null dummy.  ``bound`` defaults to the raw form when there are no coefficients."""
    d = c_void_p(16)
    bound = (not coef) if bound is None else bound
    return NinArgs(x=d, x1=d if two_sources else None, Ci=Ci, Co=Co, coef_a=d if coef else None, coef_s=d if coef else None,
                   in_bound=d if bound else None, w_packed=d, arith=arith, out_scale=1.0, act_out=act_out, out=d,
                   B=B, H=H, W=W, tile=tile)


def nin_gemm_supported(B, H, W, Ci, Co, arith=ARITH_F16X3, coef=False, **kw):
    """Whether ``nin_gemm`` takes this projection (``evc_nin_gemm_supported``; works without a GPU)."""
    a = nin_query_args(B, H, W, Ci, Co, arith, coef, **kw)
    return bool(hip_lib(require_device=False).evc_nin_gemm_supported(ctypes.byref(a)))


def nin_gemm_plan(B, H, W, Ci, Co, arith=ARITH_F16X3, coef=False, **kw):
    """The launch's plan (``evc_nin_gemm_plan_query``; works without a GPU): kernel instance, tile, K stages, moment runs."""
    out = NinPlan()
    a = nin_query_args(B, H, W, Ci, Co, arith, coef, **kw)
    _check(hip_lib(require_device=False).evc_nin_gemm_plan_query(ctypes.byref(a), ctypes.byref(out)), "evc_nin_gemm_plan_query")
    return dict(kernel=out.kernel.decode(), tile=(out.tile_m, out.tile_n), stages=out.stages, stats_runs=out.stats_runs)


def nin_gemm(x, w_packed, Co, bias=None, coef=None, res=None, out_scale=1.0, in_bound=None, want_stats=False, out=None,
             tile=0):
    """out = ((T(x) @ w^T) + bias + res) * out_scale on dense NHWC tensors: the 1x1 convolution of an attention block's
    projection as one GEMM launch without K split (include/evc_hip.h).  T(x) = x * a + s with ``coef = (a, s)`` (an affine
    GroupNorm), or x scaled from the element bound word ``in_bound``.  ``w_packed``: the F16X3 pack ``conv2d_nhwc`` takes for
    the same filter.  ``want_stats=True`` returns ``(out, stats)`` with the moments of ``out`` in ``chan_stats`` layout.
    Raises where ``nin_gemm_supported`` says no: there is no fallback here."""
    L = hip_lib()
    B, H, W, Ci = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32 and (res is None or (res.is_contiguous() and res.shape == (B, H, W, Co)))
    if out is None:
        out = torch.empty((B, H, W, Co), device=x.device, dtype=torch.float32)
    assert out.is_contiguous() and out.shape == (B, H, W, Co)
    ca, cs = coef if coef is not None else (None, None)
    assert ca is None or (ca.shape == (B, Ci) and cs.shape == (B, Ci) and ca.is_contiguous() and cs.is_contiguous())
    a = NinArgs(x=ptr(x), x1=None, Ci=Ci, Co=Co, coef_a=ptr(ca), coef_s=ptr(cs), in_bound=_word(in_bound),
                w_packed=ptr(w_packed), arith=packed_arith(w_packed), bias=ptr(bias), res=ptr(res), out_scale=float(out_scale),
                act_out=ACT_NONE, out=ptr(out), B=B, H=H, W=W, tile=tile)
    plan = NinPlan()
    _check(L.evc_nin_gemm_plan_query(ctypes.byref(a), ctypes.byref(plan)), "evc_nin_gemm_plan_query")
    stats = None
    if want_stats:
        stats = torch.empty((B, plan.stats_runs, Co, 2), device=x.device, dtype=torch.float32)
        a.stats_out = ptr(stats)
    _check(L.evc_nin_gemm_f32(ctypes.byref(a), stream_ptr()), "evc_nin_gemm_f32")
    if NIN_PROFILE is not None:
        NIN_PROFILE.append(dict(kernel=plan.kernel.decode(), tile=(plan.tile_m, plan.tile_n), shape=(B, H, W, Ci, Co),
                                coef=coef is not None, bound=in_bound is not None, res=res is not None, stats=bool(want_stats)))
    return (out, stats) if want_stats else out


# ---- 3x3 convolutions of the 16 x 16 / 8 x 8 levels with the K groups inside the workgroup (csrc/conv_small.hip): a separate
# operation like ``nin_gemm`` -- ``conv2d_nhwc`` never launches it, a caller asks ``small_conv_supported`` and keeps
# ``conv2d_nhwc`` where it says no.  Optional launch log: every ``small_conv`` call appends its shape and plan.
SMALL_CONV_PROFILE = None


def small_conv_query_args(B, H, W, C0, C1, Co, K=3, arith=ARITH_F16X3, coef=False, act_in=None, bound=False, act_out=ACT_NONE,
                          x2=False, invariant=False, variant=0):
    """``SmallConvArgs`` for the queries below (no launch, works without a GPU): they read shapes and which pointers are set,
    never memory, so every pointer is a non-null dummy.  ``act_in`` defaults to the form's own (SiLU with coefficients)."""
    d = c_void_p(16)
    act_in = (ACT_SILU if coef else ACT_NONE) if act_in is None else act_in
    return SmallConvArgs(src0=d, src1=d if C1 else None, C0=C0, C1=C1, coef_a=d if coef else None, coef_s=d if coef else None,
                         act_in=act_in, in_bound=d if bound else None, w_packed=d, arith=arith, out_scale=1.0, act_out=act_out,
                         out=d, B=B, H=H, W=W, Co=Co, KH=K, KW=K, x2_w_packed=d if x2 else None, invariant=int(bool(invariant)),
                         variant=variant)


def small_conv_supported(B, H, W, C0, C1, Co, **kw):
    """Whether ``small_conv`` takes this convolution (``evc_small_conv_supported``; works without a GPU)."""
    a = small_conv_query_args(B, H, W, C0, C1, Co, **kw)
    return bool(hip_lib(require_device=False).evc_small_conv_supported(ctypes.byref(a)))


def small_conv_plan(B, H, W, C0, C1, Co, **kw):
    """The launch's plan (``evc_small_conv_plan_query``; works without a GPU): kernel instance and its number, tile, K groups,
    chunks, rounds (chunks of the longest group), moment runs."""
    out = SmallConvPlan()
    a = small_conv_query_args(B, H, W, C0, C1, Co, **kw)
    _check(hip_lib(require_device=False).evc_small_conv_plan_query(ctypes.byref(a), ctypes.byref(out)), "evc_small_conv_plan_query")
    return dict(kernel=out.kernel.decode(), variant=out.variant, tile=(out.tile_m, out.tile_n), groups=out.groups,
                chunks=out.chunks, rounds=out.rounds, stats_runs=out.stats_runs)


def small_conv(src0, w_packed, Co, bias=None, src1=None, coef=None, act_in=ACT_NONE, res=None, out_scale=1.0, in_bound=None,
               want_stats=False, out=None, variant=0):
    """out = (conv3x3(T(cat[src0, src1]), w) + bias + res) * out_scale on dense NHWC tensors with H = W in {8, 16}: one launch,
    the K range divided over wave groups inside each workgroup (include/evc_hip.h).  T = SiLU of the GroupNorm affine with
    ``coef = (a, s)`` and ``act_in=ACT_SILU``, or nothing; ``in_bound``: the sources' element bound word (optional).
    ``w_packed``: the F16X3 pack ``conv2d_nhwc`` takes for the same filter.  ``want_stats=True`` returns ``(out, stats)`` with
    the moments of ``out`` in ``chan_stats`` layout.  Raises where ``small_conv_supported`` says no: there is no fallback."""
    L = hip_lib()
    B, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[-1]
    for t, c in ((src0, C0), (src1, C1), (res, Co)):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.shape == (B, H, W, c))
    if out is None:
        out = torch.empty((B, H, W, Co), device=src0.device, dtype=torch.float32)
    assert out.is_contiguous() and out.shape == (B, H, W, Co)
    ca, cs = coef if coef is not None else (None, None)
    assert ca is None or (ca.shape == (B, C0 + C1) and cs.shape == (B, C0 + C1) and ca.is_contiguous() and cs.is_contiguous())
    a = SmallConvArgs(src0=ptr(src0), src1=ptr(src1), C0=C0, C1=C1, coef_a=ptr(ca), coef_s=ptr(cs), act_in=act_in,
                      in_bound=_word(in_bound), w_packed=ptr(w_packed), arith=packed_arith(w_packed), bias=ptr(bias),
                      res=ptr(res), out_scale=float(out_scale), act_out=ACT_NONE, out=ptr(out), B=B, H=H, W=W, Co=Co, KH=3, KW=3,
                      variant=variant)
    plan = SmallConvPlan()
    _check(L.evc_small_conv_plan_query(ctypes.byref(a), ctypes.byref(plan)), "evc_small_conv_plan_query")
    stats = None
    if want_stats:
        stats = torch.empty((B, plan.stats_runs, Co, 2), device=src0.device, dtype=torch.float32)
        a.stats_out = ptr(stats)
    _check(L.evc_small_conv_f32(ctypes.byref(a), stream_ptr()), "evc_small_conv_f32")
    if SMALL_CONV_PROFILE is not None:
        SMALL_CONV_PROFILE.append(dict(kernel=plan.kernel.decode(), tile=(plan.tile_m, plan.tile_n), groups=plan.groups,
                                       shape=(B, H, W, C0 + C1, Co), C1=C1, coef=coef is not None, bound=in_bound is not None,
                                       res=res is not None, stats=bool(want_stats)))
    return (out, stats) if want_stats else out


def attention_set_option(name, value):
    """A/B switch of the attention kernels (include/evc_hip.h: "kv_planes", "f16_min_keys", "short_seq")."""
    if hip_lib(require_device=False).evc_attention_set_option(name.encode(), int(value)) != 0:
        raise EvcKernelError(f"unknown attention option {name!r}")


# Optional launch record (tests/attention_ledger.py): when a list is installed here ``attention`` appends the plan of the call
# it is about to make, with (B, heads, N, D, with_bounds, invariant).
ATTN_PROFILE = None


def attention_plan(B, heads, N, D, with_bounds=False, have_ws=None, invariant=False):
    """The whole plan of an attention launch without a launch (``evc_attention_plan_query``; works without a GPU): a dict of
    the kernel instance, waves per workgroup, key parts, tiles per part, the K / V pre-pass, the merge launch, LDS and
    workspace bytes.  ``have_ws=None``: as ``attention`` calls it, with a workspace exactly where the workspace size is not 0.
    Raises ``EvcKernelError`` with the launch's error code for arguments the launch refuses."""
    L = hip_lib(require_device=False)
    if have_ws is None:
        nbytes = (L.evc_attention_invariant_workspace_bytes if invariant else L.evc_attention_workspace_bytes)(B, heads, N, D)
        have_ws = nbytes > 0
    out = AttentionPlan()
    _check(L.evc_attention_plan_query(B, heads, N, D, int(bool(with_bounds)), int(bool(have_ws)), int(bool(invariant)),
                                      ctypes.byref(out)), "evc_attention_plan_query")
    return dict(kernel=out.kernel.decode(), waves=out.waves, kparts=out.kparts, tiles_per_part=out.tiles_per_part,
                kv_planes=bool(out.kv_planes), merge=bool(out.merge), short_seq=bool(out.short_seq),
                lds_bytes=out.lds_bytes, parts_bytes=out.parts_bytes, ws_bytes=out.ws_bytes)


def attention(qkv, C, heads, out=None, bounds=None, invariant=False, ws=None):
    """qkv: (B, N, 3C) with q | k | v concatenated along channels; returns (B, N, C).  ``bounds``: three int32 words
    (element bounds of q, k, v from ``moments_bound``) select the fp16-split kernel; None the f32-MFMA one.  ``out`` may be
    wider than C: its last dimension is the row stride, columns from C on are left alone.  ``ws``: a float32 workspace of at
    least the workspace bytes of the shape, instead of the shared one; False: ``evc_attention_f32``, the entry point without a
    workspace (f32 kernel, never a key split; default mode only)."""
    L = hip_lib()
    B, N, ld = qkv.shape
    D = C // heads
    inv = bool(invariant)
    if out is None:
        out = torch.empty((B, N, C), device=qkv.device, dtype=torch.float32)
    ld_out = out.shape[-1]
    assert out.is_contiguous() and tuple(out.shape[:2]) == (B, N) and ld_out >= C
    base = qkv.data_ptr()
    nbytes = (L.evc_attention_invariant_workspace_bytes if inv else L.evc_attention_workspace_bytes)(B, heads, N, D)
    if ws is None:
        ws = _workspace(nbytes, qkv.device) if nbytes > 0 else None      # stream-ordered: shared with the conv workspace
    elif ws is False:
        assert bounds is None and not inv
        ws = None
        nbytes = -1
    else:
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() * 4 >= nbytes
    if ATTN_PROFILE is not None:
        ATTN_PROFILE.append(dict(attention_plan(B, heads, N, D, bounds is not None, ws is not None, inv),
                                 call=(B, heads, N, D, bounds is not None, inv)))
    if inv:      # plan from (heads, N, D) only; bounds: (B, 3) words
        _check(L.evc_attention_invariant_f32(c_void_p(base), c_void_p(base + 4 * C), c_void_p(base + 8 * C), ld, fptr(out),
                                             ld_out, B, heads, N, D, float(int(D) ** (-0.5)),
                                             None if bounds is None else _word(bounds, 3 * B), ptr(ws), stream_ptr()),
               "evc_attention_invariant_f32")
        return out
    if bounds is not None:
        _check(L.evc_attention_f16x3_f32(c_void_p(base), c_void_p(base + 4 * C), c_void_p(base + 8 * C), ld, fptr(out), ld_out,
                                         B, heads, N, D, float(int(D) ** (-0.5)), _word(bounds, 3), ptr(ws), stream_ptr()),
               "evc_attention_f16x3_f32")
        return out
    if nbytes < 0:
        _check(L.evc_attention_f32(c_void_p(base), c_void_p(base + 4 * C), c_void_p(base + 8 * C), ld, fptr(out), ld_out, B,
                                   heads, N, D, float(int(D) ** (-0.5)), stream_ptr()), "evc_attention_f32")
        return out
    _check(L.evc_attention_ws_f32(c_void_p(base), c_void_p(base + 4 * C), c_void_p(base + 8 * C), ld, fptr(out), ld_out, B,
                                  heads, N, D, float(int(D) ** (-0.5)), ptr(ws), stream_ptr()), "evc_attention_ws_f32")
    return out


def frame_group_norm(x, N, gamma, beta, groups, eps):
    """GroupNorm over (C / groups channels x N frames) of each pixel, affine.  x: (B*N, H, W, C), a sample's frames adjacent."""
    BN, H, W, C = x.shape
    assert BN % N == 0 and x.is_contiguous()
    y = torch.empty_like(x)
    _check(hip_lib().evc_frame_group_norm_f32(fptr(x), fptr(y), fptr(gamma), fptr(beta), BN // N, N, H * W, C, groups,
                                              float(eps), stream_ptr()), "evc_frame_group_norm_f32")
    return y


def frame_attention(qkv, N, C, heads):
    """Attention over the N frames of each pixel.  qkv: (B*N, H, W, 3C) with q | k | v along channels; returns (B*N, H, W, C)."""
    BN, H, W, ld = qkv.shape
    assert BN % N == 0 and ld == 3 * C and qkv.is_contiguous()
    out = torch.empty((BN, H, W, C), device=qkv.device, dtype=torch.float32)
    _check(hip_lib().evc_frame_attention_f32(fptr(qkv), ld, fptr(out), C, BN // N, N, H * W, C, heads,
                                             float(int(C // heads) ** (-0.5)), stream_ptr()), "evc_frame_attention_f32")
    return out


def frame_mix(x, N, w, bias):
    """1x1 convolution over the frame axis: x (B*N, H, W, C), w (M, N) -> (B*M, H, W, C)."""
    BN, H, W, C = x.shape
    M = w.shape[0]
    assert BN % N == 0 and tuple(w.shape) == (M, N) and x.is_contiguous() and w.is_contiguous()
    B = BN // N
    y = torch.empty((B * M, H, W, C), device=x.device, dtype=torch.float32)
    _check(hip_lib().evc_frame_mix_f32(fptr(x), fptr(y), fptr(w), fptr(bias), B, N, M, H * W * C, stream_ptr()),
           "evc_frame_mix_f32")
    return y


def frame_taps(x, N):
    """Frames n - 1 | n | n + 1 side by side along the channels (zeros beyond a sample's frames): (B*N, H, W, C) -> (B*N, H, W, 3C)."""
    BN, H, W, C = x.shape
    assert BN % N == 0 and x.is_contiguous()
    y = torch.empty((BN, H, W, 3 * C), device=x.device, dtype=torch.float32)
    _check(hip_lib().evc_frame_taps_f32(fptr(x), fptr(y), BN // N, N, H * W, C, stream_ptr()), "evc_frame_taps_f32")
    return y


class Deconv5x5s2:
    """compressai ``deconv`` (ConvTranspose2d k 5, stride 2, padding 2, output_padding 1) in polyphase form
    (include/evc_hip.h, csrc/stride2.hip).  ``weight``: the module's (Ci, Co, 5, 5) tensor, ``bias``: (Co,)."""

    def __init__(self, weight, bias, arith=None, device="cuda"):
        Lh = hip_lib()
        w = weight.detach().to(device, torch.float32).contiguous()
        self.Ci, self.Co = w.shape[0], w.shape[1]
        self.Cp, self.CiPad = (self.Co + 15) // 16 * 16, (self.Ci + 15) // 16 * 16
        wp = torch.empty((4 * self.Cp, self.CiPad, 3, 3), device=device, dtype=torch.float32)
        _check(Lh.evc_deconv5x5s2_phase_weights_f32(fptr(w), fptr(wp), self.Ci, self.Co, self.Cp, self.CiPad, stream_ptr()),
               "evc_deconv5x5s2_phase_weights_f32")
        self.arith = default_arith() if arith is None else arith
        self.w = conv_pack_weights(wp, self.arith)
        b4 = torch.zeros((4, self.Cp), device=device, dtype=torch.float32)
        b4[:, :self.Co] = bias.detach().to(device, torch.float32)[None, :]
        self.bias4 = b4.reshape(-1).contiguous()

    def __call__(self, x, act_out=ACT_NONE):
        B, H, W, C = x.shape
        assert C == self.CiPad and x.dtype == torch.float32 and x.is_contiguous()
        Lh = hip_lib()
        ws = _workspace(Lh.evc_deconv5x5s2_workspace_bytes(B, H, W, self.Cp), x.device)
        out = torch.empty((B, 2 * H, 2 * W, self.Co), device=x.device, dtype=torch.float32)
        _check(Lh.evc_deconv5x5s2_f32(fptr(x), ptr(self.w), self.arith, fptr(self.bias4), fptr(out), ptr(ws), B, H, W, C,
                                      self.Co, act_out, stream_ptr()), "evc_deconv5x5s2_f32")
        return out


class Conv5x5s2:
    """compressai ``conv`` (Conv2d k 5, stride 2, padding 2) in polyphase form.  ``weight``: (Co, Ci, 5, 5)."""

    def __init__(self, weight, bias, arith=None, device="cuda"):
        Lh = hip_lib()
        w = weight.detach().to(device, torch.float32).contiguous()
        self.Co, self.Ci = w.shape[0], w.shape[1]
        self.Cq = (self.Ci + 3) // 4 * 4
        wq = torch.empty((self.Co, 4 * self.Cq, 3, 3), device=device, dtype=torch.float32)
        _check(Lh.evc_conv5x5s2_phase_weights_f32(fptr(w), fptr(wq), self.Co, self.Ci, self.Cq, stream_ptr()),
               "evc_conv5x5s2_phase_weights_f32")
        self.arith = default_arith() if arith is None else arith
        self.w = conv_pack_weights(wq, self.arith)
        self.bias = bias.detach().to(device, torch.float32).contiguous()

    def __call__(self, x, act_out=ACT_NONE, channels=None):
        """x: (B, 2Ho, 2Wo, ld) of which the first ``channels`` (default all) are the input."""
        B, H2, W2, ld = x.shape
        C = ld if channels is None else channels
        assert C == self.Ci and ld >= C and H2 % 2 == 0 and W2 % 2 == 0 and x.is_contiguous()
        Lh = hip_lib()
        ws = _workspace(Lh.evc_conv5x5s2_workspace_bytes(B, H2 // 2, W2 // 2, C), x.device)
        out = torch.empty((B, H2 // 2, W2 // 2, self.Co), device=x.device, dtype=torch.float32)
        _check(Lh.evc_conv5x5s2_f32(fptr(x), ld, ptr(self.w), self.arith, fptr(self.bias), fptr(out), ptr(ws), B, H2 // 2,
                                    W2 // 2, C, self.Co, act_out, stream_ptr()), "evc_conv5x5s2_f32")
        return out


class GDN:
    """GDN / IGDN / GDN1 (reference ELICUtilis/layers/gdn.py:26-106) on NHWC tensors.  ``beta`` (C,) and ``gamma`` (C, C)
    are the RAW parameters of the reference module; compressai's NonNegativeParametrizer is applied here, once:
    ``max(p, sqrt(minimum + 2^-36))^2 - 2^-36`` (minimum = beta_min for beta, 0 for gamma)."""
    PEDESTAL = (2.0 ** -18) ** 2

    def __init__(self, beta, gamma, inverse=False, simplified=False, beta_min=1e-6, device="cuda"):
        hip_lib()
        b = beta.detach().to(device, torch.float32)
        g = gamma.detach().to(device, torch.float32)
        self.C = b.numel()
        self.beta = (torch.clamp(b, min=(beta_min + self.PEDESTAL) ** 0.5) ** 2 - self.PEDESTAL).contiguous()
        gm = torch.clamp(g, min=self.PEDESTAL ** 0.5) ** 2 - self.PEDESTAL
        self.arith = default_arith()
        self.gamma = conv_pack_weights(gm.reshape(self.C, self.C, 1, 1).contiguous(), self.arith)
        self.inverse, self.simplified = bool(inverse), bool(simplified)

    def __call__(self, x, out=None):
        B, H, W, C = x.shape
        assert C == self.C and x.dtype == torch.float32
        Lh = hip_lib()
        nbytes = Lh.evc_gdn_workspace_bytes(B, H, W, C)
        if nbytes < 0:
            raise EvcKernelError(f"evc_gdn_workspace_bytes rejected the arguments ({nbytes})")
        ws = _workspace(nbytes, x.device)
        if out is None:
            out = torch.empty_like(x)
        _check(Lh.evc_gdn_f32(fptr(x), ptr(self.gamma), self.arith, fptr(self.beta), fptr(out), ptr(ws), B, H, W, C,
                              int(self.inverse), int(self.simplified), stream_ptr()), "evc_gdn_f32")
        return out


def ddpm_step(x, e, noise, k1, k2, c1, c2, sigma, clip):
    _check(hip_lib().evc_ddpm_step_f32(fptr(x), fptr(e), fptr(noise), x.numel(), k1, k2, c1, c2, sigma, int(clip),
                                       stream_ptr()), "evc_ddpm_step_f32")


def ddim_step(x, e, k1, k2, c1, c2, clip):
    _check(hip_lib().evc_ddim_step_f32(fptr(x), fptr(e), x.numel(), k1, k2, c1, c2, int(clip), stream_ptr()),
           "evc_ddim_step_f32")


def axpy(x, e, alpha, out=None):
    if out is None:
        out = torch.empty_like(x)
    _check(hip_lib().evc_axpy_f32(fptr(x), fptr(e), fptr(out), x.numel(), alpha, stream_ptr()), "evc_axpy_f32")
    return out


def pndm_transfer(x, e, d, cx, ce, clip, out=None):
    if out is None:
        out = torch.empty_like(x)
    _check(hip_lib().evc_pndm_transfer_f32(fptr(x), fptr(e), fptr(out), x.numel(), d, cx, ce, int(clip),
                                           stream_ptr()), "evc_pndm_transfer_f32")
    return out


def lincomb4(es, ws, out=None):
    es = list(es) + [None] * (4 - len(es))
    ws = list(ws) + [0.0] * (4 - len(ws))
    if out is None:
        out = torch.empty_like(es[0])
    _check(hip_lib().evc_lincomb4_f32(fptr(es[0]), fptr(es[1]), fptr(es[2]), fptr(es[3]), fptr(out), out.numel(),
                                      *[float(w) for w in ws], stream_ptr()), "evc_lincomb4_f32")
    return out


def scale_clamp(x, mul, add, clamp=None, out=None):
    if out is None:
        out = torch.empty_like(x)
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    _check(hip_lib().evc_scale_clamp_f32(fptr(x), fptr(out), x.numel(), mul, add, int(clamp is not None), lo, hi,
                                         stream_ptr()), "evc_scale_clamp_f32")
    return out


def noise_keys(pairs, device):
    """[(stream id, start frame)] -> the device key array [B][2] of ``noise_normal`` (uint32 bits in an int32 tensor)."""
    k = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert k.size and k.min() >= 0 and k.max() < 2 ** 32, "stream ids and start frames are u32"
    return torch.from_numpy(k.astype(np.uint32).view(np.int32)).to(device).contiguous()


def noise_normal(keys, shape, seed, step, raw=False, out=None):
    """Noise specification N1 (include/evc_hip.h evc_noise_normal_f32): standard normals (``raw``: the Philox words, int32) of
    sampler step tag ``step`` for a batch, sample b from the stream of keys[b] = (stream id, start frame).  shape: (B, ...)."""
    B = int(shape[0])
    n = int(np.prod(shape[1:]))
    assert keys.dtype == torch.int32 and tuple(keys.shape) == (B, 2)
    if out is None:
        out = torch.empty(tuple(shape), device=keys.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.numel() == B * n
    _check(hip_lib().evc_noise_normal_f32(fptr(out), ptr(keys), B, n, int(seed) & (2 ** 64 - 1), int(step), int(bool(raw)),
                                          stream_ptr()), "evc_noise_normal_f32")
    return out.view(torch.int32) if raw else out


# ---- YUV 4:2:0 <-> RGB (include/evc_hip.h evc_yuv420_to_rgb / evc_rgb_to_yuv420) ------------------------------------
YUV_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}


def yuv420_frame_bytes(H, W, bits=8):
    """Bytes of one planar 4:2:0 frame: Y, then U, then V."""
    return H * W * (2 if bits > 8 else 1) * 3 // 2


def _yuv_layout(H, W, bits, first, stride, offsets):
    luma = H * W * (2 if bits > 8 else 1)
    off = (0, luma, luma + luma // 4) if offsets is None else tuple(int(o) for o in offsets)
    return int(first), int(luma * 3 // 2 if stride is None else stride), off


def yuv420_to_rgb(buf, N, H, W, bits=8, mode="bicubic", first=0, stride=None, offsets=None, dtype=torch.float32, out=None):
    """buf: 1-D uint8 device tensor holding N planar 4:2:0 frames, frame n at byte ``first + n * stride`` (default: packed),
    its planes at ``offsets`` = (Y, U, V) from there (default: Y, U, V back to back) -> (N, 3, H, W) RGB, float32 unclamped or
    uint8 = rint(clamp(rgb * 255))."""
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and dtype in (torch.float32, torch.uint8)
    first, stride, off = _yuv_layout(H, W, bits, first, stride, offsets)
    if out is None:
        out = torch.empty((N, 3, H, W), device=buf.device, dtype=dtype)
    assert out.dtype == dtype and tuple(out.shape) == (N, 3, H, W)
    _check(hip_lib().evc_yuv420_to_rgb(ptr(buf), buf.numel(), first, stride, off[0], off[1], off[2], N, H, W, bits,
                                       YUV_MODES[mode], ptr(out), int(dtype == torch.uint8), stream_ptr()), "evc_yuv420_to_rgb")
    return out


def rgb_to_yuv420(x, events, bits=8, buf=None, first=0, stride=None, offsets=None):
    """x: (N, 3, H, W) float32 in [0, 1] -> the 1-D uint8 device tensor of its planar 4:2:0 samples (``buf``, ``first``,
    ``stride``, ``offsets`` as in ``yuv420_to_rgb``; default: a new packed buffer).  events: int32 device word (1 element); a
    non-finite pixel writes 0 and ORs RANGE_NONFINITE into it."""
    assert x.dim() == 4 and x.shape[1] == 3 and events.dtype == torch.int32 and events.numel() == 1
    N, _, H, W = x.shape
    first, stride, off = _yuv_layout(H, W, bits, first, stride, offsets)
    if buf is None:
        buf = torch.empty(first + N * stride, device=x.device, dtype=torch.uint8)
    assert buf.dtype == torch.uint8 and buf.dim() == 1
    _check(hip_lib().evc_rgb_to_yuv420(fptr(x.contiguous()), ptr(buf), buf.numel(), first, stride, off[0], off[1], off[2], N, H, W,
                                       bits, ptr(events), stream_ptr()), "evc_rgb_to_yuv420")
    return buf


# ---- Pillow's 8-bit resize (include/evc_hip.h evc_resample_h_u8 / evc_resample_v_u8) ----------
def _sinc(v):
    return 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)


def _bicubic_filter(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    return (((x - 5) * x + 8) * x - 4) * a if x < 2.0 else 0.0


def _hamming_filter(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    return math.sin(math.pi * x) / (math.pi * x) * (0.54 + 0.46 * math.cos(math.pi * x)) if x < 1.0 else 0.0


# name -> (filter, support): Pillow's resampling filters
RESAMPLE_FILTERS = {
    "lanczos": (lambda x: _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0, 3.0),
    "bicubic": (_bicubic_filter, 2.0),
    "bilinear": (lambda x: 1.0 - abs(x) if abs(x) < 1.0 else 0.0, 1.0),
    "hamming": (_hamming_filter, 1.0),
    "box": (lambda x: 1.0 if -0.5 < x <= 0.5 else 0.0, 0.5),
}
RESAMPLE_PRECISION = 22          # 32 - 8 - 2 bits of coefficient


def resample_tables(n_in, n_out, filter="lanczos"):
    """The tables of one axis of Pillow's 8-bit resize from ``n_in`` to ``n_out`` samples -> (bounds (n_out, 2) int32: first
    source index and tap count, coeffs (n_out, ksize) int32: the taps in units of 2^-22, zero past the count, ksize).  Every
    step is in Python floats in Pillow's order of operations.  ``filter``: a name of
    ``RESAMPLE_FILTERS`` or a (function, support) pair.  Refuses (ValueError) a table with which an output's sum of products
    with 8-bit samples could leave int32, the width the kernels accumulate in."""
    fn, fsupport = RESAMPLE_FILTERS[filter] if isinstance(filter, str) else filter
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resample_tables: sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fsupport * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coeffs = np.zeros((n_out, ksize), dtype=np.int64)
    one = float(1 << RESAMPLE_PRECISION)
    for xx in range(n_out):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), n_in) - xmin
        w = [fn((x + xmin - c + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            if ww != 0.0:
                v /= ww
            coeffs[xx, x] = int(v * one + 0.5) if v >= 0 else int(v * one - 0.5)
    worst = 255 * int(np.abs(coeffs).sum(1).max()) + (1 << (RESAMPLE_PRECISION - 1))
    if worst > 2 ** 31 - 1:
        raise ValueError(f"resample_tables: with this filter a sum of {n_in} -> {n_out} can reach {worst}, beyond int32: refused")
    return bounds, coeffs.astype(np.int32), ksize


_resample_tables = {}      # (n_in, n_out, filter, device) -> (bounds, coeffs, ksize), the arrays on the device


def _resample_device_tables(n_in, n_out, filter, device):
    key = (n_in, n_out, filter, str(device))
    if key not in _resample_tables:
        b, k, ksize = resample_tables(n_in, n_out, filter)
        _resample_tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), ksize)
    return _resample_tables[key]


def resample_u8(x, out_h, out_w, filter="lanczos", box=None):
    """PIL.Image.resize((out_w, out_h), filter) of every frame of x, (N, 3, H, W) uint8 on the device -> (N, 3, out_h, out_w)
    uint8, bit for bit (8 bits per channel: integer arithmetic).  ``box`` = (r0, c0, h, w): the part of
    each frame that is the image (default: all of it); the passes read it where it lies.  The horizontal pass runs first, the
    vertical pass on its uint8 result; a pass whose size does not change is skipped, and with both skipped the result is a
    copy of the box.  ``filter``: a name of ``RESAMPLE_FILTERS``; tables are cached per (size in, size out, filter)."""
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.is_cuda and x.is_contiguous(), "device-contiguous (N, C, H, W) uint8 required"
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"resample_u8: filter {filter!r} is not one of {', '.join(RESAMPLE_FILTERS)}")
    N, C, H, W = x.shape
    r0, c0, h, w = (0, 0, H, W) if box is None else (int(v) for v in box)
    if not (0 <= r0 and 0 <= c0 and h >= 1 and w >= 1 and r0 + h <= H and c0 + w <= W and out_h >= 1 and out_w >= 1):
        raise ValueError(f"resample_u8: box {(r0, c0, h, w)} -> {out_h}x{out_w} does not fit {H}x{W} frames")
    planes = N * C
    if planes == 0 or (out_w == w and out_h == h):
        return x[:, :, r0:r0 + h, c0:c0 + w].contiguous()
    src, rows, row_stride, plane_stride = x.data_ptr() + r0 * W + c0, h, W, H * W
    if out_w != w:
        b, k, ksize = _resample_device_tables(w, out_w, filter, x.device)
        mid = torch.empty((N, C, h, out_w), dtype=torch.uint8, device=x.device)
        _check(hip_lib().evc_resample_h_u8(c_void_p(src), planes, h, w, plane_stride, row_stride, ptr(b), ptr(k), ksize, out_w,
                                           ptr(mid), stream_ptr()), "evc_resample_h_u8")
        if out_h == h:
            return mid
        src, row_stride, plane_stride = mid.data_ptr(), out_w, h * out_w
    b, k, ksize = _resample_device_tables(h, out_h, filter, x.device)
    out = torch.empty((N, C, out_h, out_w), dtype=torch.uint8, device=x.device)
    _check(hip_lib().evc_resample_v_u8(c_void_p(src), planes, rows, out_w, plane_stride, row_stride, ptr(b), ptr(k), ksize, out_h,
                                       ptr(out), stream_ptr()), "evc_resample_v_u8")
    return out


# ---- whole frames as overlapping tiles (include/evc_hip.h evc_tile_gather_u8 / evc_tile_blend_f32) ----
_tile_origins = {}         # (oy, ox, device) -> (oy, ox host int32 arrays, the same two on the device)


def _tile_grid(N, H, W, S, oy, ox, device, cover, name):
    """The origin arrays of one grid on the host and on the device (cached per grid), after the library's own check of them
    against (N, H, W, S) -- made before anything is sized by S."""
    oy, ox = tuple(int(v) for v in oy), tuple(int(v) for v in ox)
    hy, hx = np.asarray(oy, dtype=np.int32), np.asarray(ox, dtype=np.int32)
    _check(hip_lib().evc_tile_grid_check(N, H, W, S, len(oy), len(ox), c_void_p(hy.ctypes.data), c_void_p(hx.ctypes.data), int(cover)),
           name)
    key = (oy, ox, str(device))
    if key not in _tile_origins:
        _tile_origins[key] = (hy, hx, torch.from_numpy(hy).to(device), torch.from_numpy(hx).to(device))
    return _tile_origins[key]


def tile_gather_u8(x, S, oy, ox):
    """x: (N, 3, H, W) uint8 on the device -> (ny * nx, N, 3, S, S) uint8: tile ty * nx + tx is rows oy[ty] .. oy[ty] + S - 1 and
    columns ox[tx] .. ox[tx] + S - 1 of every frame, a copy; past the end of an axis shorter than S its last sample repeats.
    oy, ox: the origins of ``video_io.tile_grid``, strictly increasing inside [0, max(L - S, 0)] (else ``EvcKernelError``)."""
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[1] == 3 and x.is_cuda and x.is_contiguous(), \
        "device-contiguous (N, 3, H, W) uint8 required"
    N, _, H, W = x.shape
    hy, hx, dy, dx = _tile_grid(N, H, W, int(S), oy, ox, x.device, False, "evc_tile_gather_u8")
    out = torch.empty((len(hy) * len(hx), N, 3, S, S), dtype=torch.uint8, device=x.device)
    _check(hip_lib().evc_tile_gather_u8(ptr(x), N, H, W, S, len(hy), len(hx), c_void_p(hy.ctypes.data), c_void_p(hx.ctypes.data),
                                        ptr(dy), ptr(dx), ptr(out), stream_ptr()), "evc_tile_gather_u8")
    return out


def tile_blend(tiles, H, W, oy, ox):
    """tiles: (ny * nx, N, 3, S, S) float32 on the device, laid out as ``tile_gather_u8`` gives them -> (N, 3, H, W) float32:
    every pixel is the mean of the tiles that cover it under the weights t(ly) * t(lx), t(i) = min(i + 1, S - i), added in
    ascending tile index in fp32 and divided by their integer sum (bit for bit tests/tile_ref.py).  The origins must cover
    every pixel (first 0, last max(L - S, 0), steps of at most S), else ``EvcKernelError``."""
    assert tiles.dtype == torch.float32 and tiles.dim() == 5 and tiles.shape[2] == 3 and tiles.shape[3] == tiles.shape[4] and \
        tiles.is_cuda and tiles.is_contiguous(), "device-contiguous (tiles, N, 3, S, S) float32 required"
    T, N, _, S, _ = tiles.shape
    assert T == len(oy) * len(ox), f"{T} tiles for a {len(oy)} x {len(ox)} grid"
    hy, hx, dy, dx = _tile_grid(N, int(H), int(W), S, oy, ox, tiles.device, True, "evc_tile_blend_f32")
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=tiles.device)
    _check(hip_lib().evc_tile_blend_f32(ptr(tiles), N, H, W, S, len(hy), len(hx), c_void_p(hy.ctypes.data), c_void_p(hx.ctypes.data),
                                        ptr(dy), ptr(dx), ptr(out), stream_ptr()), "evc_tile_blend_f32")
    return out


def tile_gather_f32(x, S, oy, ox):
    """x: (N, C, H, W) float32 on the device, any C -> (ny * nx, N, C, S, S) float32: ``tile_gather_u8`` for float planes, the
    layout ``tests/tile_ref.py::gather`` defines.  A copy: NaN / inf pass through, nothing is clamped."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_cuda and x.is_contiguous(), \
        "device-contiguous (N, C, H, W) float32 required"
    N, C, H, W = x.shape
    hy, hx, dy, dx = _tile_grid(N, H, W, int(S), oy, ox, x.device, False, "evc_tile_gather_f32")
    out = torch.empty((len(hy) * len(hx), N, C, S, S), dtype=torch.float32, device=x.device)
    _check(hip_lib().evc_tile_gather_f32(ptr(x), N, C, H, W, S, len(hy), len(hx), c_void_p(hy.ctypes.data), c_void_p(hx.ctypes.data),
                                         ptr(dy), ptr(dx), ptr(out), stream_ptr()), "evc_tile_gather_f32")
    return out


def tile_blend_planes(tiles, H, W, oy, ox):
    """tiles: (ny * nx, N, C, S, S) float32 with C a multiple of 3 -> (N, C, H, W) float32: ``tile_blend`` of the same memory
    seen as (ny * nx, N * C / 3, 3, S, S) -- every plane is blended on its own, so the view changes no bit."""
    if tiles.dim() != 5 or tiles.shape[2] % 3:
        raise NotImplementedError(f"tile_blend_planes: tiles of shape {tuple(tiles.shape)}: (tiles, N, C, S, S) with C a multiple of 3 "
                                  "is built (evc_tile_blend_f32 takes planes in threes)")
    T, N, C, S, _ = tiles.shape
    return tile_blend(tiles.view(T, N * C // 3, 3, S, S), H, W, oy, ox).view(N, C, int(H), int(W))


def gate_residual(a, b, x, out=None):
    if out is None:
        out = torch.empty_like(x)
    _check(hip_lib().evc_gate_residual_f32(fptr(a), fptr(b), fptr(x), fptr(out), x.numel(), stream_ptr()),
           "evc_gate_residual_f32")
    return out


def elic_gather_params(ms, mean_off, scale_off, C, parity, scale_table):
    """ms: (B, H, W, ld) -> (idx int32 (B, C, H, W/2), means float32 (B, C, H, W/2))."""
    B, H, W, ld = ms.shape
    idx = torch.empty((B, C, H, W // 2), device=ms.device, dtype=torch.int32)
    means = torch.empty((B, C, H, W // 2), device=ms.device, dtype=torch.float32)
    _check(hip_lib().evc_elic_gather_params_f32(fptr(ms), ld, mean_off, scale_off, C, B, H, W, parity,
                                                fptr(scale_table), scale_table.numel(), fptr(idx, torch.int32),
                                                fptr(means), stream_ptr()), "evc_elic_gather_params_f32")
    return idx, means


def elic_scatter_symbols(symbols, means, y_hat, c0, parity):
    B, C, H, Wh = symbols.shape
    _check(hip_lib().evc_elic_scatter_symbols_f32(fptr(symbols, torch.int32), fptr(means), fptr(y_hat),
                                                  y_hat.shape[-1], c0, C, B, H, 2 * Wh, parity, stream_ptr()),
           "evc_elic_scatter_symbols_f32")


def elic_quantize(y, c0, means, parity):
    """y: (B, H, W, ld); means: (B, C, H, W/2) -> int32 symbols (B, C, H, W/2)."""
    B, C, H, Wh = means.shape
    sym = torch.empty((B, C, H, Wh), device=y.device, dtype=torch.int32)
    _check(hip_lib().evc_elic_quantize_f32(fptr(y), y.shape[-1], c0, fptr(means), C, B, H, 2 * Wh, parity,
                                           fptr(sym, torch.int32), stream_ptr()), "evc_elic_quantize_f32")
    return sym


def elic_rate_pass(ms, mean_off, scale_off, C, y, c0, parity, y_hat, bits=None):
    """One (slice, parity) pass of the rate estimate: ms (B, H, W, ld), y / y_hat (B, H, W, ld_y); fills y_hat at the pass's
    checkerboard sites of channels c0 .. c0+C and returns bits (B,) float64 on the device (``bits``: where to write them)."""
    B, H, W, ld = ms.shape
    assert y.shape == y_hat.shape and y.shape[:3] == ms.shape[:3]
    if bits is None:
        bits = torch.empty((B,), device=ms.device, dtype=torch.float64)
    assert bits.shape == (B,)
    _check(hip_lib().evc_elic_rate_pass_f32(fptr(ms), ld, mean_off, scale_off, C, fptr(y), y.shape[-1], c0, B, H, W, parity,
                                            fptr(y_hat), fptr(bits, torch.float64), stream_ptr()), "evc_elic_rate_pass_f32")
    return bits


def bottleneck_rate(z, C, medians, density, bits=None, out=None):
    """z: (B, H, W, ld) -> (z_hat (B, H, W, ld) with channels < C written, bits (B,) float64 on the device); medians (C,),
    density (C, 58) as ``entropy.pack_density`` lays it out.  ``out``: the tensor to write z_hat into."""
    B, H, W, ld = z.shape
    assert medians.shape == (C,) and density.shape == (C, 58)
    z_hat = out if out is not None else (torch.zeros_like(z) if ld > C else torch.empty_like(z))
    assert z_hat.shape == z.shape
    if bits is None:
        bits = torch.empty((B,), device=z.device, dtype=torch.float64)
    assert bits.shape == (B,)
    _check(hip_lib().evc_bottleneck_rate_f32(fptr(z), ld, C, B, H, W, fptr(medians), fptr(density), fptr(z_hat),
                                             fptr(bits, torch.float64), stream_ptr()), "evc_bottleneck_rate_f32")
    return z_hat, bits


def ssim_planes(a, b, taps, c1, c2, out=None):
    """a, b: (N, H, W) float32 planes in [0, 1]; taps: the 11 window taps, float64 on the device -> out (N,) float64 on the
    device: the mean of each plane's SSIM map (include/evc_hip.h evc_ssim_planes_f32)."""
    L = hip_lib()
    N, H, W = a.shape
    assert b.shape == a.shape and taps.shape == (11,)
    if out is None:
        out = torch.empty((N,), device=a.device, dtype=torch.float64)
    assert out.shape == (N,)
    nbytes = L.evc_ssim_workspace_bytes(N, H, W)
    if nbytes < 0:
        raise EvcKernelError(f"evc_ssim_workspace_bytes rejected the arguments ({nbytes})")
    ws = torch.empty((max(1, nbytes // 8),), device=a.device, dtype=torch.float64)
    _check(L.evc_ssim_planes_f32(fptr(a), fptr(b), N, H, W, fptr(taps, torch.float64), float(c1), float(c2),
                                 fptr(out, torch.float64), ptr(ws), stream_ptr()), "evc_ssim_planes_f32")
    return out


def msssim_levels(a, b, levels, taps, c1, c2, out=None):
    """a, b: (N, H, W) float32 planes in [0, 1]; taps: the 11 window taps, float64 on the device -> out (N, levels, 2) float64
    on the device: per level the means of the SSIM map and of its cs factor (include/evc_hip.h evc_msssim_levels_f32)."""
    L = hip_lib()
    N, H, W = a.shape
    assert b.shape == a.shape and taps.shape == (11,)
    nbytes = L.evc_msssim_workspace_bytes(N, H, W, levels)
    if nbytes < 0:
        raise EvcKernelError(f"evc_msssim_workspace_bytes rejected the arguments ({nbytes})")
    if out is None:
        out = torch.empty((N, levels, 2), device=a.device, dtype=torch.float64)
    assert out.shape == (N, levels, 2)
    ws = torch.empty((max(1, nbytes // 8),), device=a.device, dtype=torch.float64)
    _check(L.evc_msssim_levels_f32(fptr(a), fptr(b), N, H, W, levels, fptr(taps, torch.float64), float(c1), float(c2),
                                   fptr(out, torch.float64), ptr(ws), stream_ptr()), "evc_msssim_levels_f32")
    return out


def frame_sqerr(a, b, out=None):
    """a, b: (n, ...) float32 frames on the device, contiguous -> out (n,) float64 on the device: per frame the sum of
    ((double)a - (double)b)^2 (include/evc_hip.h evc_frame_sqerr_f64); a frame's value does not depend on the launch."""
    n = int(a.shape[0])
    assert a.dim() >= 1 and a.shape == b.shape and n > 0 and a.numel() > 0
    if out is None:
        out = torch.empty((n,), device=a.device, dtype=torch.float64)
    assert out.shape == (n,)
    _check(hip_lib().evc_frame_sqerr_f64(fptr(a), fptr(b), n, a.numel() // n, fptr(out, torch.float64), stream_ptr()),
           "evc_frame_sqerr_f64")
    return out


# ---- host rANS -------------------------------------------------------------------------------

def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def rans_encode(symbols, indexes, cdfs, cdf_sizes, offsets):
    """-> bytes.  Arguments are int arrays; ``cdfs`` is (n_cdfs, ld)."""
    L = rans_lib()
    s, i, c, z, o = _i32(symbols).ravel(), _i32(indexes).ravel(), _i32(cdfs), _i32(cdf_sizes).ravel(), _i32(offsets).ravel()
    cap = L.evc_rans_max_encoded_bytes(s.size)
    out = np.empty(cap, dtype=np.uint8)
    P32, P8 = POINTER(c_int32), POINTER(c_uint8)
    n = L.evc_rans_encode_with_indexes(s.ctypes.data_as(P32), i.ctypes.data_as(P32), s.size, c.ctypes.data_as(P32),
                                       c.shape[1], z.ctypes.data_as(P32), o.ctypes.data_as(P32), c.shape[0],
                                       out.ctypes.data_as(P8), cap)
    if n < 0:
        raise EvcKernelError(f"evc_rans_encode_with_indexes failed ({n})")
    return out[:n].tobytes()


def rans_decode(data, indexes, cdfs, cdf_sizes, offsets):
    """-> int32 array of len(indexes) symbols."""
    L = rans_lib()
    buf = np.frombuffer(data, dtype=np.uint8)
    i, c, z, o = _i32(indexes).ravel(), _i32(cdfs), _i32(cdf_sizes).ravel(), _i32(offsets).ravel()
    out = np.empty(i.size, dtype=np.int32)
    P32, P8 = POINTER(c_int32), POINTER(c_uint8)
    rc = L.evc_rans_decode_with_indexes(buf.ctypes.data_as(P8), buf.size, i.ctypes.data_as(P32), i.size,
                                        c.ctypes.data_as(P32), c.shape[1], z.ctypes.data_as(P32),
                                        o.ctypes.data_as(P32), c.shape[0], out.ctypes.data_as(P32))
    if rc != 0:
        raise EvcKernelError(f"evc_rans_decode_with_indexes failed ({rc})")
    return out


def pmf_to_quantized_cdf(pmf, precision=16):
    L = rans_lib()
    p = np.ascontiguousarray(pmf, dtype=np.float32)
    out = np.empty(p.size + 1, dtype=np.int32)
    rc = L.evc_pmf_to_quantized_cdf(p.ctypes.data_as(POINTER(c_float)), p.size, precision,
                                    out.ctypes.data_as(POINTER(c_int32)))
    if rc != 0:
        raise EvcKernelError(f"evc_pmf_to_quantized_cdf failed ({rc})")
    return out

"""ctypes binding of libnoisediff_hip.so (the C ABI in include/noisediff_hip.h).

No fallback: ``load()`` raises if the library is missing (build it with
``python -m noisediff_amd.build`` / ``__graft_entry__.build()``), and every call is
checked -- a non-zero return raises ``HipError`` with the library's message.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnoisediff_hip.so")

# enum nd_prologue / nd_act
PRO_NONE, PRO_AFFINE_SILU, PRO_AFFINE_MAP_SILU, PRO_LAYERNORM, PRO_SILU, PRO_LEAKY, PRO_LEAKY_SECOND, PRO_AFFINE_GENMAP_SILU = 0, 1, 2, 3, 4, 5, 6, 7
ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2
OBJECTIVES = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1                           # enum nd_layout
CONV3X3_DIRECT, CONV3X3_WINO, CONV3X3_WINO2, CONV3X3_WINO4, CONV3X3_WINO4_16 = 0, 1, 2, 3, 4      # enum nd_conv3x3_kernel

fptr = C.c_void_p   # device pointers travel as integers


class HipError(RuntimeError):
    pass


class Src(C.Structure):
    _fields_ = [("p0", fptr), ("p1", fptr), ("c0", C.c_int32), ("c1", C.c_int32), ("ld0", C.c_int32), ("ld1", C.c_int32),
                ("mode", C.c_int32), ("upsample", C.c_int32), ("unshuffle", C.c_int32), ("map_blocked", C.c_int32),
                ("mad", fptr), ("map", fptr), ("vec", fptr), ("gamma", fptr), ("beta", fptr), ("rowstats", fptr)]


class AdamItem(C.Structure):
    _fields_ = [("p", fptr), ("g", fptr), ("m", fptr), ("v", fptr), ("n", C.c_int64), ("step_size", C.c_float), ("bias2_sqrt", C.c_float),
                ("vec4", C.c_int32), ("reserved", C.c_int32), ("step", fptr)]


class EmaItem(C.Structure):
    _fields_ = [("ema", fptr), ("src", fptr), ("n", C.c_int64), ("vec4", C.c_int32), ("no_ema", C.c_int32)]


class PackItem(C.Structure):
    _fields_ = [("w", fptr), ("packed", fptr), ("cin", C.c_int32), ("cout", C.c_int32), ("transposed", C.c_int32), ("reserved", C.c_int32)]


class Conv3x3(C.Structure):
    _fields_ = [("src", Src), ("weight", fptr), ("bias", fptr), ("out", fptr), ("stats", fptr), ("slot_count", fptr),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("ldo", C.c_int32)]


class Pointwise(C.Structure):
    _fields_ = [("src", Src), ("weight", fptr), ("bias", fptr), ("out", fptr), ("res0", fptr), ("res1", fptr), ("vec", fptr),
                ("gn_t", fptr), ("gn_mad", fptr), ("B", C.c_int32), ("HW", C.c_int32), ("W", C.c_int32), ("cin", C.c_int32),
                ("cout", C.c_int32), ("ldo", C.c_int32), ("ldr0", C.c_int32), ("ldr1", C.c_int32), ("ldt", C.c_int32), ("act", C.c_int32),
                ("shuffle_c", C.c_int32), ("shuffle_h", C.c_int32), ("shuffle_w", C.c_int32)]


class ChainStage(C.Structure):
    _fields_ = [("weight", fptr), ("bias", fptr), ("cin", C.c_int32), ("cout", C.c_int32), ("act", C.c_int32), ("res", C.c_int32)]


class Chain(C.Structure):
    _fields_ = [("src", Src), ("st", ChainStage * 3), ("out", fptr), ("n_stages", C.c_int32), ("B", C.c_int32), ("HW", C.c_int32),
                ("ldo", C.c_int32)]


class ChainTail(C.Structure):
    _fields_ = [("chain", Chain), ("mad", fptr), ("r0", fptr), ("r1", fptr), ("ldr0", C.c_int32), ("ldr1", C.c_int32)]


class NarrowFold(C.Structure):
    _fields_ = [("p0", fptr), ("p1", fptr), ("t", fptr), ("mad", fptr), ("weight", fptr), ("bias", fptr), ("res0", fptr), ("out", fptr),
                ("B", C.c_int32), ("HW", C.c_int32), ("c0", C.c_int32), ("c1", C.c_int32), ("c2", C.c_int32), ("ld0", C.c_int32), ("ld1", C.c_int32),
                ("ldt", C.c_int32), ("cout", C.c_int32), ("ldo", C.c_int32), ("ldr0", C.c_int32), ("reserved", C.c_int32)]


class RawSample(C.Structure):
    _fields_ = [("frame", C.c_int32), ("frame_clean", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("flip", C.c_int32),
                ("branch", C.c_int32), ("iso", C.c_float), ("ratio", C.c_float), ("blc", C.c_float), ("reserved", C.c_int32),
                ("k", C.c_double), ("sd", C.c_double), ("ratio64", C.c_double)]


class PhysicsSample(C.Structure):
    _fields_ = [("frame", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("flip", C.c_int32), ("read_kind", C.c_int32),
                ("row_stream", C.c_uint32), ("reserved", C.c_int32 * 2), ("ratio", C.c_double), ("K", C.c_double), ("s_read", C.c_double),
                ("lam", C.c_double), ("s_row", C.c_double), ("qstep", C.c_double), ("bias", C.c_double)]


class FramePatch(C.Structure):
    _fields_ = [("frame_out", C.c_int32), ("frame_clean", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("ax0", C.c_int32), ("ay0", C.c_int32),
                ("ax1", C.c_int32), ("ay1", C.c_int32), ("ratio", C.c_float), ("reserved", C.c_int32 * 3)]


class DevelopParams(C.Structure):
    _fields_ = [("black", C.c_int32 * 4), ("white", C.c_int32), ("scale_mul", C.c_float * 4), ("rgb_cam", C.c_float * 9),
                ("x0", C.c_int32), ("y0", C.c_int32), ("bps", C.c_int32), ("full", C.c_int32)]


RAW_PACK, RAW_PACK_SHADED, RAW_TRAIN_REAL = 0, 1, 2       # enum nd_raw_mode
RAW_RESCALE, RAW_CLIP = 1, 2
PHYS_CLIP01 = 1
CHAIN_RES_NONE, CHAIN_RES_INPUT, CHAIN_RES_INPUT_RAW = 0, 1, 2


class SamplerState(C.Structure):
    _fields_ = [("step", fptr), ("t_cur", fptr), ("t_next", fptr), ("coef", fptr), ("time_out", fptr), ("rng", fptr),
                ("n_steps", C.c_int32), ("B", C.c_int32)]


class DiffusionNoising(C.Structure):
    _fields_ = [("x0", fptr), ("noise", fptr), ("offset", fptr), ("t_in", fptr), ("sqrt_alphas_cumprod", fptr), ("sqrt_one_minus_alphas_cumprod", fptr),
                ("rng", fptr), ("t_out", fptr), ("x_t", fptr), ("target", fptr), ("noise_out", fptr), ("offset_out", fptr),
                ("seed", C.c_uint64), ("first_sample", C.c_int64), ("draw", C.c_int64), ("offset_strength", C.c_float),
                ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("T", C.c_int32),
                ("objective", C.c_int32), ("auto_normalize", C.c_int32), ("x0_channels_last", C.c_int32)]


i32, i64, u64, vp, f32, f64 = C.c_int, C.c_int64, C.c_uint64, C.c_void_p, C.c_float, C.c_double

# name -> (restype, argtypes); everything include/noisediff_hip.h declares
SIGNATURES = {
    "nd_version": (i32, []),
    "nd_last_error": (C.c_char_p, []),
    "nd_device_arch": (i32, [C.c_char_p, i32]),
    "nd_conv3x3_nhwc_f32": (i32, [C.POINTER(Conv3x3), vp]),
    "nd_conv3x3_takes": (i32, [i32, C.POINTER(Conv3x3), i32]),
    "nd_conv3x3_stat_slots": (i32, [i32, i32, i32, i32]),
    "nd_conv3x3_tiling_id": (i32, [i32, i32, i32, i32]),
    "nd_pack_conv3x3_weight_floats": (i64, [i32, i32]),
    "nd_pack_conv3x3_weight": (i32, [vp, vp, i32, i32, vp]),
    "nd_pack_conv3x3_weight_dgrad": (i32, [vp, vp, i32, i32, vp]),
    "nd_conv3x3_wino_nhwc_f32": (i32, [C.POINTER(Conv3x3), vp]),
    "nd_conv3x3_wino2_nhwc_f32": (i32, [C.POINTER(Conv3x3), vp]),
    "nd_conv3x3_wino_stat_slots": (i32, [i32, i32]),
    "nd_conv3x3_wino4_stat_slots": (i32, [i32, i32]),
    "nd_pack_conv3x3_wino_weight_floats": (i64, [i32, i32]),
    "nd_pack_conv3x3_wino_weight": (i32, [vp, vp, i32, i32, vp]),
    "nd_pack_conv3x3_wino_weight_dgrad": (i32, [vp, vp, i32, i32, vp]),
    "nd_conv3x3_wino4_nhwc_f32": (i32, [C.POINTER(Conv3x3), vp]),
    "nd_conv3x3_wino4_16_nhwc_f32": (i32, [C.POINTER(Conv3x3), vp]),
    "nd_pack_conv3x3_wino4_weight_floats": (i64, [i32, i32]),
    "nd_pack_conv3x3_wino4_weight": (i32, [vp, vp, i32, i32, vp]),
    "nd_pack_conv3x3_wino4_weight_dgrad": (i32, [vp, vp, i32, i32, vp]),
    "nd_conv3x3_wino4_splitk_plan": (i32, [i32, i32, i32, i32, i32]),
    "nd_conv3x3_wino4_splitk_workspace_floats": (i64, [i32, i32, i32, i32, i32]),
    "nd_conv3x3_wino4_splitk_nhwc_f32": (i32, [vp, vp, i32, vp]),
    "nd_conv3x3_wino4_16_splitk_plan": (i32, [i32, i32, i32, i32]),
    "nd_conv3x3_wino4_16_splitk_nhwc_f32": (i32, [vp, vp, i32, vp]),
    "nd_conv3x3_wgrad_workspace_floats": (i64, [i32, i32, i32, i32, i32]),
    "nd_conv3x3_wgrad_nhwc_f32": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "nd_groupnorm_train_workspace_floats": (i64, [i32, i32, i32]),
    "nd_linear_wgrad_workspace_floats": (i64, [i64, i32, i32]),
    "nd_groupnorm_silu_train_workspace_floats": (i64, [i32, i32, i32]),
    "nd_groupnorm_silu_train_forward_f32": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, C.c_float, vp]),
    "nd_token_sum_workspace_floats": (i64, [i32, i32, i32]),
    "nd_token_sum_f32": (i32, [vp, i32, vp, vp, i32, i32, i32, vp]),
    "nd_modulate_silu_forward_f32": (i32, [vp, i32, vp, i32, vp, i32, i64, i32, vp]),
    "nd_modulate_silu_backward_f32": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, i64, i32, vp]),
    "nd_groupnorm_silu_train_backward_f32": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_layernorm_train_workspace_floats": (i64, [i64, i32]),
    "nd_layernorm_train_forward_f32": (i32, [vp, i32, vp, vp, vp, i32, vp, i64, i32, C.c_float, vp]),
    "nd_layernorm_train_backward_f32": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, i64, i32, vp]),
    "nd_linear_wgrad_f32": (i32, [vp, i32, vp, i32, vp, vp, vp, i64, i32, i32, vp]),
    "nd_groupnorm_train_forward_f32": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, C.c_float, vp]),
    "nd_groupnorm_train_backward_f32": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_pointwise_gemm_nhwc_f32": (i32, [C.POINTER(Pointwise), vp]),
    "nd_pointwise_chain_nhwc_f32": (i32, [C.POINTER(Chain), vp]),
    "nd_pointwise_chain_supported": (i32, [i32, i32, i32, i32]),
    "nd_pack_chain_weight_floats": (i64, [i32, i32, i32]),
    "nd_pack_chain_weight": (i32, [vp, vp, i32, i32, i32, vp]),
    "nd_pointwise_chain_split_nhwc_f32": (i32, [C.POINTER(Chain), vp]),
    "nd_pack_chain_weight_split_floats": (i64, [i32, i32, i32]),
    "nd_pack_chain_weight_split": (i32, [vp, vp, i32, i32, i32, vp]),
    "nd_pointwise_gemm_split_nhwc_f32": (i32, [C.POINTER(Pointwise), vp]),
    "nd_pointwise_gemm_split_takes": (i32, [C.POINTER(Pointwise)]),
    "nd_pointwise_gemm_takes": (i32, [C.POINTER(Pointwise)]),
    "nd_pointwise_chain_takes": (i32, [i32, i32, i32, i32, i32]),
    "nd_groupnorm_train_takes": (i32, [i32, i32]),
    "nd_layernorm_train_takes": (i32, [i32]),
    "nd_rmsnorm_train_takes": (i32, [i32]),
    "nd_token_sum_takes": (i32, [i32]),
    "nd_conv3x3_wgrad_plan": (i32, [i32, i32, i32, i32, i32]),
    "nd_conv3x3_wgrad_cat_takes": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32]),
    "nd_pack_pointwise_weight_split_floats": (i64, [i32, i32]),
    "nd_pack_pointwise_weight_split": (i32, [vp, vp, i32, i32, vp]),
    "nd_pointwise_chain_tail_split_nhwc_f32": (i32, [C.POINTER(ChainTail), vp]),
    "nd_pointwise_chain_tail_takes": (i32, [i32, i32, i32, i32]),
    "nd_pointwise_narrow_fold_nhwc_f32": (i32, [C.POINTER(NarrowFold), vp]),
    "nd_pointwise_narrow_fold_takes": (i32, [i32, i32, i32, i32]),
    "nd_pack_narrow_fold_floats": (i64, [i32, i32]),
    "nd_pack_narrow_fold": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "nd_pointwise_downsample_nhwc_f32": (i32, [C.POINTER(Pointwise), vp]),
    "nd_pointwise_downsample_takes": (i32, [C.POINTER(Pointwise)]),
    "nd_pack_pointwise_weight_split_unshuffle": (i32, [vp, vp, i32, i32, i32, vp]),
    "nd_pack_attn_tail_fold_floats": (i64, [i32]),
    "nd_pack_attn_tail_fold": (i32, [vp, vp, vp, vp, vp, vp, i32, vp]),
    "nd_pack_pointwise_weight_floats": (i64, [i32, i32]),
    "nd_pack_pointwise_weight": (i32, [vp, vp, i32, i32, i32, vp]),
    "nd_pack_pointwise_weight_t": (i32, [vp, vp, i32, i32, vp]),
    "nd_pack_pointwise_weights_batch": (i32, [vp, i32, vp]),
    "nd_pack_conv3x3_wino4_weights_batch": (i32, [vp, i32, vp]),
    "nd_conv3x3_wgrad_cat_nhwc_f32": (i32, [vp, i32, i32, vp, i32, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_conv3x3_wgrad_form": (i32, [i32]),
    "nd_conv7x7_c4_wgrad_workspace_floats": (i64, [i32, i32, i32, i32]),
    "nd_conv7x7_c4_wgrad_f32": (i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_adam_chunk_elements": (i32, []),
    "nd_adam_step_f32": (i32, [vp, i32, vp, i32, f64, f64, f32, f32, vp]),
    "nd_adam_step_capturable_f32": (i32, [vp, i32, vp, i32, f32, f64, f64, f32, f32, vp]),
    "nd_adam_step_capturable_lr_f32": (i32, [vp, i32, vp, i32, vp, f64, f64, f32, f32, vp]),
    "nd_ema_chunk_elements": (i32, []),
    "nd_ema_update_f32": (i32, [vp, i32, vp, i32, vp, vp, vp, f64, i64, i64, f64, f64, f64, vp]),
    "nd_diffusion_noising_f32": (i32, [C.POINTER(DiffusionNoising), vp]),
    "nd_diffusion_train_advance": (i32, [vp, vp]),
    "nd_diffusion_loss_slice_elements": (i32, []),
    "nd_diffusion_loss_workspace_bytes": (i64, [i32, i32, i32]),
    "nd_diffusion_loss_f32": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
    "nd_diffusion_loss_backward_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "nd_denoise_loss_slice_pixels": (i32, []),
    "nd_denoise_loss_workspace_bytes": (i64, [i32, i32, i32]),
    "nd_denoise_loss_f32": (i32, [vp, i32, vp, i32, i32, i32, f64, f64, vp, vp, vp, vp]),
    "nd_denoise_loss_backward_f32": (i32, [vp, i32, vp, vp, vp, i32, i32, i32, f64, f64, vp]),
    "nd_groupnorm_finalize_f32": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, f32, vp]),
    "nd_groupnorm_finalize_train_f32": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, f32, vp]),
    "nd_layernorm_stats_f32": (i32, [vp, i32, vp, vp, i32, i32, i32, f32, vp]),
    "nd_affine_silu_add_f32": (i32, [vp, i32, vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, vp]),
    "nd_linear_rows_f32": (i32, [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "nd_sinusoidal_time_emb_f32": (i32, [vp, vp, vp, i32, i32, vp]),
    "nd_cond_step_lds_bytes": (i64, [i32, i32]),
    "nd_cond_step_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_cond_table_build_f32": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    "nd_cond_step_table_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp]),
    "nd_cond_step_ptable_f32": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp]),
    "nd_embedding_rows_f32": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "nd_conv7x7_c4_f32": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "nd_pack_conv7x7_weight": (i32, [vp, vp, i32, vp]),
    "nd_conv7x7_c4_split_f32": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "nd_pack_conv7x7_weight_split_floats": (i64, [i32]),
    "nd_pack_conv7x7_weight_split": (i32, [vp, vp, i32, vp]),
    "nd_pos_enc_f32": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_maxpool2x2_nhwc_f32": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "nd_nchw_to_nhwc_pad_f32": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "nd_nchw_to_nhwc_f32": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "nd_nhwc_to_nchw_f32": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "nd_sampler_begin_step": (i32, [C.POINTER(SamplerState), vp]),
    "nd_sampler_advance": (i32, [C.POINTER(SamplerState), vp]),
    "nd_sampler_step_ddpm_f32": (i32, [vp, vp, vp, i64, C.POINTER(SamplerState), i32, u64, i64, i32, i32, i32, vp]),
    "nd_sampler_step_ddim_f32": (i32, [vp, vp, vp, i64, C.POINTER(SamplerState), i32, u64, i64, i32, i32, i32, vp]),
    "nd_philox_normal_f32": (i32, [vp, u64, i64, i32, i32, i32, i32, vp]),
    "nd_attention_mfma_f32": (i32, [vp, i32, vp, i32, i32, i32, i32, i32, vp]),
    "nd_attention_train_forward_f32": (i32, [vp, i32, vp, i32, vp, i32, i32, i32, i32, vp]),
    "nd_attention_backward_workspace_floats": (i64, [i32, i32, i32]),
    "nd_attention_backward_f32": (i32, [vp, i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, vp]),
    "nd_linear_attention_backward_workspace_floats": (i64, [i32, i32, i32]),
    "nd_linear_attention_backward_f32": (i32, [vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, vp]),
    "nd_rmsnorm_backward_workspace_floats": (i64, [i64, i32]),
    "nd_rmsnorm_backward_f32": (i32, [vp, i32, vp, i32, vp, vp, i32, vp, vp, i32, i32, i32, vp]),
    "nd_linear_attention_workspace_floats": (i64, [i32, i32, i32]),
    "nd_linear_attention_f32": (i32, [vp, i32, vp, i32, vp, i32, i32, i32, i32, vp]),
    "nd_rmsnorm_nhwc_f32": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, vp]),
    "nd_rmsnorm_add_nhwc_f32": (i32, [vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, vp]),
    "nd_stream_create": (i32, [C.POINTER(vp)]),
    "nd_stream_destroy": (i32, [vp]),
    "nd_stream_sync": (i32, [vp]),
    "nd_graph_begin": (i32, [vp]),
    "nd_graph_end": (i32, [vp, C.POINTER(vp)]),
    "nd_graph_launch": (i32, [vp, vp]),
    "nd_graph_destroy": (i32, [vp]),
    "nd_event_create": (i32, [C.POINTER(vp)]),
    "nd_event_record": (i32, [vp, vp]),
    "nd_event_elapsed_ms": (i32, [vp, vp, C.POINTER(f32)]),
    "nd_event_destroy": (i32, [vp]),
    "nd_event_create_untimed": (i32, [C.POINTER(vp)]),
    "nd_stream_wait_event": (i32, [vp, vp]),
    "nd_stream_device": (i32, [vp]),
    "nd_conv3x3_wgrad_leaky_nhwc_f32": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "nd_conv3x3_wgrad_cat_workspace_floats": (i64, [i32, i32, i32, i32, i32, i32]),
    "nd_conv3x3_wgrad_cat_leaky_second_nhwc_f32": (i32, [vp, i32, i32, vp, i32, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_leaky_grad_join_f32": (i32, [vp, vp, vp, i32, vp, i32, i32, i32, i32, vp]),
    "nd_linear_wgrad_leaky_f32": (i32, [vp, i32, vp, i32, vp, vp, vp, i64, i32, i32, vp]),
    "nd_convt2x2_wgrad_workspace_floats": (i64, [i32, i32, i32, i32, i32]),
    "nd_convt2x2_wgrad_leaky_f32": (i32, [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "nd_pointwise_gemm_unshuffle_crop_nhwc_f32": (i32, [C.POINTER(Pointwise), i32, i32, vp]),
    "nd_image_quality_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "nd_image_quality_f32": (i32, [vp, vp, vp, f64, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_illum_scale_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "nd_illum_scale_f32": (i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_illum_apply_f32": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_histogram_chunk_elements": (i32, []),
    "nd_histogram_workspace_bytes": (i64, [i32, i64, i32]),
    "nd_histogram_f32": (i32, [vp, i32, i64, vp, i32, vp, vp, vp]),
    "nd_kl_div_f64": (i32, [vp, vp, i64, i64, i32, i32, i32, vp, vp]),
    "nd_kl_div_hist_f64": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "nd_patch_std_mean_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "nd_patch_std_mean_f32": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_level_table_bytes": (i64, [i32]),
    "nd_level_moments_reset": (i32, [vp, i32, vp, vp]),
    "nd_level_moments_f32": (i32, [vp, vp, i64, f32, i32, vp, vp, vp]),
    "nd_level_stats_f64": (i32, [vp, i32, vp, vp, vp, vp]),
    "nd_level_curve_f64": (i32, [vp, vp, i32, f32, i32, vp, vp, vp, vp]),
    "nd_theil_sen_workspace_bytes": (i64, [i32, i64]),
    "nd_theil_sen_f64": (i32, [vp, vp, vp, i32, vp, i64, i32, f64, vp, vp, vp]),
    "nd_denoise_batch_f32": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, u64, i64, i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "nd_philox_poisson_f32": (i32, [vp, vp, u64, i64, i32, i32, i64, vp]),
    "nd_pack_darkshading_f32": (i32, [vp, vp, i32, i32, vp]),
    "nd_raw_pack_u16_f32": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, i32, i32, f32, f32, vp, vp, i32, i32, i32, vp]),
    "nd_raw_poisson_gaussian_f32": (i32, [vp, i32, i32, i32, vp, vp, u64, i64, i32, vp, vp, vp, vp, f32, f32, vp, vp, i32, i32, i32, vp]),
    "nd_raw_to_bayer_u16": (i32, [vp, vp, C.POINTER(C.c_int32), i32, i32, i32, i32, vp]),
    "nd_raw_diffusion_batch_f32": (i32, [vp, i32, i32, i32, vp, f32, f32, vp, vp, vp, vp, i32, i32, i32, vp]),
    "nd_raw_physics_noise_f32": (i32, [vp, i32, i32, i32, vp, vp, u64, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, i32, vp, vp, vp, i32, i32, i32,
                                       vp]),
    "nd_raw_develop": (i32, [vp, vp, i32, i32, i32, C.POINTER(DevelopParams), vp, vp, i32, i32, vp]),
    "nd_frame_assemble": (i32, [vp, vp, i32, i32, i32, vp, f32, f32, vp, vp, vp, i32, i32, i32, vp]),
    "nd_dark_stack_add_u16": (i32, [vp, i32, i32, i32, vp, vp]),
    "nd_dark_stack_mean_f64": (i32, [vp, i32, i32, i32, vp, vp]),
    "nd_calib_row_sums_i64": (i32, [vp, i32, i32, i32, vp, i32, vp, vp]),
    "nd_calib_residual_f64": (i32, [vp, i32, i32, i32, vp, i32, vp, vp, vp]),
    "nd_calib_row_stats_f64": (i32, [vp, i32, i32, i32, i32, vp, i32, vp, vp]),
    "nd_calib_quantiles_f64": (i32, [i64, i32, f64, vp, vp]),
    "nd_ppcc_workspace_bytes": (i64, [i32]),
    "nd_probplot_f64": (i32, [vp, i32, i64, i32, vp, vp, vp, vp]),
    "nd_ppcc_max_f64": (i32, [vp, i32, i64, f64, f64, f64, i32, vp, vp, vp]),
}

_UNCHECKED = {"nd_conv3x3_takes", "nd_pointwise_gemm_takes", "nd_pointwise_gemm_split_takes", "nd_pointwise_chain_supported", "nd_pointwise_chain_takes",
              "nd_groupnorm_train_takes", "nd_layernorm_train_takes", "nd_rmsnorm_train_takes", "nd_token_sum_takes", "nd_conv3x3_wgrad_plan", "nd_conv3x3_wgrad_cat_takes",
              "nd_pointwise_chain_tail_takes", "nd_pointwise_narrow_fold_takes", "nd_pack_narrow_fold_floats", "nd_pointwise_downsample_takes", "nd_pack_attn_tail_fold_floats", "nd_version", "nd_last_error", "nd_stream_device", "nd_conv3x3_wgrad_form", "nd_adam_chunk_elements", "nd_ema_chunk_elements", "nd_conv7x7_c4_wgrad_workspace_floats", "nd_conv3x3_stat_slots", "nd_conv3x3_tiling_id", "nd_pack_conv3x3_weight_floats",
              "nd_pack_pointwise_weight_floats", "nd_linear_attention_workspace_floats", "nd_conv3x3_wino_stat_slots", "nd_conv3x3_wino4_stat_slots",
              "nd_pack_conv3x3_wino_weight_floats", "nd_pack_conv3x3_wino4_weight_floats", "nd_conv3x3_wino4_splitk_plan", "nd_conv3x3_wino4_16_splitk_plan", "nd_conv3x3_wino4_splitk_workspace_floats", "nd_token_sum_workspace_floats", "nd_cond_step_lds_bytes", "nd_conv3x3_wgrad_workspace_floats",
              "nd_groupnorm_train_workspace_floats", "nd_linear_wgrad_workspace_floats",
              "nd_layernorm_train_workspace_floats", "nd_groupnorm_silu_train_workspace_floats", "nd_conv3x3_wgrad_cat_workspace_floats",
              "nd_convt2x2_wgrad_workspace_floats", "nd_image_quality_workspace_bytes", "nd_illum_scale_workspace_bytes",
              "nd_histogram_chunk_elements", "nd_histogram_workspace_bytes", "nd_patch_std_mean_workspace_bytes", "nd_level_table_bytes", "nd_ppcc_workspace_bytes",
              "nd_theil_sen_workspace_bytes", "nd_attention_backward_workspace_floats", "nd_linear_attention_backward_workspace_floats",
              "nd_rmsnorm_backward_workspace_floats", "nd_diffusion_loss_slice_elements", "nd_diffusion_loss_workspace_bytes",
              "nd_denoise_loss_slice_pixels", "nd_denoise_loss_workspace_bytes"}

_lib: Optional[C.CDLL] = None


def load(path: str = LIB_PATH) -> C.CDLL:
    """dlopen the library and attach prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it ships its own libamdhip64; loading ours before torch's puts two HIP runtimes in the process
    # and the second one to initialise reports "no ROCm-capable device"
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise HipError(f"{path} is missing: the HIP library is the product and there is no fallback. "
                       "Build it with `python -m noisediff_amd.build`.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(code: int, what: str = "") -> None:
    if code != 0:
        msg = load().nd_last_error().decode(errors="replace")
        raise HipError(f"{what or 'libnoisediff_hip'} failed with code {code}: {msg}")


def call(name: str, *args):
    """Checked call: raises HipError on a non-zero status."""
    r = getattr(load(), name)(*args)
    if name not in _UNCHECKED:
        check(r, name)
    return r


def ptr(t) -> Optional[int]:
    """Device address of an operand: None (NULL), an integer address, or anything with data_ptr() (a torch tensor)."""
    return t if t is None or isinstance(t, int) else t.data_ptr()


# ---- launch descriptors, each filled in ONE place.  Operands are what ptr() takes; a width that is not given is the operand's last dimension.  The structs hold raw
# addresses only, so every builder hangs the operands it was given on the struct (``_refs``; a struct built from a source carries that source's along): whoever holds
# a descriptor holds its operands.  Positional parameters and plain assignments, no keyword dictionaries: a training step builds several hundred of these.
def src(t, t2=None, mode: int = PRO_NONE, c: Optional[int] = None, ld: Optional[int] = None, offset: int = 0, c1: Optional[int] = None, ld1: Optional[int] = None,
        mad=None, map=None, vec=None, gamma=None, beta=None, rowstats=None, upsample: int = 0, unshuffle: int = 0, map_blocked: int = 0) -> Src:
    """An nd_src: ``c`` channels of ``t`` at a pixel stride of ``ld`` from element ``offset`` on, then (``t2``) ``c1`` channels of a second source at ``ld1``."""
    s = Src()
    s.p0 = ptr(t) + 4 * offset if offset else ptr(t)
    s.c0, s.ld0, s.mode = t.shape[-1] if c is None else c, t.shape[-1] if ld is None else ld, mode
    if t2 is not None:
        s.p1, s.c1, s.ld1 = ptr(t2), t2.shape[-1] if c1 is None else c1, t2.shape[-1] if ld1 is None else ld1
    elif c1 or ld1:                      # widths without addresses: a question to nd_*_takes
        s.c1, s.ld1 = c1 or 0, ld1 or 0
    if upsample or unshuffle or map_blocked:         # (a new struct is all zeros: the common plain source sets nothing more)
        s.upsample, s.unshuffle, s.map_blocked = upsample, unshuffle, map_blocked
    if not (mad is None and map is None and vec is None and gamma is None and beta is None and rowstats is None):
        s.mad, s.map, s.vec, s.gamma, s.beta, s.rowstats = ptr(mad), ptr(map), ptr(vec), ptr(gamma), ptr(beta), ptr(rowstats)
    s._refs = (t, t2, mad, map, vec, gamma, beta, rowstats)
    return s


def src_rows(s: Src, b0: int, pixels: int, map_width: int = 0) -> Src:
    """A copy of ``s`` that starts at sample ``b0``: every per-sample operand it has (p0, p1, mad, map, vec) moved by its own stride.  ``pixels``: the source's
    pixels per sample (a quarter of the output's behind ``upsample``); ``map_width``: the map's floats per pixel, 2 (c0 + c1) stored, fewer where the kernel forms it."""
    r = Src.from_buffer_copy(s)
    r._refs = getattr(s, "_refs", ())
    for name, step in (("p0", pixels * s.ld0), ("p1", pixels * s.ld1), ("mad", 3 * (s.c0 + s.c1)), ("map", pixels * map_width), ("vec", s.c0 + s.c1)) if b0 else ():
        if getattr(s, name):
            setattr(r, name, getattr(s, name) + 4 * b0 * step)
    return r


def conv3x3(s: Src, weight, bias, out, B: int, H: int, W: int, cin: int, cout: int, ldo: Optional[int] = None, stats=None, slot_count=None) -> Conv3x3:
    """An nd_conv3x3 over the source ``s``; ``stats`` with ``slot_count``: the statistics epilogue's two outputs."""
    d = Conv3x3()
    d.src, d.weight, d.bias, d.out = s, ptr(weight), ptr(bias), ptr(out)
    if stats is not None:
        d.stats, d.slot_count = ptr(stats), ptr(slot_count)
    d.B, d.H, d.W, d.cin, d.cout, d.ldo = B, H, W, cin, cout, cout if ldo is None else ldo
    d._refs = (getattr(s, "_refs", ()), weight, bias, out, stats, slot_count)
    return d


def pointwise(s: Src, weight, bias, out, B: int, HW: int, W: int, cin: int, cout: int, ldo: Optional[int] = None, act: int = ACT_NONE, res0=None, res1=None, vec=None,
              gn_t=None, gn_mad=None, shuffle=None, ldr0: Optional[int] = None, ldr1: Optional[int] = None, ldt: Optional[int] = None) -> Pointwise:
    """An nd_pointwise over the source ``s``; ``gn_t`` with ``gn_mad``: silu(GroupNorm(gn_t)) added in the epilogue; ``shuffle`` = (c, h, w): the pixel-shuffled store."""
    d = Pointwise()
    d.src, d.weight, d.bias, d.out, d.vec = s, ptr(weight), ptr(bias), ptr(out), ptr(vec)
    d.B, d.HW, d.W, d.cin, d.cout, d.ldo, d.act = B, HW, W, cin, cout, cout if ldo is None else ldo, act
    if res0 is not None:
        d.res0, d.ldr0 = ptr(res0), res0.shape[-1] if ldr0 is None else ldr0
    if res1 is not None:
        d.res1, d.ldr1 = ptr(res1), res1.shape[-1] if ldr1 is None else ldr1
    if gn_t is not None:
        d.gn_t, d.ldt, d.gn_mad = ptr(gn_t), gn_t.shape[-1] if ldt is None else ldt, ptr(gn_mad)
    if shuffle is not None:
        d.shuffle_c, d.shuffle_h, d.shuffle_w = shuffle
    d._refs = (getattr(s, "_refs", ()), weight, bias, out, res0, res1, vec, gn_t, gn_mad)
    return d

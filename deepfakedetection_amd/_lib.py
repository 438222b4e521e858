"""ctypes binding of libdfd_hip.so (declared in include/dfd_hip.h).

The product path has no CPU or ATen fallback: if the shared object is missing or a
symbol cannot be resolved, importing/using the kernels raises immediately.
"""

from __future__ import annotations

import ctypes
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_int64, c_long, c_size_t, c_uint32, c_uint64, c_void_p
from pathlib import Path

import os as _os

# DFD_LIB_PATH: load another build of the same library (kernel timing experiments)
LIB_PATH = Path(_os.environ.get("DFD_LIB_PATH") or Path(__file__).resolve().parent / "libdfd_hip.so")

DFD_OK = 0
ERRORS = {-1: "DFD_EINVAL", -2: "DFD_EUNSUPPORTED", -3: "DFD_ELAUNCH", -4: "DFD_EWORKSPACE"}
F32, BF16 = 0, 1
ACT_NONE, ACT_SILU, ACT_RELU, ACT_GELU = 0, 1, 2, 3
PRO_NONE, PRO_BN_ACT, PRO_BN_ACT_GATE, PRO_AFFINE2 = 0, 1, 2, 3
MAX_PARTIALS = 1024
ADAMW_TABLE_COLS = 5
ADAMW_HP_LEN = 8
EMA_TABLE_COLS = 4
EMA_LERP, EMA_COPY = 0, 1
CLIP_MODE_NORM, CLIP_MODE_VALUE = 0, 1
CLIP_CFG_LEN = 2
CLIP_STATE_LEN = 8
(CLIP_NORM, CLIP_COEF, CLIP_SKIP, CLIP_STEPS, CLIP_CLIPPED, CLIP_SKIPPED, CLIP_NORM_SUM, CLIP_NORM_MAX) = range(8)
MIX_JOB_WORDS = 8
MIX_KEEP, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2
MIX_NHWC, MIX_NCHW = 0, 1
AUG_MAX_OPS = 4
BLUR_MAX_RADIUS = 32
BLUR_MAX_PIXELS = 78 * 1024
AUG_POLICY_JOB_WORDS = 16 + 2 + 9 * AUG_MAX_OPS     # struct dfd_augment_policy_job in int32 words (216 bytes)
# csrc/dfd_metrics.hip (the DFD_ROC_* / DFD_CONFUSION_* constants of include/dfd_hip.h)
ROC_TILE = 2048                     # scores per workgroup of dfd_roc_curve's tile passes
ROC_SCAN_WIDTH = 1024               # tile totals its scan takes per trip
ROC_MAX_N = 1 << 28
ROC_MAX_CUTS = 4096
ROC_STATS_LEN = 5
(ROC_P, ROC_N, ROC_G, ROC_NONFINITE, ROC_TWO_U) = range(5)
CONFUSION_LDS_MAX_J = 128           # largest J whose J x J int32 histogram stays in LDS
CONFUSION_MAX_J = 1024
# csrc/dfd_calib.hip (the DFD_CALIB_* constants of include/dfd_hip.h)
CALIB_MAX_N = 1 << 28
CALIB_MAX_J = 1024
CALIB_MAX_BINS = 64
CALIB_MAX_BETAS = 64
CALIB_THREAD_MAX_J = 16             # widest row that one thread takes; above it one wave per row
CALIB_MAX_BLOCKS = 1024             # stage-1 workgroups at most
CALIB_STAGE2_WIDTH = 64             # partials the stage-2 loop takes per trip
CALIB_LAYOUT_THREAD, CALIB_LAYOUT_WAVE = 0, 1
(CALIB_VALID, CALIB_NONFINITE, CALIB_OOB, CALIB_CORRECT) = range(4)
# csrc/dfd_fuse.hip (the DFD_FUSE_* constants of include/dfd_hip.h)
FUSE_MAX_MODELS = 8
FUSE_MAX_CANDS = 8
FUSE_MAX_J = 1024
FUSE_MAX_N = 1 << 28
FUSE_MAX_TERMS = 45                 # nll + K gradient entries + the K (K + 1) / 2 of the Hessian's upper triangle at K = 8
FUSE_THREAD_MAX_KJ = 16             # largest K * J that one thread takes; above it one wave per row
FUSE_MAX_BLOCKS = 1024              # stage-1 workgroups at most
FUSE_STAGE2_WIDTH = 64              # partials the stage-2 loop takes per trip
FUSE_LAYOUT_THREAD, FUSE_LAYOUT_WAVE = 0, 1
FUSE_LOGIT, FUSE_PROB = 0, 1
# csrc/dfd_boot.hip (the DFD_BOOT_* constants of include/dfd_hip.h)
BOOT_STREAM = 0x626F6F74            # "boot": the last counter word of every bootstrap draw
BOOT_MAX_N = 1 << 24
BOOT_MAX_REPLICATES = 65536
BOOT_MAX_MEMBERS = 8
BOOT_STATS_LEN = 10
(BOOT_P, BOOT_N, BOOT_TWO_U, BOOT_TP, BOOT_FP, BOOT_HITS, BOOT_F0, BOOT_T0, BOOT_F1, BOOT_T1) = range(10)
BOOT_SCRATCH_BYTES = 512            # reduction scratch in front of the LDS tier's counts
BOOT_LDS_MAX_N = (160 * 1024 - BOOT_SCRATCH_BYTES) // 4       # largest n whose uint32 counts stay in one workgroup's LDS
BOOT_DRAW_TILE = 4096               # draws per workgroup of the global tier's draw kernel
BOOT_TIER_LDS, BOOT_TIER_GLOBAL = 0, 1
BOOT_GROUPED_MAX_WEIGHT = (1 << 31) - 1     # the cluster bootstrap: groups times the largest group at most
# csrc/dfd_group.hip (the DFD_GROUP_* constants of include/dfd_hip.h)
GROUP_MEAN, GROUP_VOTE, GROUP_MAX = 0, 1, 2
GROUP_MAX_N = 1 << 24
GROUP_MAX_J = 1024
GROUP_LDS_BYTES = 65536             # the workspace size up to which every workgroup keeps a private copy of the cells in LDS
GROUP_LDS_MAX_BLOCKS = 256
GROUP_GLOBAL_MAX_BLOCKS = 2048
GROUP_TIER_LDS, GROUP_TIER_GLOBAL = 0, 1
(GROUP_INVALID, GROUP_OOB, GROUP_MIXED, GROUP_EMPTY) = range(4)


class DwShape(Structure):
    _fields_ = [(n, c_int) for n in ("N", "H", "W", "C", "Ho", "Wo", "k", "stride", "pad_top", "pad_left")]


class StemShape(Structure):
    _fields_ = [(n, c_int) for n in ("N", "H", "W", "Cout", "Ho", "Wo", "k", "stride", "pad_top", "pad_left")]


class Mat(Structure):
    """struct dfd_mat: element (b, h, r, c) at base + b*sb + h*sh + r*sr + c*sc (element units)."""

    _fields_ = [(n, c_long) for n in ("sb", "sh", "sr", "sc")]


class Prologue(Structure):
    _fields_ = [
        ("mode", c_int), ("act", c_int), ("HW", c_int), ("_pad", c_int),
        ("a2", c_void_p), ("coef", c_void_p), ("gate", c_void_p),
    ]


P = c_void_p
_PI = POINTER(c_int)

# name -> (restype, argtypes); every symbol include/dfd_hip.h declares
SIGNATURES: dict[str, tuple] = {
    "dfd_version": (c_int, []),
    "dfd_tune": (c_int, [c_int, c_int]),
    "dfd_dw_mm_plan": (c_int, [POINTER(DwShape), c_int, _PI]),
    "dfd_bn_finalize": (c_int, [P, c_int, c_int, c_double, P, P, P, P, c_float, c_float, P, P]),
    "dfd_bn_eval_coeffs": (c_int, [P, P, P, P, c_float, c_int, P, P]),
    "dfd_bn_bwd_finalize": (c_int, [P, c_int, c_int, c_double, P, P, c_int, P, P, c_int, P, P]),
    "dfd_bn_act_apply": (c_int, [c_int, P, P, c_int, P, P, P, c_int, c_int, c_int, P]),
    "dfd_bn_bwd_reduce": (c_int, [c_int, P, P, P, P, c_int, c_int, c_int, P, c_int, _PI, P]),
    "dfd_gemm_bias_act": (c_int, [c_int, P, P, c_int, c_int, c_int, P, c_int, P, P, c_int, P, P, P]),
    "dfd_gemm_plan": (c_int, [c_int, c_int, c_int]),
    "dfd_pw_ntd_plan": (c_int, [c_int, c_int, c_int]),
    "dfd_bias_grad_ws": (c_size_t, [c_int, c_int, c_int]),
    "dfd_bias_grad": (c_int, [c_int, P, P, c_int, c_int, c_int, P, c_int, P, c_size_t, P]),
    "dfd_act_bn_bwd": (c_int, [c_int, P, P, P, P, P, c_int, P, c_int, c_int, c_int, P, c_int, _PI, P]),
    "dfd_act_bn_bwd_se": (c_int, [c_int, P, P, P, P, P, c_int, P, c_int, c_int, c_int, P, c_int, _PI, P, P, c_int, P, P, P, P, c_int, P]),
    "dfd_prep_weights_multi": (c_int, [P, c_int, P]),
    "dfd_resize_crop_u8": (c_int, [P, P, P, c_int, c_int, c_int, c_int, P]),
    "dfd_augment_u8": (c_int, [P, P, P, c_int, c_int, c_int, P]),
    "dfd_image_prep": (c_int, [P, P, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), P, P, P]),
    "dfd_pool_ws": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dfd_pool_act": (c_int, [c_int, P, P, c_int, P, c_int, c_int, c_int, P, c_size_t, P]),
    "dfd_pool_bwd_reduce": (c_int, [c_int, P, P, P, c_int, P, c_int, c_int, c_int, P, c_size_t, P]),
    "dfd_scale_rows": (c_int, [c_int, P, P, P, c_int, c_int, c_int, P]),
    "dfd_se_fc_fwd": (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P]),
    "dfd_se_fc_bwd": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, c_int, P, P]),
    "dfd_dwconv_fwd": (c_int, [c_int, P, P, c_int, P, P, POINTER(DwShape), P, c_int, _PI, P]),
    "dfd_dwconv_bwd_data": (c_int, [c_int, P, P, P, P, P, P, c_int, P, POINTER(DwShape), P, c_int, _PI, P]),
    "dfd_dwconv_bwd_weight": (c_int, [c_int, P, P, P, P, P, c_int, P, POINTER(DwShape), c_int, P, c_size_t, P]),
    "dfd_dwconv_bwd_weight_ws": (c_size_t, [POINTER(DwShape)]),
    "dfd_pwconv_fwd": (c_int, [c_int, P, POINTER(Prologue), P, P, P, c_int, c_int, c_int, P, c_int, _PI, P]),
    "dfd_pwconv_wgrad": (c_int, [c_int, P, POINTER(Prologue), c_int, P, POINTER(Prologue), c_int, c_int, P, c_int, P, c_size_t, P]),
    "dfd_pwconv_wgrad_ws": (c_size_t, [c_int, c_int, c_int]),
    "dfd_gradcam_map": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P]),
    "dfd_cam_render": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P, c_double, P, P, P, c_size_t, P]),
    "dfd_cam_render_ws": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dfd_pwconv_bwd_fused": (c_int, [c_int, P, P, P, P, P, P, c_int, c_int, c_int, P, P, c_int, P, c_size_t, P]),
    "dfd_pw_prep_weights": (c_int, [c_int, P, P, P, c_int, c_int, P]),
    "dfd_stem_conv_fwd": (c_int, [c_int, P, P, P, POINTER(StemShape), P, c_int, _PI, P]),
    "dfd_stem_conv_wgrad": (c_int, [c_int, P, P, P, P, P, POINTER(StemShape), c_int, P, c_size_t, P]),
    "dfd_stem_conv_wgrad_ws": (c_size_t, [POINTER(StemShape)]),
    "dfd_dropout": (c_int, [P, P, c_float, P, c_int, P]),
    "dfd_linear_fwd": (c_int, [P, P, P, P, c_int, c_int, c_int, P]),
    "dfd_linear_bwd": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    "dfd_ce_loss": (c_int, [P, P, c_int, c_int, c_float, c_float, P, P, P, P]),
    "dfd_softmax_argmax": (c_int, [P, c_int, c_int, P, P, P]),
    "dfd_adamw_step": (c_int, [P, c_int, P, P]),
    # ---- ABI 137
    "dfd_ema_update": (c_int, [P, c_int, P, P]),
    # ---- ABI 138
    "dfd_mix_batch": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_ce_loss_soft": (c_int, [P, P, c_int, c_int, c_float, c_float, P, P, P, P]),
    # ---- ABI 139
    "dfd_augment_policy_u8": (c_int, [P, P, P, P, c_int, c_int, c_int, P]),
    # ---- ABI 140
    "dfd_grad_sumsq": (c_int, [P, c_int, P, P]),
    "dfd_grad_clip_finish": (c_int, [P, c_int, P, P, P, P]),
    "dfd_adamw_step_clip": (c_int, [P, c_int, P, P, P, P]),
    # ---- ABI 142
    "dfd_jpeg_u8": (c_int, [P, P, P, P, c_int, c_int, c_int, P]),
    "dfd_jpeg_ws": (c_size_t, [c_int, c_int, c_int]),
    # ---- ABI 144
    "dfd_blur_u8": (c_int, [P, P, P, c_int, c_int, c_int, P]),
    # ---- ABI 146
    "dfd_roc_ws": (c_size_t, [c_int]),
    "dfd_roc_curve": (c_int, [P, P, c_int, c_int64, P, c_size_t, P, P, P, P, P]),
    "dfd_roc_sweep": (c_int, [P, P, P, P, c_int, P, c_int, P, P, P]),
    "dfd_confusion": (c_int, [P, P, c_int, c_int, P, P, P]),
    # ---- ABI 147
    "dfd_ce_loss_w": (c_int, [P, P, c_int, c_int, c_int, c_float, c_float, P, c_float, P, P, P, P, P]),
    # ---- ABI 148
    "dfd_bgemm_plan": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "dfd_attn_softmax_plan": (c_int, [c_int, c_int, _PI, _PI]),
    # ---- ABI 149
    "dfd_rowtable_grad_plan": (c_int, [c_int, c_long, c_int, c_int, _PI, POINTER(c_long), _PI]),
    # ---- ABI 150
    "dfd_calib_bins_ws": (c_size_t, [c_int, c_int]),
    "dfd_calib_bins": (c_int, [P, P, c_int, c_int, c_int, P, c_size_t, P, P, P, P]),
    "dfd_calib_nll_ws": (c_size_t, [c_int, c_int, c_int]),
    "dfd_calib_nll": (c_int, [P, P, c_int, c_int, POINTER(c_double), c_int, P, c_size_t, P, P, P]),
    "dfd_calib_plan": (c_int, [c_int, c_int, _PI]),
    "dfd_softmax_argmax_t": (c_int, [P, c_int, c_int, c_float, P, P, P]),
    # ---- ABI 151
    "dfd_fuse_scores": (c_int, [P, c_int, c_int, c_int, c_int, POINTER(c_double), POINTER(c_double), P, P, P, P, P]),
    "dfd_fuse_nll_ws": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dfd_fuse_nll": (c_int, [P, c_int, P, c_int, c_int, POINTER(c_double), c_int, P, c_size_t, P, P, P]),
    "dfd_fuse_agree": (c_int, [P, c_int, P, c_int, c_int, P, P, P, P]),
    "dfd_fuse_plan": (c_int, [c_int, c_int, c_int, _PI]),
    # ---- ABI 152
    "dfd_stem_bwd_fused_ok": (c_int, [c_int, POINTER(StemShape), P]),
    "dfd_stem_bwd_fused": (c_int, [c_int, P, P, P, P, c_int, P, P, POINTER(StemShape), c_int, P, c_size_t, c_int, P]),
    # ---- ABI 153
    "dfd_boot_ws": (c_size_t, [c_int, c_int]),
    "dfd_boot_plan": (c_int, [c_int, c_int, c_int, c_size_t, _PI]),
    "dfd_boot_counts": (c_int, [c_int, c_int, c_int, c_uint64, P, P]),
    "dfd_boot_stats": (c_int, [P, P, c_int, P, P, POINTER(c_double), c_int, c_int, c_uint64, P, c_size_t, P, P]),
    # ---- ABI 154
    "dfd_boot_ws_grouped": (c_size_t, [c_int, c_int, c_int]),
    "dfd_boot_plan_grouped": (c_int, [c_int, c_int, c_int, c_int, c_int, c_size_t, _PI]),
    "dfd_boot_stats_grouped": (c_int, [P, P, c_int, P, P, POINTER(c_double), P, c_int, c_int, c_int, c_int, c_uint64, P, c_size_t, P, P]),
    "dfd_group_ws": (c_size_t, [c_int, c_int, c_int]),
    "dfd_group_plan": (c_int, [c_int, c_int, c_int, _PI]),
    "dfd_group_pool": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P, P, P, P, P, P]),
    # ---- ABI 111
    "dfd_bn_eval_coeffs_multi": (c_int, [P, c_int, P]),
    "dfd_sum_batch_begin": (c_int, []),
    "dfd_sum_batch_end": (c_int, []),
    "dfd_sum_batch_end_deferred": (c_int, []),
    "dfd_sum_passengers_flush": (c_int, [P]),
    "dfd_sum_passengers_discard": (c_int, []),
    "dfd_se_fwd": (c_int, [c_int, P, P, c_int, c_int, c_int, c_int, P, P, P, P, c_int, c_int, P, P, P, P, P, c_size_t, P]),
    "dfd_se_bwd": (c_int, [c_int, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, c_int, c_int, P, P, P, P, P, P, c_int,
                           P, c_size_t, P, P]),
    # ---- ABI 112 (eval form of the MBConv block)
    "dfd_pwconv_fwd_eval": (c_int, [c_int, P, P, P, c_int, P, c_int, c_int, c_int, P]),
    "dfd_dwconv_fwd_eval_tiles": (c_int, [c_int, P]),
    "dfd_dwconv_fwd_eval": (c_int, [c_int, P, P, P, c_int, P, P, P, P, P]),
    "dfd_se_fwd_parts": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P, P, c_int, c_int, P, P, P, P, P]),
    # ---- ABI 110
    "dfd_bn_finalize_ex": (c_int, [P, c_int, c_int, c_double, P, P, P, P, P, P, c_float, c_float, P, P]),
    "dfd_bn_eval_coeffs_ex": (c_int, [P, P, P, P, P, P, c_float, c_int, P, P]),
    "dfd_bn_bwd_finalize_ex": (c_int, [P, c_int, c_int, c_double, P, P, P, P, c_int, P, P, P, P, c_int, P, P]),
    "dfd_affine2_apply": (c_int, [c_int, P, P, P, P, c_long, c_int, P]),
    "dfd_bn_add_act": (c_int, [c_int, P, P, P, c_int, P, c_long, c_int, P]),
    "dfd_bn_add_act_bwd": (c_int, [c_int, P, P, P, P, c_int, P, c_long, c_int, P, c_int, _PI, P]),
    "dfd_channel_stats": (c_int, [c_int, P, c_long, c_int, P, c_int, _PI, P]),
    "dfd_sum_rows": (c_int, [P, c_int, c_long, P, c_int, P]),
    "dfd_sum_rows_deferred": (c_int, [P, c_int, c_long, P, c_int, P]),
    "dfd_up2_act_fwd": (c_int, [c_int, P, c_int, P, c_int, c_int, c_int, c_int, P]),
    "dfd_up2_act_bwd": (c_int, [c_int, P, P, c_int, P, c_int, c_int, c_int, c_int, P, P]),
    "dfd_subsample_add": (c_int, [c_int, P, P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_subsample_add_bwd": (c_int, [c_int, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_bgemm": (c_int, [c_int, P, POINTER(Mat), c_int, P, POINTER(Mat), c_int, P, POINTER(Mat), P, c_float, c_int, c_int,
                          c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_attn_softmax_fwd": (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    "dfd_attn_softmax_bwd": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    "dfd_bias_gather": (c_int, [P, P, P, c_int, c_int, c_long, P]),
    "dfd_bias_scatter": (c_int, [P, P, P, c_int, c_int, c_long, c_int, P]),
    "dfd_im2col": (c_int, [c_int, P, P, c_int, P, POINTER(DwShape), P]),
    "dfd_conv_fwd": (c_int, [c_int, P, POINTER(DwShape), P, c_int, P, c_int, P, P, c_int, POINTER(c_int), P]),
    "dfd_conv_wgrad_ws": (c_size_t, [POINTER(DwShape), c_int]),
    "dfd_conv_wgrad": (c_int, [c_int, P, P, c_int, P, POINTER(DwShape), P, c_int, P, c_int, P, c_size_t, P]),
    "dfd_col2im": (c_int, [c_int, P, P, POINTER(DwShape), P]),
    "dfd_conv_weight_perm": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_layernorm_fwd": (c_int, [c_int, P, P, P, c_float, P, P, c_long, c_int, P]),
    "dfd_layernorm_bwd": (c_int, [c_int, P, P, P, P, P, P, P, c_int, _PI, c_long, c_int, P]),
    "dfd_copy_rows": (c_int, [c_int, P, P, P, P, c_long, c_int, P]),
    "dfd_add_rowtable": (c_int, [c_int, P, P, P, c_long, c_int, c_int, P]),
    "dfd_rowtable_grad_ws": (c_size_t, [c_int, c_int]),
    "dfd_rowtable_grad": (c_int, [c_int, P, P, c_long, c_int, c_int, c_int, P, c_size_t, P]),
    "dfd_avgpool_fwd": (c_int, [c_int, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_avgpool_bwd": (c_int, [c_int, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_relpos_bias_fwd": (c_int, [P, P, P, c_int, c_int, c_int, P]),
    "dfd_relpos_bias_bwd": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P]),
    "dfd_axpby": (c_int, [P, P, c_float, c_float, P, P, c_long, P]),
    "dfd_add": (c_int, [c_int, P, P, P, c_long, P]),
    "dfd_rand": (c_int, [P, c_uint32, c_float, P, c_long, P]),
    "dfd_step_tick": (c_int, [P, c_int, P, P]),
    "dfd_mx_quant_weights_multi": (c_int, [P, c_int, P]),
    "dfd_mx_quant_rows": (c_int, [c_int, P, POINTER(Prologue), P, P, c_long, c_int, P]),
    "dfd_mx_gemm": (c_int, [P, P, P, P, c_int, P, c_long, c_int, c_int, P]),
    "dfd_wattn_parts": (c_int, [c_int]),
    "dfd_wattn_fwd": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_float, P]),
    "dfd_wattn_bwd": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, P]),
    "dfd_attn_scores": (c_int, [P, P, P, P, c_float, c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_attn_apply": (c_int, [P, c_int, P, P, c_float, c_int, c_int, c_int, c_int, c_int, P]),
    "dfd_coord_mlp_fwd_multi": (c_int, [P, c_int, P]),
    "dfd_coord_mlp_bwd_multi": (c_int, [P, c_int, P]),
    "dfd_relpos_bias_fwd_multi": (c_int, [P, c_int, P]),
    "dfd_relpos_bias_bwd_multi": (c_int, [P, c_int, P]),
}

class BnEvalJob(Structure):
    """dfd_bn_eval_job"""
    _fields_ = [("gamma", c_void_p), ("beta", c_void_p), ("conv_bias", c_void_p), ("ls", c_void_p), ("running_mean", c_void_p),
                ("running_var", c_void_p), ("bnstate", c_void_p), ("eps", c_float), ("C", c_int)]


class MxJob(Structure):
    """struct dfd_mx_job (include/dfd_hip.h)."""

    _fields_ = [("src", c_void_p), ("q", c_void_p), ("scale", c_void_p), ("kn", c_void_p), ("N", c_int), ("K", c_int),
                ("kn_dtype", c_int), ("_pad", c_int)]


class CmlpJob(Structure):
    """struct dfd_cmlp_job (include/dfd_hip.h)."""

    _fields_ = [(n, c_void_p) for n in ("coords", "w0", "b0", "w2", "table", "dtable", "dw0", "db0", "dw2")] + \
               [(n, c_int) for n in ("T", "D", "Hd", "_pad")]


class RelposJob(Structure):
    """struct dfd_relpos_job (include/dfd_hip.h)."""

    _fields_ = [(n, c_void_p) for n in ("table", "idx", "full", "dfull", "dtable")] + [(n, c_int) for n in ("H", "T", "n_local", "n_global")]


class PrepJob(Structure):
    """struct dfd_prep_job (include/dfd_hip.h)."""

    _fields_ = [("src", c_void_p), ("nk", c_void_p), ("kn", c_void_p), ("N", c_int), ("K", c_int), ("dtype", c_int),
                ("_pad", c_int)]


_lib: ctypes.CDLL | None = None


def load() -> ctypes.CDLL:
    """Load libdfd_hip.so and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its bundled HIP runtime must be the one this process uses.  If libdfd_hip.so is
    # dlopen'ed before torch, the loader resolves libamdhip64 to the system copy, torch then brings its
    # own, and every launch on a torch stream fails (two runtimes, foreign stream handles).
    import torch  # noqa: F401

    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m deepfakedetection_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise RuntimeError(f"libdfd_hip.so does not export {name}") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(code: int, op: str, detail: str = "") -> None:
    if code != DFD_OK:
        raise RuntimeError(f"{op} failed with {ERRORS.get(code, code)} {detail}")


__all__ = [
    "ACT_GELU", "ACT_NONE", "ACT_RELU", "ACT_SILU", "ADAMW_HP_LEN", "ADAMW_TABLE_COLS", "BF16", "CLIP_CFG_LEN", "CLIP_CLIPPED", "CLIP_COEF",
    "CLIP_MODE_NORM", "CLIP_MODE_VALUE", "CLIP_NORM", "CLIP_NORM_MAX", "CLIP_NORM_SUM", "CLIP_SKIP", "CLIP_SKIPPED", "CLIP_STATE_LEN", "CLIP_STEPS", "EMA_COPY", "EMA_LERP", "EMA_TABLE_COLS", "F32",
    "MAX_PARTIALS", "MIX_CUTMIX", "MIX_JOB_WORDS", "MIX_KEEP", "MIX_MIXUP", "MIX_NCHW", "MIX_NHWC", "Mat", "PRO_AFFINE2", "PRO_BN_ACT", "PRO_BN_ACT_GATE", "PRO_NONE", "DwShape", "Prologue",
    "StemShape", "SIGNATURES", "check", "load", "c_int64",
]

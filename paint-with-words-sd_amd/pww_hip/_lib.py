"""ctypes binding of libpww_hip.so (the C ABI declared in include/pww_hip.h).

The library is plain HIP behind `extern "C"`; nothing here depends on torch. Loading fails LOUDLY:
there is no CPU or PyTorch fallback for the kernels (the oracle under oracle/ is test-only).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PWW_HIP_LIB", os.path.join(_HERE, "libpww_hip.so"))
# the product library compiled with -DPWW_EXPERIMENTS=1: + the forms that were measured and not made a default (include/pww_hip.h, section
# "experiments"). Tests and A/B tools load it (`load_experiments()`, or a whole process through PWW_HIP_LIB); the product never does.
EXPERIMENTS_LIB_PATH = os.environ.get("PWW_HIP_EXPERIMENTS_LIB", os.path.join(_HERE, "libpww_hip_experiments.so"))

# the side libraries (SIDE below; `load_side(name)`), each loaded on the first call that needs it:
#   long      the launches of prompts longer than 77 tokens (128 < M <= 256 keys; include/pww_hip_long.h)
#   scope     cross-attention with a per-head / per-row score statistic (M <= 128 keys; include/pww_hip_scope.h)
#   linear    linear layers with a bias / residual / GEGLU epilogue (include/pww_hip_linear.h): ops.linear
#   regions   region prompts: the region masks at latent resolution and the per-pixel blend of the noise predictions (include/pww_hip_regions.h)
LONG_LIB_PATH = os.environ.get("PWW_HIP_LONG_LIB", os.path.join(_HERE, "libpww_hip_long.so"))
SCOPE_LIB_PATH = os.environ.get("PWW_HIP_SCOPE_LIB", os.path.join(_HERE, "libpww_hip_scope.so"))
LINEAR_LIB_PATH = os.environ.get("PWW_HIP_LINEAR_LIB", os.path.join(_HERE, "libpww_hip_linear.so"))
REGIONS_LIB_PATH = os.environ.get("PWW_HIP_REGIONS_LIB", os.path.join(_HERE, "libpww_hip_regions.so"))
#   lora      unmerged LoRA adapters chosen per batch row (include/pww_hip_lora.h): ops.lora_update. Its spec is in SIDE_MORE below.
LORA_LIB_PATH = os.environ.get("PWW_HIP_LORA_LIB", os.path.join(_HERE, "libpww_hip_lora.so"))
#   convtail  conv2 of a ResnetBlock2D with the block's 1 x 1 shortcut as further K-slabs (include/pww_hip_convtail.h): ops.conv3x3_shortcut.
#             Its spec is in SIDE_CONV below.
CONVTAIL_LIB_PATH = os.environ.get("PWW_HIP_CONVTAIL_LIB", os.path.join(_HERE, "libpww_hip_convtail.so"))
#   canvas    canvases larger than the UNet's window: the gather of the windows and the combine of their noise predictions
#             (include/pww_hip_canvas.h): ops.canvas_gather, ops.canvas_combine. Its spec is in SIDE_EXTRA below.
CANVAS_LIB_PATH = os.environ.get("PWW_HIP_CANVAS_LIB", os.path.join(_HERE, "libpww_hip_canvas.so"))
#   concat    the up blocks without torch.cat: GroupNorm and conv2 + shortcut reading the two halves of the concatenation where they lie
#             (include/pww_hip_concat.h): ops.group_norm_cat, ops.conv3x3_shortcut_cat. Its spec is in SIDE_EXTRA below.
CONCAT_LIB_PATH = os.environ.get("PWW_HIP_CONCAT_LIB", os.path.join(_HERE, "libpww_hip_concat.so"))
#   hold      region strength (img2img): the strength map of a request, its feather and the per-step hold of the pixels that are not
#             released yet (include/pww_hip_hold.h): ops.hold_strength_map, ops.hold_apply. Its spec is in SIDE_EXTRA below.
HOLD_LIB_PATH = os.environ.get("PWW_HIP_HOLD_LIB", os.path.join(_HERE, "libpww_hip_hold.so"))
#   convwide  the 160-wide tile of the plain 3 x 3 convolution (csrc/pww_conv.hip compiled for that width alone: the product library is at
#             its size limit; include/pww_hip_convwide.h): ops.conv3x3 where the plan is that tile. Its spec is in SIDE_EXTRA below.
CONVWIDE_LIB_PATH = os.environ.get("PWW_HIP_CONVWIDE_LIB", os.path.join(_HERE, "libpww_hip_convwide.so"))
#   vae       the AutoencoderKL decoder: the mid block's one-head attention of head dim 512 and the tail -- conv_norm_out, SiLU, conv_out to 3
#             channels, image -- in two launches (include/pww_hip_vae.h): pww_hip.vae. Its spec is in SIDE_EXTRA below.
VAE_LIB_PATH = os.environ.get("PWW_HIP_VAE_LIB", os.path.join(_HERE, "libpww_hip_vae.so"))
#   vaeenc    the AutoencoderKL encoder: the head (image -> conv_in, 3 input channels), the downsamplers (stride 2, padding on the right and
#             bottom only: csrc/pww_conv.hip compiled for that geometry) and the tail -- conv_norm_out, SiLU, conv_out to 8 channels,
#             quant_conv, mean / logvar, the scaled latent -- in two launches (include/pww_hip_vaeenc.h): pww_hip.vae_encode. Its spec is in
#             SIDE_EXTRA below.
VAEENC_LIB_PATH = os.environ.get("PWW_HIP_VAEENC_LIB", os.path.join(_HERE, "libpww_hip_vaeenc.so"))
#   text      the CLIP text encoder: the embedding gather with layer 0's first LayerNorm, the causal self-attention of at most 128 tokens with
#             head dim 64, and QuickGELU / GELU in place (include/pww_hip_text.h): pww_hip.text_encode. Its spec is in SIDE_EXTRA below.
TEXT_LIB_PATH = os.environ.get("PWW_HIP_TEXT_LIB", os.path.join(_HERE, "libpww_hip_text.so"))
#   control   the residuals of a ControlNet: its 1 x 1 zero convolutions, the conditioning scale and the add into the UNet's skip tensors and
#             mid-block output as ONE grouped GEMM (include/pww_hip_control.h): ops.control_residuals. Its spec is in SIDE_EXTRA below.
CONTROL_LIB_PATH = os.environ.get("PWW_HIP_CONTROL_LIB", os.path.join(_HERE, "libpww_hip_control.so"))
#   step      one sampler step as ONE elementwise launch: the guidance combine, the scheduler's affine update (Euler, Euler ancestral, DDIM,
#             DPM-Solver++ 2M: seven numbers per step), the history write and the next UNet input (include/pww_hip_step.h): ops.sched_step.
#             Its spec is in SIDE_EXTRA below.
STEP_LIB_PATH = os.environ.get("PWW_HIP_STEP_LIB", os.path.join(_HERE, "libpww_hip_step.so"))

PWW_OK, PWW_EINVAL, PWW_ENOTSUP, PWW_EHIP = 0, -22, -95, -5
MIN_VERSION = 127        # oldest libpww_hip ABI (pww_version(): major * 100 + minor) this package drives
DTYPE_F16, DTYPE_BF16 = 0, 1
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1
ACT_NONE, ACT_SILU = 0, 1
LINEAR_NONE, LINEAR_BIAS, LINEAR_BIAS_RESIDUAL, LINEAR_BIAS_GEGLU = 0, 1, 2, 3
MAX_HEAD_DIM = 160

# every symbol include/pww_hip.h declares for libpww_hip.so (tests check the library exports all of them) ...
EXPORTS = ("pww_version", "pww_has_experiments", "pww_last_error", "pww_device_arch", "pww_self_attn_fwd", "pww_cross_attn_fwd",
           "pww_cross_attn_fwd_stat", "pww_cross_attn_fwd_stat_ex",
           "pww_qk_reduce", "pww_mask_build", "pww_mask_build_rgb", "pww_mask_build_f32", "pww_resize_tokens", "pww_gauss_blur", "pww_inpaint_prep", "pww_cfg_combine", "pww_store_f32",
           "pww_workspace_bytes", "pww_profile_arm", "pww_profile_elapsed_us", "pww_profile_reset", "pww_debug_timeline", "pww_debug_path_counts",
           "pww_debug_last_attn_route",
           "pww_qproj_stat", "pww_qproj_parts", "pww_cross_attn_fwd_parts", "pww_mask_build_f32_levels", "pww_qk_parts", "pww_qk_parts_count",
           "pww_group_norm_fwd", "pww_group_norm_workspace_bytes", "pww_add_layer_norm", "pww_add_layer_norm_bias", "pww_geglu", "pww_bias_residual",
           "pww_conv3x3_workspace_bytes", "pww_conv3x3_fwd", "pww_cross_attn_probs")
# ... and what only libpww_hip_experiments.so has on top of them (the header's "experiments" section)
EXPERIMENT_EXPORTS = ("pww_cross_attn_fwd_fused", "pww_cross_attn_fwd_fused_ex", "pww_cross_fused_workspace_bytes", "pww_cross_fused_state_bytes",
                      "pww_cross_attn_fwd_parts_out", "pww_cross_attn_out_supported")


# every symbol include/pww_hip_long.h declares for libpww_hip_long.so
LONG_EXPORTS = ("pww_long_version", "pww_long_last_error", "pww_long_qk_parts", "pww_long_qk_parts_count", "pww_long_cross_attn_fwd_parts",
                "pww_long_cross_attn_probs", "pww_long_profile_arm", "pww_long_profile_elapsed_us")
LONG_MIN_VERSION = 100
LONG_MIN_KEYS, LONG_MAX_KEYS = 129, 256


# every symbol include/pww_hip_scope.h declares for libpww_hip_scope.so
SCOPE_EXPORTS = ("pww_scope_version", "pww_scope_last_error", "pww_scope_head_parts_count", "pww_scope_head_parts", "pww_scope_cross_attn_fwd")
SCOPE_MIN_VERSION = 100
SCOPE_HEAD, SCOPE_ROW = 1, 2


# every symbol include/pww_hip_linear.h declares for libpww_hip_linear.so
LINEAR_EXPORTS = ("pww_linear_version", "pww_linear_last_error", "pww_linear_workspace_bytes", "pww_linear_fwd")
LINEAR_MIN_VERSION = 100


# every symbol include/pww_hip_regions.h declares for libpww_hip_regions.so
REGIONS_EXPORTS = ("pww_regions_version", "pww_regions_last_error", "pww_regions_masks", "pww_regions_combine")
REGIONS_MIN_VERSION = 100
REGIONS_MAX, REGIONS_MAX_PLANE, REGIONS_MAX_FEATHER = 8, 9216, 8.0      # PWW_REGIONS_MAX* of the header


# every symbol include/pww_hip_lora.h declares for libpww_hip_lora.so
LORA_EXPORTS = ("pww_lora_version", "pww_lora_last_error", "pww_lora_fwd")
LORA_MIN_VERSION = 100
LORA_MAX_ADAPTERS, LORA_MAX_RANK, LORA_MAX_SEGMENTS = 8, 128, 3      # PWW_LORA_MAX_* of the header


# every symbol include/pww_hip_convtail.h declares for libpww_hip_convtail.so
CONVTAIL_EXPORTS = ("pww_convtail_version", "pww_convtail_last_error", "pww_convtail_workspace_bytes", "pww_convtail_fwd")
CONVTAIL_MIN_VERSION = 100


# every symbol include/pww_hip_canvas.h declares for libpww_hip_canvas.so
CANVAS_EXPORTS = ("pww_canvas_version", "pww_canvas_last_error", "pww_canvas_gather", "pww_canvas_combine")
CANVAS_MIN_VERSION = 100
CANVAS_MAX_WINDOWS, CANVAS_MAX_RAMP, CANVAS_MIN_WINDOW, CANVAS_MAX_WINDOW = 64, 64, 8, 128      # PWW_CANVAS_* of the header


# every symbol include/pww_hip_concat.h declares for libpww_hip_concat.so
CONCAT_EXPORTS = ("pww_concat_version", "pww_concat_last_error", "pww_concat_group_norm_workspace_bytes", "pww_concat_group_norm_fwd",
                  "pww_concat_convtail_workspace_bytes", "pww_concat_convtail_fwd")
CONCAT_MIN_VERSION = 100


# every symbol include/pww_hip_hold.h declares for libpww_hip_hold.so
HOLD_EXPORTS = ("pww_hold_version", "pww_hold_last_error", "pww_hold_strength_map", "pww_hold_feather", "pww_hold_apply", "pww_hold_taps",
                "pww_hold_thresholds")
HOLD_MIN_VERSION = 100
HOLD_MAX_COLORS, HOLD_MAX_FEATHER, HOLD_MAX_RADIUS, HOLD_MAX_STEPS = 8, 8.0, 24, 100000      # PWW_HOLD_MAX_* of the header


# every symbol include/pww_hip_convwide.h declares for libpww_hip_convwide.so
CONVWIDE_EXPORTS = ("pww_convwide_version", "pww_convwide_last_error", "pww_convwide_takes", "pww_convwide_workspace_bytes", "pww_convwide_fwd")
CONVWIDE_MIN_VERSION = 100


# every symbol include/pww_hip_vae.h declares for libpww_hip_vae.so
VAE_EXPORTS = ("pww_vae_version", "pww_vae_last_error", "pww_vae_attn_fwd", "pww_vae_tail_workspace_bytes", "pww_vae_tail_chunks", "pww_vae_tail_stats",
               "pww_vae_tail_fwd")
VAE_MIN_VERSION = 100
VAE_HEAD_DIM, VAE_TAIL_CHANNELS, VAE_TAIL_GROUPS, VAE_TAIL_MAX_CHUNKS = 512, 128, 32, 64      # PWW_VAE_* of the header
VAE_OUT_SAMPLE, VAE_OUT_UINT8 = 0, 1


# every symbol include/pww_hip_vaeenc.h declares for libpww_hip_vaeenc.so
VAEENC_EXPORTS = ("pww_vaeenc_version", "pww_vaeenc_last_error", "pww_vaeenc_head_fwd", "pww_vaeenc_down_workspace_bytes", "pww_vaeenc_down_fwd",
                  "pww_vaeenc_tail_workspace_bytes", "pww_vaeenc_tail_chunks", "pww_vaeenc_tail_stats", "pww_vaeenc_tail_fwd")
VAEENC_MIN_VERSION = 100
VAEENC_HEAD_CHANNELS, VAEENC_TAIL_CHANNELS, VAEENC_TAIL_GROUPS, VAEENC_TAIL_MAX_CHUNKS = 128, 512, 32, 64      # PWW_VAEENC_* of the header
VAEENC_IN_SAMPLE, VAEENC_IN_UINT8 = 0, 1


# every symbol include/pww_hip_text.h declares for libpww_hip_text.so
TEXT_EXPORTS = ("pww_text_version", "pww_text_last_error", "pww_text_embed_ln", "pww_text_attn_fwd", "pww_text_act")
TEXT_MIN_VERSION = 100
TEXT_HEAD_DIM, TEXT_MAX_TOKENS, TEXT_MAX_WIDTH = 64, 128, 4096      # PWW_TEXT_* of the header
TEXT_ACT_QUICK_GELU, TEXT_ACT_GELU = 0, 1


# every symbol include/pww_hip_control.h declares for libpww_hip_control.so
CONTROL_EXPORTS = ("pww_control_version", "pww_control_last_error", "pww_control_fwd", "pww_control_plan")
CONTROL_MIN_VERSION = 100
CONTROL_MAX_PROBLEMS, CONTROL_TILE_M, CONTROL_TILE_N = 16, 128, 64      # PWW_CONTROL_* of the header


# every symbol include/pww_hip_step.h declares for libpww_hip_step.so
STEP_EXPORTS = ("pww_step_version", "pww_step_last_error", "pww_step_fwd")
STEP_MIN_VERSION = 100
STEP_SRC_F32, STEP_ROW = 2, 7      # PWW_STEP_* of the header


class AttnDesc(ctypes.Structure):
    """struct pww_attn_desc (include/pww_hip.h)."""
    _fields_ = [("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("N", ctypes.c_int32),
                ("M", ctypes.c_int32), ("D", ctypes.c_int32),
                ("q_stride", ctypes.c_int64 * 3), ("k_stride", ctypes.c_int64 * 3),
                ("v_stride", ctypes.c_int64 * 3), ("o_stride", ctypes.c_int64 * 3),
                ("scale", ctypes.c_float), ("bias_stride", ctypes.c_int64 * 4)]


class CrossOpts(ctypes.Structure):
    """struct pww_cross_opts (optional arguments of the *_ex cross-attention entry points)."""
    _fields_ = [("size", ctypes.c_uint32), ("bias_cols", ctypes.c_int32), ("coeff_scalar_dev", ctypes.c_void_p),
                ("bias_compact", ctypes.c_void_p), ("col_idx", ctypes.c_void_p), ("R", ctypes.c_int32), ("gated_images", ctypes.c_int32),
                ("compact_stride", ctypes.c_int64 * 2), ("col_idx_stride", ctypes.c_int64)]


class QprojDesc(ctypes.Structure):
    """struct pww_qproj_desc (query projection + score-statistic partials)."""
    _fields_ = [("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("N", ctypes.c_int32), ("Cin", ctypes.c_int32), ("H", ctypes.c_int32),
                ("D", ctypes.c_int32), ("M", ctypes.c_int32), ("x_stride", ctypes.c_int64 * 2), ("q_stride", ctypes.c_int64 * 2),
                ("k_stride", ctypes.c_int64 * 2)]


class GnDesc(ctypes.Structure):
    """struct pww_gn_desc (GroupNorm + addend + activation)."""
    _fields_ = [("dtype", ctypes.c_int32), ("layout", ctypes.c_int32), ("B", ctypes.c_int32), ("C", ctypes.c_int32), ("HW", ctypes.c_int32),
                ("G", ctypes.c_int32), ("eps", ctypes.c_float), ("act", ctypes.c_int32), ("add_stride", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class LnDesc(ctypes.Structure):
    """struct pww_ln_desc (add + LayerNorm)."""
    _fields_ = [("dtype", ctypes.c_int32), ("C", ctypes.c_int32), ("rows", ctypes.c_int64), ("a_stride", ctypes.c_int64), ("x_stride", ctypes.c_int64),
                ("s_stride", ctypes.c_int64), ("y_stride", ctypes.c_int64), ("eps", ctypes.c_float), ("_pad", ctypes.c_int32)]


class ConvDesc(ctypes.Structure):
    """struct pww_conv_desc (3 x 3 convolution over NHWC tensors; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("Hin", ctypes.c_int32), ("Win", ctypes.c_int32),
                ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32), ("stride", ctypes.c_int32), ("upsample", ctypes.c_int32), ("tile_n", ctypes.c_int32),
                ("splitk", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class LinearDesc(ctypes.Structure):
    """struct pww_linear_desc (linear layer with a bias / residual / GEGLU epilogue; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
                ("epilogue", ctypes.c_int32), ("x_stride", ctypes.c_int64), ("y_stride", ctypes.c_int64), ("r_stride", ctypes.c_int64),
                ("tile_n", ctypes.c_int32), ("splitk", ctypes.c_int32)]


class ProbsDesc(ctypes.Structure):
    """struct pww_probs_desc (head-averaged cross-attention probabilities; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("images", ctypes.c_int32), ("accumulate", ctypes.c_int32), ("weight", ctypes.c_float),
                ("out_stride", ctypes.c_int64 * 2)]


class LoraDesc(ctypes.Structure):
    """struct pww_lora_desc (per-row low-rank update; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("R", ctypes.c_int32), ("T", ctypes.c_int32), ("K", ctypes.c_int32),
                ("N", ctypes.c_int32), ("n_seg", ctypes.c_int32), ("rank", ctypes.c_int32), ("n_adapters", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("x_row_stride", ctypes.c_int64), ("x_tok_stride", ctypes.c_int64), ("y_row_stride", ctypes.c_int64), ("y_tok_stride", ctypes.c_int64)]


class ConvTailDesc(ctypes.Structure):
    """struct pww_convtail_desc (3 x 3 convolution + 1 x 1 shortcut as one implicit GEMM; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("Cin", ctypes.c_int32), ("C2", ctypes.c_int32), ("Cout", ctypes.c_int32), ("tile_n", ctypes.c_int32), ("splitk", ctypes.c_int32)]


class ConcatGnDesc(ctypes.Structure):
    """struct pww_concat_gn_desc (GroupNorm over two channels_last tensors laid end to end; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("C1", ctypes.c_int32), ("C2", ctypes.c_int32),
                ("HW", ctypes.c_int32), ("G", ctypes.c_int32), ("eps", ctypes.c_float), ("act", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class ConcatTailDesc(ctypes.Structure):
    """struct pww_concat_tail_desc (pww_convtail_desc with the shortcut's input in two parts; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("Cin", ctypes.c_int32), ("C1", ctypes.c_int32), ("C2", ctypes.c_int32), ("Cout", ctypes.c_int32), ("tile_n", ctypes.c_int32),
                ("splitk", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class VaeAttnDesc(ctypes.Structure):
    """struct pww_vae_attn_desc (one-head attention of head dim 512; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("N", ctypes.c_int32), ("D", ctypes.c_int32),
                ("scale", ctypes.c_float), ("q_batch_stride", ctypes.c_int64), ("q_row_stride", ctypes.c_int64), ("k_batch_stride", ctypes.c_int64),
                ("k_row_stride", ctypes.c_int64), ("v_batch_stride", ctypes.c_int64), ("v_row_stride", ctypes.c_int64),
                ("o_batch_stride", ctypes.c_int64), ("o_row_stride", ctypes.c_int64)]


class VaeTailDesc(ctypes.Structure):
    """struct pww_vae_tail_desc (GroupNorm + SiLU + 3 x 3 convolution to 3 channels + image; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("C", ctypes.c_int32), ("out", ctypes.c_int32), ("eps", ctypes.c_float)]


class VaeEncHeadDesc(ctypes.Structure):
    """struct pww_vaeenc_head_desc (image -> conv_in, channels_last; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("form", ctypes.c_int32)]


class VaeEncDownDesc(ctypes.Structure):
    """struct pww_vaeenc_down_desc (3 x 3 convolution, stride 2, padding on the right and bottom only; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32), ("tile_n", ctypes.c_int32), ("splitk", ctypes.c_int32)]


class VaeEncTailDesc(ctypes.Structure):
    """struct pww_vaeenc_tail_desc (GroupNorm + SiLU + conv to 8 channels + quant_conv + latent; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("C", ctypes.c_int32), ("eps", ctypes.c_float), ("scale", ctypes.c_float)]


class ControlProblem(ctypes.Structure):
    """struct pww_control_problem (one GEMM of the grouped launch: a zero convolution, its skip and its output)."""
    _fields_ = [("h", ctypes.c_void_p), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("skip", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("h_stride", ctypes.c_int64), ("skip_stride", ctypes.c_int64), ("out_stride", ctypes.c_int64)]


class ControlDesc(ctypes.Structure):
    """struct pww_control_desc (the grouped launch; size-prefixed)."""
    _fields_ = [("size", ctypes.c_uint32), ("dtype", ctypes.c_int32), ("n", ctypes.c_int32), ("scale_index", ctypes.c_int32)]


class Region(ctypes.Structure):
    """struct pww_region."""
    _fields_ = [("r", ctypes.c_uint8), ("g", ctypes.c_uint8), ("b", ctypes.c_uint8), ("_pad", ctypes.c_uint8),
                ("strength", ctypes.c_float)]


class PwwHipError(RuntimeError):
    pass


_lib = None
_exp = None


def _bind(lib, experiments):
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.pww_version.restype = ctypes.c_int
    # first of all: an older library lacks symbols that are bound below, and has to end here with the rebuild hint
    if lib.pww_version() // 100 != 1 or lib.pww_version() < MIN_VERSION:
        raise PwwHipError("libpww_hip ABI version %d.%02d is not 1.x >= 1.%02d (rebuild: python paint-with-words-sd_amd/build.py)"
                          % (lib.pww_version() // 100, lib.pww_version() % 100, MIN_VERSION % 100))
    lib.pww_last_error.restype = ctypes.c_char_p
    lib.pww_device_arch.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    lib.pww_self_attn_fwd.argtypes = [vp, vp, vp, vp, ctypes.POINTER(AttnDesc), vp]
    lib.pww_cross_attn_fwd.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.POINTER(AttnDesc), vp]
    lib.pww_cross_attn_fwd_stat.argtypes = [vp, vp, vp, vp, vp, vp, i32, ctypes.c_double, f32, vp, ctypes.POINTER(AttnDesc), vp]
    lib.pww_cross_attn_fwd_stat_ex.argtypes = [vp, vp, vp, vp, vp, vp, i32, ctypes.c_double, f32, vp, ctypes.POINTER(AttnDesc),
                                               ctypes.POINTER(CrossOpts), vp]
    lib.pww_qproj_stat.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(QprojDesc), i32, vp, ctypes.c_size_t, vp]
    lib.pww_qproj_stat.restype = ctypes.c_int
    lib.pww_qproj_parts.argtypes = [ctypes.POINTER(QprojDesc)]
    lib.pww_qproj_parts.restype = ctypes.c_int32
    lib.pww_cross_attn_fwd_parts.argtypes = [vp, vp, vp, vp, vp, i32, f32, vp, ctypes.POINTER(AttnDesc), vp, i32, vp, ctypes.POINTER(CrossOpts), vp]
    lib.pww_cross_attn_fwd_parts.restype = ctypes.c_int
    lib.pww_qk_parts.argtypes = [vp, vp, vp, ctypes.POINTER(AttnDesc), i32, i32, vp, ctypes.c_size_t, vp]
    lib.pww_qk_parts.restype = ctypes.c_int
    lib.pww_qk_parts_count.argtypes = [ctypes.POINTER(AttnDesc)]
    lib.pww_qk_parts_count.restype = ctypes.c_int32
    lib.pww_mask_build_f32_levels.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.pww_mask_build_f32_levels.restype = ctypes.c_int
    lib.pww_group_norm_workspace_bytes.argtypes = [ctypes.POINTER(GnDesc)]
    lib.pww_group_norm_workspace_bytes.restype = ctypes.c_size_t
    lib.pww_group_norm_fwd.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.POINTER(GnDesc), vp, ctypes.c_size_t, vp]
    lib.pww_group_norm_fwd.restype = ctypes.c_int
    lib.pww_add_layer_norm.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.POINTER(LnDesc), vp]
    lib.pww_add_layer_norm.restype = ctypes.c_int
    lib.pww_add_layer_norm_bias.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(LnDesc), vp]
    lib.pww_add_layer_norm_bias.restype = ctypes.c_int
    lib.pww_geglu.argtypes = [vp, vp, ctypes.c_int64, i32, ctypes.c_int64, ctypes.c_int64, i32, vp]
    lib.pww_geglu.restype = ctypes.c_int
    lib.pww_bias_residual.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.pww_bias_residual.restype = ctypes.c_int
    lib.pww_conv3x3_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc)]
    lib.pww_conv3x3_workspace_bytes.restype = ctypes.c_size_t
    lib.pww_conv3x3_fwd.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(ConvDesc), vp, ctypes.c_size_t, vp]
    lib.pww_conv3x3_fwd.restype = ctypes.c_int
    lib.pww_cross_attn_probs.argtypes = [vp, vp, vp, vp, i32, ctypes.c_double, f32, vp, ctypes.POINTER(AttnDesc), ctypes.POINTER(CrossOpts), vp,
                                         ctypes.POINTER(ProbsDesc), vp]
    lib.pww_cross_attn_probs.restype = ctypes.c_int
    lib.pww_debug_timeline.argtypes = [vp, ctypes.c_size_t]
    lib.pww_debug_timeline.restype = None
    lib.pww_debug_path_counts.argtypes = [vp]
    lib.pww_debug_path_counts.restype = None
    lib.pww_debug_last_attn_route.argtypes = [ctypes.POINTER(i32), ctypes.c_int]
    lib.pww_debug_last_attn_route.restype = ctypes.c_int
    lib.pww_qk_reduce.argtypes = [vp, vp, ctypes.POINTER(AttnDesc), vp, vp, ctypes.c_size_t, vp]
    lib.pww_mask_build.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.pww_mask_build_rgb.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp]
    lib.pww_mask_build_f32.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, vp, vp]
    lib.pww_resize_tokens.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.pww_gauss_blur.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
    lib.pww_inpaint_prep.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.pww_cfg_combine.argtypes = [vp, vp, f32, vp, i64, i32, vp]
    lib.pww_store_f32.argtypes = [vp, ctypes.POINTER(ctypes.c_float), i32, vp]
    lib.pww_store_f32.restype = ctypes.c_int
    lib.pww_workspace_bytes.argtypes = [ctypes.POINTER(AttnDesc)]
    lib.pww_workspace_bytes.restype = ctypes.c_size_t
    lib.pww_profile_arm.argtypes = []
    lib.pww_profile_arm.restype = ctypes.c_int
    lib.pww_profile_elapsed_us.argtypes = [i32, ctypes.POINTER(ctypes.c_float)]
    lib.pww_profile_elapsed_us.restype = ctypes.c_int
    lib.pww_profile_reset.argtypes = []
    lib.pww_profile_reset.restype = None
    for name in ("pww_device_arch", "pww_self_attn_fwd", "pww_cross_attn_fwd", "pww_cross_attn_fwd_stat", "pww_cross_attn_fwd_stat_ex", "pww_qk_reduce",
                 "pww_mask_build", "pww_mask_build_rgb", "pww_mask_build_f32", "pww_resize_tokens", "pww_gauss_blur", "pww_inpaint_prep", "pww_cfg_combine"):
        getattr(lib, name).restype = ctypes.c_int
    lib.pww_has_experiments.restype = ctypes.c_int
    if experiments:
        lib.pww_cross_attn_fwd_fused.argtypes = [vp, vp, vp, vp, vp, i32, f32, vp, ctypes.POINTER(AttnDesc), vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
        lib.pww_cross_attn_fwd_fused_ex.argtypes = [vp, vp, vp, vp, vp, i32, f32, vp, ctypes.POINTER(AttnDesc), vp, vp, ctypes.c_size_t, vp,
                                                    ctypes.c_size_t, ctypes.POINTER(CrossOpts), vp]
        lib.pww_cross_attn_fwd_fused.restype = lib.pww_cross_attn_fwd_fused_ex.restype = ctypes.c_int
        lib.pww_cross_fused_workspace_bytes.argtypes = [ctypes.POINTER(AttnDesc)]
        lib.pww_cross_fused_workspace_bytes.restype = ctypes.c_size_t
        lib.pww_cross_fused_state_bytes.argtypes = [ctypes.POINTER(AttnDesc)]
        lib.pww_cross_fused_state_bytes.restype = ctypes.c_size_t
        lib.pww_cross_attn_fwd_parts_out.argtypes = [vp, vp, vp, vp, vp, i32, f32, vp, ctypes.POINTER(AttnDesc), vp, i32, vp, ctypes.POINTER(CrossOpts),
                                                     vp, vp, vp, ctypes.POINTER(ctypes.c_int64), vp]
        lib.pww_cross_attn_fwd_parts_out.restype = ctypes.c_int
        lib.pww_cross_attn_out_supported.argtypes = [ctypes.POINTER(AttnDesc), ctypes.c_int32, ctypes.c_int32]
        lib.pww_cross_attn_out_supported.restype = ctypes.c_int32
    return lib


def load():
    """Load libpww_hip.so once; raise PwwHipError with build instructions if it is missing. (PWW_HIP_LIB may point a whole process at
    libpww_hip_experiments.so: the same ABI plus the experiments section.)"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise PwwHipError(
            "libpww_hip.so not found at %s. Build it with `python paint-with-words-sd_amd/build.py` "
            "(or __graft_entry__.build()). There is no CPU/PyTorch fallback for the PwW kernels." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    # (a library from before pww_has_experiments -- an int function, ctypes' default -- is too old: _bind's version check says so)
    _lib = _bind(lib, hasattr(lib, "pww_has_experiments") and bool(lib.pww_has_experiments()))
    return _lib


def has_experiments():
    """True if the library `load()` returns carries the experiments section (a process started with PWW_HIP_LIB=...experiments.so)."""
    return bool(load().pww_has_experiments())


def load_experiments():
    """libpww_hip_experiments.so (test / tool infrastructure: the statistic formed inside the attention launch, the attention + to_out launch, the A/B kernels
    behind PWW_DEBUG). The product never calls this; a missing library raises with the build command."""
    global _exp
    if _exp is not None:
        return _exp
    if has_experiments():
        _exp = load()
        return _exp
    if not os.path.isfile(EXPERIMENTS_LIB_PATH):
        raise PwwHipError("libpww_hip_experiments.so not found at %s: this entry point is not part of the product library. Build it with "
                          "`python paint-with-words-sd_amd/build.py --experiments` (tests: the `experiments_lib` fixture does)." % EXPERIMENTS_LIB_PATH)
    lib = ctypes.CDLL(EXPERIMENTS_LIB_PATH)
    lib.pww_has_experiments.restype = ctypes.c_int
    if not lib.pww_has_experiments():
        raise PwwHipError("%s was not built with -DPWW_EXPERIMENTS=1" % EXPERIMENTS_LIB_PATH)
    _exp = _bind(lib, True)
    return _exp


# ---- the side libraries: libpww_hip_<name>.so behind include/pww_hip_<name>.h, each loaded on the first call that needs it --------------
_P = ctypes.POINTER
_vp, _i32, _i64, _f32, _f64, _sz, _int = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_int
_HINT = "(rebuild: python paint-with-words-sd_amd/build.py, or __graft_entry__.build())"
# name -> path: the module attribute that holds the file's path (read per call: PWW_HIP_<NAME>_LIB sets it, tests patch it)
#         exports / min_version: every symbol the header declares, the oldest ABI (pww_<name>_version()) this package drives
#         missing_ok: a missing file returns None (the caller has another route that computes the same thing) instead of raising
#         needs: what cannot run without the library (error text)
#         sigs: entry point -> (argtypes, restype); pww_<name>_version and pww_<name>_last_error are bound by load_side itself
SIDE = {
    "long": dict(path="LONG_LIB_PATH", exports=LONG_EXPORTS, min_version=LONG_MIN_VERSION, missing_ok=False, needs="prompts longer than 77 tokens need it", sigs={
        "pww_long_qk_parts": ([_vp, _vp, _vp, _P(AttnDesc), _i32, _i32, _vp, _sz, _vp], _int),
        "pww_long_qk_parts_count": ([_P(AttnDesc)], _i32),
        "pww_long_cross_attn_fwd_parts": ([_vp, _vp, _vp, _vp, _vp, _i32, _f32, _vp, _P(AttnDesc), _vp, _i32, _vp, _P(CrossOpts), _vp], _int),
        "pww_long_cross_attn_probs": ([_vp, _vp, _vp, _vp, _i32, _f64, _f32, _vp, _P(AttnDesc), _P(CrossOpts), _vp, _P(ProbsDesc), _vp], _int),
        "pww_long_profile_arm": ([], _int),
        "pww_long_profile_elapsed_us": ([_P(_f32)], _int)}),
    "scope": dict(path="SCOPE_LIB_PATH", exports=SCOPE_EXPORTS, min_version=SCOPE_MIN_VERSION, missing_ok=True, needs="per-head / per-row score statistics need it", sigs={
        "pww_scope_head_parts_count": ([_P(AttnDesc)], _i32),
        "pww_scope_head_parts": ([_vp, _vp, _vp, _P(AttnDesc), _i32, _vp, _sz, _vp], _int),
        "pww_scope_cross_attn_fwd": ([_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _P(AttnDesc), _vp, _i32, _vp, _P(CrossOpts), _vp], _int)}),
    "linear": dict(path="LINEAR_LIB_PATH", exports=LINEAR_EXPORTS, min_version=LINEAR_MIN_VERSION, missing_ok=False, needs="linear layers on the native kernel need it", sigs={
        "pww_linear_workspace_bytes": ([_P(LinearDesc)], _sz),
        "pww_linear_fwd": ([_vp, _vp, _vp, _vp, _vp, _P(LinearDesc), _vp, _sz, _vp], _int)}),
    "regions": dict(path="REGIONS_LIB_PATH", exports=REGIONS_EXPORTS, min_version=REGIONS_MIN_VERSION, missing_ok=False, needs="region prompts need it", sigs={
        "pww_regions_masks": ([_vp, _i32, _i32, _vp, _i32, _f32, _vp, _vp], _int),
        "pww_regions_combine": ([_vp, _vp, _vp, _vp, _f32, _vp, _i32, _i32, _i32, _i64, _i32, _vp], _int)}),
}
# the libraries that came after the four of SIDE: the same fields, the same loader
SIDE_MORE = {
    "lora": dict(path="LORA_LIB_PATH", exports=LORA_EXPORTS, min_version=LORA_MIN_VERSION, missing_ok=False, needs="LoRA adapters on the native kernel need it", sigs={
        "pww_lora_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _P(LoraDesc), _vp], _int)}),
}
# the side libraries of the convolutions (build.py: SIDE_LIBS_CONV). missing_ok: the caller keeps the 1 x 1 GEMM + conv3x3 sequence, which
# computes the same thing on this repository's own kernel
SIDE_CONV = {
    "convtail": dict(path="CONVTAIL_LIB_PATH", exports=CONVTAIL_EXPORTS, min_version=CONVTAIL_MIN_VERSION, missing_ok=True, needs="conv2 with the shortcut as K-slabs needs it", sigs={
        "pww_convtail_workspace_bytes": ([_P(ConvTailDesc)], _sz),
        "pww_convtail_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(ConvTailDesc), _vp, _sz, _vp], _int)}),
}
# the open-ended table (build.py: SIDE_LIBS_EXTRA): SIDE, SIDE_MORE and SIDE_CONV are closed, and every later side library is a row here
SIDE_EXTRA = {
    "canvas": dict(path="CANVAS_LIB_PATH", exports=CANVAS_EXPORTS, min_version=CANVAS_MIN_VERSION, missing_ok=False, needs="canvases larger than the window need it", sigs={
        "pww_canvas_gather": ([_vp, _vp, _P(_i32), _i32, _P(_i32), _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp], _int),
        "pww_canvas_combine": ([_vp, _vp, _vp, _vp, _f32, _vp, _P(_i32), _i32, _P(_i32), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp], _int)}),
    # missing_ok: the caller materialises torch.cat and runs the one-source ops, which compute the same bits
    "concat": dict(path="CONCAT_LIB_PATH", exports=CONCAT_EXPORTS, min_version=CONCAT_MIN_VERSION, missing_ok=True, needs="the up blocks without torch.cat need it", sigs={
        "pww_concat_group_norm_workspace_bytes": ([_P(ConcatGnDesc)], _sz),
        "pww_concat_group_norm_fwd": ([_vp, _vp, _vp, _vp, _vp, _P(ConcatGnDesc), _vp, _sz, _vp], _int),
        "pww_concat_convtail_workspace_bytes": ([_P(ConcatTailDesc)], _sz),
        "pww_concat_convtail_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(ConcatTailDesc), _vp, _sz, _vp], _int)}),
    "hold": dict(path="HOLD_LIB_PATH", exports=HOLD_EXPORTS, min_version=HOLD_MIN_VERSION, missing_ok=False, needs="region strengths (img2img) need it", sigs={
        "pww_hold_strength_map": ([_vp, _P(ctypes.c_uint8), _P(_f32), _f32, _vp, _i32, _i32, _i32, _vp], _int),
        "pww_hold_feather": ([_vp, _vp, _vp, _i32, _i32, _f32, _vp], _int),
        "pww_hold_apply": ([_vp, _vp, _vp, _vp, _f32, _f32, _f32, _i32, _i32, _i64, _vp], _int),
        "pww_hold_taps": ([_f32, _P(_f32), _i32], _int),
        "pww_hold_thresholds": ([_i32, _P(_f32)], _int)}),
    # required: the measured table plans the 160-wide tile for most of the SD1.5 UNet's convolutions at 2 rows, and the product library has
    # no code object for it -- there is no other implementation to fall back to
    "convwide": dict(path="CONVWIDE_LIB_PATH", exports=CONVWIDE_EXPORTS, min_version=CONVWIDE_MIN_VERSION, missing_ok=False, needs="the 160-wide tile of conv3x3 needs it", sigs={
        "pww_convwide_takes": ([_P(ConvDesc)], _int),
        "pww_convwide_workspace_bytes": ([_P(ConvDesc)], _sz),
        "pww_convwide_fwd": ([_vp, _vp, _vp, _vp, _vp, _P(ConvDesc), _vp, _sz, _vp], _int)}),
    # required where the plug runs (pww_hip/vae.py): PWW_VAE_ATTN=0 / PWW_VAE_TAIL=0 choose the stock sequences, a missing file does not
    "vae": dict(path="VAE_LIB_PATH", exports=VAE_EXPORTS, min_version=VAE_MIN_VERSION, missing_ok=False, needs="the AutoencoderKL decoder's attention and tail need it", sigs={
        "pww_vae_attn_fwd": ([_vp, _vp, _vp, _vp, _P(VaeAttnDesc), _vp], _int),
        "pww_vae_tail_workspace_bytes": ([_P(VaeTailDesc)], _sz),
        "pww_vae_tail_chunks": ([_P(VaeTailDesc)], _int),
        "pww_vae_tail_stats": ([_vp, _vp, _P(VaeTailDesc), _vp, _sz, _vp], _int),
        "pww_vae_tail_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _P(VaeTailDesc), _vp, _sz, _vp], _int)}),
    # required where the plug runs (pww_hip/vae_encode.py): PWW_VAE_ENC_HEAD=0 / _DOWN=0 / _TAIL=0 choose the stock sequences, a missing file does not
    "vaeenc": dict(path="VAEENC_LIB_PATH", exports=VAEENC_EXPORTS, min_version=VAEENC_MIN_VERSION, missing_ok=False, needs="the AutoencoderKL encoder's head, downsamplers and tail need it", sigs={
        "pww_vaeenc_head_fwd": ([_vp, _vp, _vp, _vp, _vp, _P(VaeEncHeadDesc), _vp], _int),
        "pww_vaeenc_down_workspace_bytes": ([_P(VaeEncDownDesc)], _sz),
        "pww_vaeenc_down_fwd": ([_vp, _vp, _vp, _vp, _P(VaeEncDownDesc), _vp, _sz, _vp], _int),
        "pww_vaeenc_tail_workspace_bytes": ([_P(VaeEncTailDesc)], _sz),
        "pww_vaeenc_tail_chunks": ([_P(VaeEncTailDesc)], _int),
        "pww_vaeenc_tail_stats": ([_vp, _vp, _P(VaeEncTailDesc), _vp, _sz, _vp], _int),
        "pww_vaeenc_tail_fwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(VaeEncTailDesc), _vp, _sz, _vp], _int)}),
    # missing_ok: the stock route (ops.cfg_combine, scheduler.step, scale_model_input, cat and cast) computes the same thing
    "step": dict(path="STEP_LIB_PATH", exports=STEP_EXPORTS, min_version=STEP_MIN_VERSION, missing_ok=True, needs="the fused sampler step needs it", sigs={
        "pww_step_fwd": ([_vp, _vp, _vp, _vp, _f32, _vp, _vp, _P(_f32), _i64, _i32, _i32, _i32, _vp], _int)}),
    # missing_ok: the stock route (the zero convolutions as modules, a multiplication by the scale word, the adds) computes the same thing
    "control": dict(path="CONTROL_LIB_PATH", exports=CONTROL_EXPORTS, min_version=CONTROL_MIN_VERSION, missing_ok=True, needs="the grouped ControlNet residual launch needs it", sigs={
        "pww_control_fwd": ([_P(ControlProblem), _P(ControlDesc), _vp, _vp], _int),
        "pww_control_plan": ([_P(ControlProblem), _i32, _P(_i32), _i32], _int)}),
    # required where the route runs (pww_hip/text_encode.py): PWW_TEXT_EMBED=0 / _ATTN=0 / _ACT=0 choose the stock sequences, a missing file does not
    "text": dict(path="TEXT_LIB_PATH", exports=TEXT_EXPORTS, min_version=TEXT_MIN_VERSION, missing_ok=False, needs="the CLIP text encoder's embedding, attention and activation need it", sigs={
        "pww_text_embed_ln": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp], _int),
        "pww_text_attn_fwd": ([_vp, _vp, _i32, _i32, _i32, _i64, _i64, _i32, _vp], _int),
        "pww_text_act": ([_vp, _i64, _i32, _i64, _i32, _i32, _vp], _int)}),
}
_side = {}      # name -> loaded handle


def side_spec(name):
    """The table entry of a side library (SIDE, SIDE_MORE, SIDE_CONV or SIDE_EXTRA)."""
    for table in (SIDE, SIDE_MORE, SIDE_CONV):
        if name in table:
            return table[name]
    return SIDE_EXTRA[name]


def load_side(name):
    """libpww_hip_<name>.so of SIDE / SIDE_MORE / SIDE_CONV / SIDE_EXTRA, loaded once. A missing file returns None where the table says so (scope: the caller keeps the
    materialised route) and raises otherwise -- there is no second implementation to fall back to. A file that is there but stale, broken
    or short of an entry point raises. Every failure is a PwwHipError with the rebuild hint."""
    lib = _side.get(name)
    if lib is not None:
        return lib
    spec = side_spec(name)
    path, so, pre = globals()[spec["path"]], "libpww_hip_%s.so" % name, "pww_%s_" % name
    if not os.path.isfile(path):
        if spec["missing_ok"]:
            return None
        raise PwwHipError("%s not found at %s: %s %s" % (so, path, spec["needs"], _HINT))
    try:
        lib = ctypes.CDLL(path)
        getattr(lib, pre + "version").restype = _int
        version = getattr(lib, pre + "version")()
    except (OSError, AttributeError) as e:
        raise PwwHipError("%s at %s cannot be loaded: %s %s" % (so, path, e, _HINT))
    # first of all: an older library lacks symbols that are bound below
    if version // 100 != 1 or version < spec["min_version"]:
        raise PwwHipError("%s ABI version %d is not 1.x >= %d %s" % (so[:-3], version, spec["min_version"], _HINT))
    missing = [n for n in spec["exports"] if not hasattr(lib, n)]
    if missing:
        raise PwwHipError("%s at %s lacks %s %s" % (so, path, missing, _HINT))
    for fn, (argtypes, restype) in spec["sigs"].items():
        getattr(lib, fn).argtypes, getattr(lib, fn).restype = argtypes, restype
    getattr(lib, pre + "last_error").restype = ctypes.c_char_p
    lib.pww_last_error = getattr(lib, pre + "last_error")        # (`check(rc, what, lib)` asks the library it is given)
    _side[name] = lib
    return lib


# the public names (ops.py calls them per launch: after the first call, one lookup and one test)
def load_long():
    lib = _side.get("long")
    return lib if lib is not None else load_side("long")


def load_scope():
    lib = _side.get("scope")
    return lib if lib is not None else load_side("scope")


def load_linear():
    lib = _side.get("linear")
    return lib if lib is not None else load_side("linear")


def load_regions():
    lib = _side.get("regions")
    return lib if lib is not None else load_side("regions")


def load_lora():
    lib = _side.get("lora")
    return lib if lib is not None else load_side("lora")


def load_convtail():
    lib = _side.get("convtail")
    return lib if lib is not None else load_side("convtail")


def load_canvas():
    lib = _side.get("canvas")
    return lib if lib is not None else load_side("canvas")


def load_concat():
    lib = _side.get("concat")
    return lib if lib is not None else load_side("concat")


def load_hold():
    lib = _side.get("hold")
    return lib if lib is not None else load_side("hold")


def load_convwide():
    lib = _side.get("convwide")
    return lib if lib is not None else load_side("convwide")


def load_vae():
    lib = _side.get("vae")
    return lib if lib is not None else load_side("vae")


def load_vaeenc():
    lib = _side.get("vaeenc")
    return lib if lib is not None else load_side("vaeenc")


def load_text():
    lib = _side.get("text")
    return lib if lib is not None else load_side("text")


def load_control():
    lib = _side.get("control")
    return lib if lib is not None else load_side("control")


def load_step():
    lib = _side.get("step")
    return lib if lib is not None else load_side("step")


class experiments:
    """TEST / TOOL scope: inside `with _lib.experiments():` every op of this process runs on libpww_hip_experiments.so (`load()` returns
    it), e.g. a whole request with the compact bias form; the product library is back afterwards."""

    def __enter__(self):
        global _lib
        load()
        self._prev = _lib
        _lib = load_experiments()
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self._prev
        return False


def check(rc, what, lib=None):
    if rc != PWW_OK:
        msg = (lib or load()).pww_last_error().decode("utf-8", "replace")
        raise PwwHipError("%s failed (rc=%d): %s" % (what, rc, msg))


def device_arch():
    buf = ctypes.create_string_buffer(64)
    check(load().pww_device_arch(buf, 64), "pww_device_arch")
    return buf.value.decode()

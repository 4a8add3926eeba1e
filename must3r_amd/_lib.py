"""ctypes binding of ``libmust3r_hip.so`` (C ABI declared in ``include/must3r_hip.h``).

The shared library is built in-tree by ``must3r_amd/csrc/Makefile`` (``__graft_entry__.build()``).
There is no CPU or eager-PyTorch fallback: if the library is missing or no gfx950 device is visible
the product path raises, it never silently computes elsewhere.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmust3r_hip.so")

BF16, F16, F16_W2, F16_WA = 0, 1, 2, 3
ATTN_FP8 = 0x100   # OR-able: fp8 (e4m3) attention operands, include/must3r_hip.h
MEM_KV, MEM_NORM_Y, MEM_RAW = 0, 1, 2
PART_ENCODER, PART_DECODER = 1, 2
EPI_STORE16, EPI_STORE16_GELU, EPI_QKV_ROPE, EPI_RESID_F32, EPI_F32, EPI_HEAD = range(6)
ABI_VERSION = 21
ACT_NORM_EXP, ACT_LINEAR = 0, 1
EXPORT_MAX_THR, EXPORT_GLB, EXPORT_PLY = 8, 0, 1
RENDER_MAX_POINT_SIZE = 8   # MUST3R_RENDER_MAX_POINT_SIZE
RENDER_MESH_WAVE_AREA = 64  # MUST3R_RENDER_MESH_WAVE_AREA
NORM_AVG_DIS, NORM_AVG_LOG1P, NORM_SQRT_DIS, NORM_MEDIAN_DIS = range(4)
LOSS_W_SCALAR, LOSS_W_MEAN, LOSS_W_CONF, LOSS_W_PIXEL = range(4)
RESAMPLE_AA_BILINEAR, RESAMPLE_PIL_LANCZOS, RESAMPLE_PIL_BICUBIC, RESAMPLE_NEAREST_EXACT = range(4)
IMG_U8_HWC, IMG_F32_CHW = 0, 1
LIN_BIAS, LIN_BIAS_RES, LIN_BIAS_GELU = range(3)
TRAIN_LINEAR_F32, TRAIN_LINEAR_BF16 = 0, 1   # must3r_hip_train_linear_mode
TRAIN_ATTENTION_F32, TRAIN_ATTENTION_BF16 = 0, 1   # must3r_hip_train_attention_mode

class Config(C.Structure):
    _fields_ = [("img_size", C.c_int32), ("patch_size", C.c_int32),
                ("enc_dim", C.c_int32), ("enc_depth", C.c_int32), ("enc_heads", C.c_int32),
                ("dec_dim", C.c_int32), ("dec_depth", C.c_int32), ("dec_heads", C.c_int32),
                ("mlp_ratio", C.c_int32), ("rope_freq", C.c_float), ("rope_f0", C.c_float)]


class Group(C.Structure):
    _fields_ = [("tokens", C.c_void_p), ("pos", C.c_void_p),
                ("n_views", C.c_int32), ("n_tokens", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("pointmaps", C.c_void_p), ("pointmaps_scene_stride", C.c_int64)]


# must3r_hip_cp_exchange_fn: (user, layer, slots, slot_bytes, n_slots, my_slot, stream) -> status
CpExchangeFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p)


class Cp(C.Structure):
    """must3r_hip_cp: context-parallel cross attention over a memory sharded across ranks (include/must3r_hip.h, ABI 8)."""
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("n_mem_total", C.c_int32), ("partial16", C.c_int32),
                ("slots", C.c_void_p), ("slot_bytes", C.c_size_t), ("exchange", CpExchangeFn), ("user", C.c_void_p)]


class DecodeArgs(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("mem_mode", C.c_int32), ("render", C.c_int32), ("first_call", C.c_int32),
                ("n_groups", C.c_int32), ("groups", C.POINTER(Group)), ("n_mem", C.c_int32),
                ("mem", C.POINTER(C.c_void_p)), ("feats", C.c_void_p),
                ("mem_capacity", C.c_int32), ("n_scenes", C.c_int32), ("mem_scene_stride", C.c_int64),
                ("cp", C.POINTER(Cp)), ("causal", C.c_int32)]


class ImageDesc(C.Structure):
    """must3r_hip_image_desc: one image of a must3r_hip_resample call (include/must3r_hip.h, ABI 9)."""
    _fields_ = [("src", C.c_void_p), ("src_format", C.c_int32), ("channels", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("row_stride", C.c_int64), ("plane_stride", C.c_int64),
                ("crop_y", C.c_int32), ("crop_x", C.c_int32), ("crop_h", C.c_int32), ("crop_w", C.c_int32),
                ("resize_h", C.c_int32), ("resize_w", C.c_int32),
                ("out_y", C.c_int32), ("out_x", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32), ("out_offset", C.c_int64)]


class AttnOp(C.Structure):
    """must3r_hip_attn_op: one attention route of the decoder, or one context-parallel stage (include/must3r_hip.h, ABI 10)."""
    _fields_ = [("dtype", C.c_int32), ("Q", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p), ("O", C.c_void_p),
                ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32), ("heads", C.c_int32),
                ("views_dev", C.c_void_p), ("n_views", C.c_int32), ("view0_inline", C.c_int32), ("view0", C.c_int32 * 6),
                ("max_nq", C.c_int32), ("max_nk", C.c_int32), ("q_prescaled", C.c_int32),
                ("nsplit", C.c_int32), ("scratch", C.c_void_p), ("total_q_rows", C.c_int32), ("dense_rows", C.c_int32),
                ("stage", C.c_int32), ("slot_o", C.c_void_p), ("slot_ml", C.c_void_p), ("p16", C.c_int32), ("nslots", C.c_int32),
                ("stride_o", C.c_int64), ("stride_ml", C.c_int64), ("picked", C.POINTER(C.c_char_p))]


class LnOp(C.Structure):
    """must3r_hip_ln_op: one LayerNorm launch, every field of the kernels' descriptor (include/must3r_hip.h, ABI 15)."""
    _fields_ = [("dtype", C.c_int32), ("x", C.c_void_p), ("x16", C.c_void_p), ("add", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p),
                ("out16", C.c_void_p), ("out16_lo", C.c_void_p), ("out16_dup", C.c_void_p), ("ld16", C.c_int32),
                ("out32", C.c_void_p), ("copy32", C.c_void_p), ("raw16", C.c_void_p), ("M", C.c_int32), ("C", C.c_int32), ("eps", C.c_float),
                ("rows_per_group", C.c_int32), ("add_groups", C.c_int32), ("picked", C.POINTER(C.c_char_p)), ("mean_out", C.c_void_p)]


class GemmOp(C.Structure):
    """must3r_hip_gemm_op: one GEMM launch with the grouped and per-scene fields of the kernels' descriptor (include/must3r_hip.h, ABI 17)."""
    _fields_ = [("dtype", C.c_int32), ("epi", C.c_int32), ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("lda", C.c_int32), ("ldc", C.c_int32), ("wsplit", C.c_int32),
                ("Wlo_sp", C.c_void_p), ("Widx_sp", C.c_void_p), ("wsp_rows", C.c_int32), ("out_scale", C.c_float), ("scale_cols", C.c_int32),
                ("batch", C.c_int32), ("strideA", C.c_int64), ("strideW", C.c_int64), ("strideB", C.c_int64), ("out_table", C.c_void_p), ("wdiv", C.c_int32),
                ("pos", C.c_void_p), ("rope_tab", C.c_void_p), ("rope_cols", C.c_int32), ("rope_npos", C.c_int32),
                ("bias2", C.c_void_p), ("row_start2", C.c_int32), ("row_period2", C.c_int32), ("accumulate", C.c_int32),
                ("ntok", C.c_int32), ("gw", C.c_int32), ("H", C.c_int32), ("Wimg", C.c_int32), ("head_views", C.c_int32), ("head_scene_skip", C.c_int64),
                ("picked", C.POINTER(C.c_char_p))]


class LnFoldOp(C.Structure):
    """must3r_hip_lnfold_op: one LN-fold GEMM launch of a one-view update, plain or split weights (include/must3r_hip.h, ABI 18)."""
    _fields_ = [("dtype", C.c_int32), ("epi", C.c_int32), ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("lda", C.c_int32), ("ldc", C.c_int32), ("wsplit", C.c_int32),
                ("x16_out", C.c_void_p), ("copy32_out", C.c_void_p), ("stats_out", C.c_void_p),
                ("ln_stats", C.c_void_p), ("ln_s", C.c_void_p), ("ln_eps", C.c_float), ("ln_shift", C.c_void_p), ("ln_shift_init", C.c_int32),
                ("pos", C.c_void_p), ("rope_tab", C.c_void_p), ("rope_cols", C.c_int32), ("rope_npos", C.c_int32),
                ("out_scale", C.c_float), ("scale_cols", C.c_int32), ("bias2", C.c_void_p), ("row_start2", C.c_int32),
                ("picked", C.POINTER(C.c_char_p))]


class ExportView(C.Structure):
    """must3r_hip_export_view: one view of a scene export (include/must3r_hip.h, ABI 13)."""
    _fields_ = [("conf", C.c_void_p), ("pts", C.c_void_p), ("rgb", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("M", C.c_double * 12)]


class RenderCamera(C.Structure):
    """must3r_hip_render_camera: one pinhole camera of a render call (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("w2c", C.c_double * 12), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("z_near", C.c_float), ("z_far", C.c_float), ("W", C.c_int32), ("H", C.c_int32)]


class RenderDesc(C.Structure):
    """must3r_hip_render_desc: the HOST view and camera tables, the threshold, the point size, the background, the scratch, the (optional) DEVICE outputs and
    the stream of one render call (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("views", C.POINTER(ExportView)), ("cams", C.POINTER(RenderCamera)), ("n_views", C.c_int32), ("n_cams", C.c_int32),
                ("thr", C.c_float), ("point_size", C.c_int32), ("background", C.c_uint8 * 3), ("reserved", C.c_uint8 * 5),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("rgb", C.c_void_p), ("depth", C.c_void_p), ("index", C.c_void_p),
                ("stream", C.c_void_p)]


class RenderMeshDesc(C.Structure):
    """must3r_hip_render_mesh_desc: ``RenderDesc`` without the point size, for the triangle rasteriser (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("views", C.POINTER(ExportView)), ("cams", C.POINTER(RenderCamera)), ("n_views", C.c_int32), ("n_cams", C.c_int32),
                ("thr", C.c_float), ("background", C.c_uint8 * 3), ("reserved", C.c_uint8 * 1),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("rgb", C.c_void_p), ("depth", C.c_void_p), ("index", C.c_void_p),
                ("stream", C.c_void_p)]


class MetricsLossArgs(C.Structure):
    """must3r_hip_metrics_loss_args: one fused loss pass over [B, V, H, W] (include/must3r_hip.h, ABI 14)."""
    _fields_ = [("n_scenes", C.c_int32), ("n_views", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("gt_pts", C.c_void_p), ("in_camera0", C.c_void_p), ("w2c", C.c_void_p), ("pr_pts", C.c_void_p), ("pr_local", C.c_void_p),
                ("conf", C.c_void_p), ("valid", C.c_void_p), ("sky", C.c_void_p), ("gt_scale", C.c_void_p), ("pr_scale", C.c_void_p),
                ("pr_warp", C.c_void_p), ("gt_warp", C.c_int32), ("has_dist_clip", C.c_int32), ("loss_in_log", C.c_int32),
                ("dist_clip", C.c_float), ("sky_loss_value", C.c_float), ("alpha", C.c_float),
                ("counts", C.c_void_p), ("sums", C.c_void_p),
                ("pix_g", C.c_void_p), ("pix_l", C.c_void_p), ("msk_g", C.c_void_p), ("msk_l", C.c_void_p)]


class MetricsLossGradArgs(C.Structure):
    """must3r_hip_metrics_loss_grad_args: weights, counts, scale path and outputs of the loss backward (include/must3r_hip.h, ABI 16)."""
    _fields_ = [("w_g", C.c_void_p), ("w_l", C.c_void_p), ("weighting", C.c_int32), ("factor_mode", C.c_int32), ("n_own", C.c_int32),
                ("reserved", C.c_int32), ("counts", C.c_void_p), ("own_factor", C.c_void_p), ("n_valid", C.c_void_p),
                ("grad_pts", C.c_void_p), ("grad_local", C.c_void_p), ("grad_conf", C.c_void_p)]


class HeadGradArgs(C.Structure):
    """must3r_hip_head_grad_args: inputs and (optional) outputs of the prediction head's backward (include/must3r_hip.h, ABI 19)."""
    _fields_ = [("x", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("W", C.c_void_p), ("G", C.c_void_p),
                ("n_views", C.c_int32), ("H", C.c_int32), ("Wimg", C.c_int32), ("D", C.c_int32), ("eps", C.c_float), ("reserved", C.c_int32),
                ("dx", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("dW", C.c_void_p), ("db", C.c_void_p)]


class HeadForwardArArgs(C.Structure):
    """must3r_hip_head_forward_ar_args: the arguments of must3r_hip_head_forward, the DEVICE orientation flags and the stream of the head's forward over a batch
    stored landscape (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("x", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("W", C.c_void_p), ("b", C.c_void_p),
                ("dtype", C.c_int32), ("n_views", C.c_int32), ("H", C.c_int32), ("Wimg", C.c_int32), ("D", C.c_int32), ("eps", C.c_float),
                ("pointmaps", C.c_void_p), ("transposed", C.c_void_p), ("stream", C.c_void_p)]


class HeadGradArArgs(C.Structure):
    """must3r_hip_head_grad_ar_args: the ABI 19 descriptor, the DEVICE orientation flags and the stream of the head's backward over a batch stored landscape
    (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("g", HeadGradArgs), ("transposed", C.c_void_p), ("stream", C.c_void_p)]


class AttnTrainArgs(C.Structure):
    """must3r_hip_attn_train_args: operands, HOST view table and (optional) outputs of the attention training forward / backward (include/must3r_hip.h, ABI 20)."""
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("dO", C.c_void_p),
                ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("lddo", C.c_int32), ("heads", C.c_int32), ("n_views", C.c_int32),
                ("views", C.c_void_p), ("O", C.c_void_p), ("lse", C.c_void_p), ("dQ", C.c_void_p), ("dK", C.c_void_p), ("dV", C.c_void_p),
                ("ldo", C.c_int32), ("lddq", C.c_int32), ("lddk", C.c_int32), ("lddv", C.c_int32)]


class AttnMaskedArgs(C.Structure):
    """must3r_hip_attn_masked_args: the ABI 20 descriptor, the packed key masks (DEVICE), each view's mask row (HOST) and the stream of the masked attention
    training forward / backward (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("core", AttnTrainArgs), ("mask_bits", C.c_void_p), ("view_mask", C.c_void_p), ("mask_rows", C.c_int32), ("mask_ld", C.c_int32),
                ("stream", C.c_void_p)]


class MlpSublayerArgs(C.Structure):
    """must3r_hip_mlp_sublayer_args: inputs and (optional) outputs of the MLP sublayer's training forward / backward (include/must3r_hip.h, ABI 21)."""
    _fields_ = [("x", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("W1", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p),
                ("dy", C.c_void_p), ("M", C.c_int32), ("D", C.c_int32), ("hidden", C.c_int32), ("eps", C.c_float), ("out", C.c_void_p),
                ("dx", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("dW1", C.c_void_p), ("db1", C.c_void_p), ("dW2", C.c_void_p),
                ("db2", C.c_void_p)]


class AttnSublayerArgs(C.Structure):
    """must3r_hip_attn_sublayer_args: inputs, device positions and RoPE table, HOST view table and (optional) outputs of the attention sublayer's training
    forward / backward (include/must3r_hip.h, ABI 21)."""
    _fields_ = [("x", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("Wqkv", C.c_void_p), ("bqkv", C.c_void_p), ("Wproj", C.c_void_p),
                ("bproj", C.c_void_p), ("dy", C.c_void_p), ("pos", C.c_void_p), ("rope_tab", C.c_void_p), ("views", C.c_void_p),
                ("M", C.c_int32), ("D", C.c_int32), ("n_views", C.c_int32), ("rope_npos", C.c_int32), ("eps", C.c_float), ("reserved", C.c_int32),
                ("out", C.c_void_p), ("dx", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("dWqkv", C.c_void_p), ("dbqkv", C.c_void_p),
                ("dWproj", C.c_void_p), ("dbproj", C.c_void_p)]


class CrossSublayerArgs(C.Structure):
    """must3r_hip_cross_sublayer_args: inputs, HOST view table, (optional) outputs and the stream of the cross-attention sublayer's training forward /
    backward (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("x", C.c_void_p), ("mem", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("Wq", C.c_void_p), ("bq", C.c_void_p),
                ("Wk", C.c_void_p), ("bk", C.c_void_p), ("Wv", C.c_void_p), ("bv", C.c_void_p), ("Wproj", C.c_void_p), ("bproj", C.c_void_p),
                ("dy", C.c_void_p), ("views", C.c_void_p), ("out", C.c_void_p),
                ("dx", C.c_void_p), ("dmem", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("dWq", C.c_void_p), ("dbq", C.c_void_p),
                ("dWk", C.c_void_p), ("dbk", C.c_void_p), ("dWv", C.c_void_p), ("dbv", C.c_void_p), ("dWproj", C.c_void_p), ("dbproj", C.c_void_p),
                ("M", C.c_int32), ("Rm", C.c_int32), ("D", C.c_int32), ("n_views", C.c_int32), ("ldmem", C.c_int32), ("lddmem", C.c_int32),
                ("eps", C.c_float), ("reserved", C.c_int32), ("stream", C.c_void_p)]


class CrossSublayerMaskedArgs(C.Structure):
    """must3r_hip_cross_sublayer_masked_args: the cross-attention sublayer's descriptor and the key masks handed to its attention core (include/must3r_hip.h,
    ABI 21, additive)."""
    _fields_ = [("core", CrossSublayerArgs), ("mask_bits", C.c_void_p), ("view_mask", C.c_void_p), ("mask_rows", C.c_int32), ("mask_ld", C.c_int32)]


FEEDBACK_MAX_LAYERS = 32


class FeedbackPrepareArgs(C.Structure):
    """must3r_hip_feedback_prepare_args: the per-layer pointers by value, the offset, (optional) outputs and the stream of the feedback add + ``norm_y`` of
    all layers, forward / backward (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [(n, C.c_void_p * FEEDBACK_MAX_LAYERS) for n in ("x", "gamma", "beta", "dy", "y", "dx", "dgamma", "dbeta")] + [
        ("offset", C.c_void_p), ("doffset", C.c_void_p), ("L", C.c_int32), ("R", C.c_int32), ("D", C.c_int32), ("add_layers", C.c_int32),
        ("eps", C.c_float), ("reserved", C.c_int32), ("stream", C.c_void_p)]


OPTIM_CHUNK = 32768   # MUST3R_OPTIM_CHUNK: elements of one chunk of the optimizer's tensor table


class OptimTensor(C.Structure):
    """must3r_hip_optim_tensor: one parameter tensor of the optimizer's table, DEVICE pointers (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("step", C.c_void_p), ("n", C.c_int64),
                ("group", C.c_int32), ("reserved", C.c_int32)]


class OptimGroup(C.Structure):
    """must3r_hip_optim_group: the numbers of one parameter group, ``lr`` the effective rate (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("lr", C.c_double), ("weight_decay", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class OptimControl(C.Structure):
    """must3r_hip_optim_control: the device record optim_norm writes and optim_adamw reads (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("norm", C.c_float), ("coef", C.c_float), ("found_inf", C.c_int32), ("reserved", C.c_int32)]


class OptimArgs(C.Structure):
    """must3r_hip_optim_args: the HOST tables, the control record, the (optional) scaler state and the stream of the optimizer's two passes
    (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("tensors", C.POINTER(OptimTensor)), ("groups", C.POINTER(OptimGroup)), ("n_tensors", C.c_int32), ("n_groups", C.c_int32),
                ("control", C.c_void_p), ("scale", C.c_void_p), ("growth_tracker", C.c_void_p),
                ("max_norm", C.c_float), ("growth_factor", C.c_float), ("backoff_factor", C.c_float), ("growth_interval", C.c_int32),
                ("stream", C.c_void_p)]


class PatchRowsArgs(C.Structure):
    """must3r_hip_patch_rows_args: the image batch, the DEVICE orientation flags, the (optional) rows and positions and the stream of the gather in front
    of the trainable patch embedding (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("img", C.c_void_p), ("transposed", C.c_void_p), ("rows", C.c_void_p), ("pos", C.c_void_p),
                ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("reserved", C.c_int32), ("stream", C.c_void_p)]


GT_VIEW_BLOCKS = 32   # MUST3R_GT_VIEW_BLOCKS: the scratch behind n_valid holds 4 * V * GT_VIEW_BLOCKS bytes


class GtArgs(C.Structure):
    """must3r_hip_gt_args: depth (fp32, or uint16 with per-view (div, mul)), intrinsics, poses and DEVICE orientation flags of a batch stored landscape, the
    (optional) ground-truth outputs, the scratch behind ``n_valid`` and the stream (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("depth", C.c_void_p), ("depth_scale", C.c_void_p), ("K", C.c_void_p), ("c2w", C.c_void_p), ("transposed", C.c_void_p),
                ("pts3d", C.c_void_p), ("valid", C.c_void_p), ("sky", C.c_void_p), ("n_valid", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("V", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("depth_u16", C.c_int32), ("stream", C.c_void_p)]


AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE = range(4)   # MUST3R_AUG_*: the operations of the colour jitter
AUG_TILE = 64   # MUST3R_AUG_TILE


class AugmentColorView(C.Structure):
    """must3r_hip_augment_color_view: one view of the colour jitter's HOST table -- where its planes lie in the resampler's output, its true size, the
    portrait flag, the order of the four operations, and a flag and a factor per operation (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("src_offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("portrait", C.c_int32), ("order", C.c_int32 * 4),
                ("apply", C.c_int32 * 4), ("factor", C.c_float * 4), ("reserved", C.c_int32)]


class AugmentColorArgs(C.Structure):
    """must3r_hip_augment_color_args: the resampler's output, the HOST view table, the ImgNorm batch stored landscape, the scratch and the stream
    (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("src", C.c_void_p), ("src_elems", C.c_int64), ("views", C.POINTER(AugmentColorView)), ("out", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("V", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("reserved", C.c_int32), ("stream", C.c_void_p)]


class AugmentDepthView(C.Structure):
    """must3r_hip_augment_depth_view: one view of the depth gather's HOST table -- its raw depth map on the DEVICE and the geometry the image went through
    (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("src", C.c_void_p), ("row_stride", C.c_int64), ("H", C.c_int32), ("W", C.c_int32),
                ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_w", C.c_int32), ("crop_h", C.c_int32),
                ("resize_w", C.c_int32), ("resize_h", C.c_int32),
                ("win_x", C.c_int32), ("win_y", C.c_int32), ("out_w", C.c_int32), ("out_h", C.c_int32), ("portrait", C.c_int32), ("reserved", C.c_int32)]


class AugmentDepthArgs(C.Structure):
    """must3r_hip_augment_depth_args: the HOST view table, the depth batch stored landscape (fp32 or uint16), the scratch and the stream
    (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("views", C.POINTER(AugmentDepthView)), ("out", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("V", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("depth_u16", C.c_int32), ("stream", C.c_void_p)]


SLAM_RECORD_DOUBLES, SLAM_FOCAL_STATE_DOUBLES = 32, 4   # MUST3R_SLAM_RECORD_DOUBLES, MUST3R_SLAM_FOCAL_STATE_DOUBLES
SLAM_MODE_NN, SLAM_MODE_NORM, SLAM_MODE_MEANCONF, SLAM_MODE_MEDIANCONF = 1, 2, 4, 8   # MUST3R_SLAM_MODE_*


class SlamPoseArgs(C.Structure):
    """must3r_hip_slam_pose_args: raw head output of B views, the activated outputs, focal and c2w, the agent's running focal sums and (f, c) log on the
    DEVICE, the scratch and the stream (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("pm", C.c_void_p), ("pts3d", C.c_void_p), ("pts3d_local", C.c_void_p), ("conf", C.c_void_p), ("focal", C.c_void_p), ("c2w", C.c_void_p),
                ("focal_state", C.c_void_p), ("focal_log", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("activation", C.c_int32),
                ("is_first", C.c_int32), ("use_seq_focal", C.c_int32), ("update_focal", C.c_int32), ("focal_log_cap", C.c_int32), ("stream", C.c_void_p)]


class SlamKeyframeArgs(C.Structure):
    """must3r_hip_slam_keyframe_args: one frame's activated maps and its c2w on the DEVICE, the map's index (or none), the compacted points, the
    per-frame record, the scratch and the stream (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("pts3d", C.c_void_p), ("pts3d_local", C.c_void_p), ("conf", C.c_void_p), ("c2w", C.c_void_p), ("focal", C.c_void_p),
                ("focal_state", C.c_void_p), ("index", C.c_void_p), ("sel", C.c_void_p), ("dist", C.c_void_p), ("record", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("quantile", C.c_double), ("min_conf", C.c_float),
                ("H", C.c_int32), ("W", C.c_int32), ("subsamp", C.c_int32), ("divider", C.c_int32), ("mode", C.c_int32), ("stream", C.c_void_p)]


JPEG_SUBSEQ_BYTES = 128   # MUST3R_JPEG_SUBSEQ_BYTES
JPEG_PATH_FAST, JPEG_PATH_SEQUENTIAL = 0, 1   # MUST3R_JPEG_PATH_*


class JpegHuff(C.Structure):
    """must3r_hip_jpeg_huff: one Huffman table as the kernels read it (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("look", C.c_uint16 * 512), ("maxcode", C.c_int32 * 18), ("valoff", C.c_int32 * 18), ("vals", C.c_uint8 * 256)]


class JpegInfo(C.Structure):
    """must3r_hip_jpeg_info: what must3r_hip_jpeg_parse takes the marker segments of one file to (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("blocks_per_mcu", C.c_int32), ("n_blocks", C.c_int32),
                ("restart_interval", C.c_int32), ("n_segments", C.c_int32), ("reserved", C.c_int32),
                ("scan_offset", C.c_int64), ("scan_bytes", C.c_int64), ("comp_dc", C.c_int32 * 3), ("comp_ac", C.c_int32 * 3),
                ("quant", (C.c_uint16 * 64) * 3), ("natural", C.c_uint8 * 64), ("dc", JpegHuff * 2), ("ac", JpegHuff * 2)]


class JpegImage(C.Structure):
    """must3r_hip_jpeg_image: one image of a decode call -- HOST info and segment offsets, DEVICE file bytes and output (include/must3r_hip.h, ABI 21)."""
    _fields_ = [("info", C.POINTER(JpegInfo)), ("seg_offsets", C.POINTER(C.c_uint32)), ("data", C.c_void_p), ("data_bytes", C.c_size_t),
                ("out", C.c_void_p), ("out_row_stride", C.c_int64)]


class JpegBatch(C.Structure):
    """must3r_hip_jpeg_batch: the HOST image table, the DEVICE path flags, the scratch and the stream of one decode call (include/must3r_hip.h, ABI 21)."""
    _fields_ = [("images", C.POINTER(JpegImage)), ("n_images", C.c_int32), ("reserved", C.c_int32), ("flags", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("stream", C.c_void_p)]


PNG_OUT_RGB8, PNG_OUT_GRAY8, PNG_OUT_GRAY16 = 0, 1, 2   # MUST3R_PNG_OUT_*
# MUST3R_PNG_STATUS_*: the status word of one image after must3r_hip_png_decode
PNG_STATUS = {0: "ok", 1: "invalid block type", 2: "invalid set of code lengths", 3: "invalid code", 4: "invalid literal/length or distance symbol",
              5: "distance beyond the written output", 6: "output beyond the expected size", 7: "the stream ends early", 8: "final size is not the expected one",
              9: "stored block length check", 10: "Adler-32 mismatch", 11: "filter type above 4"}


class PngInfo(C.Structure):
    """must3r_hip_png_info: what must3r_hip_png_parse takes the chunks of one file to (include/must3r_hip.h, ABI 21, additive)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("color_type", C.c_int32), ("bit_depth", C.c_int32), ("channels", C.c_int32), ("bpp", C.c_int32),
                ("n_idat", C.c_int32), ("reserved", C.c_int32), ("rowbytes", C.c_int64), ("inflated_bytes", C.c_int64), ("idat_bytes", C.c_int64)]


class PngRange(C.Structure):
    """must3r_hip_png_range: the payload of one IDAT chunk, bytes from the start of the file (include/must3r_hip.h, ABI 21)."""
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint64)]


class PngImage(C.Structure):
    """must3r_hip_png_image: one image of a decode call -- HOST info, DEVICE zlib stream, output and optional scanline buffer (include/must3r_hip.h, ABI 21)."""
    _fields_ = [("info", C.POINTER(PngInfo)), ("zdata", C.c_void_p), ("out", C.c_void_p), ("out_row_stride", C.c_int64),
                ("out_format", C.c_int32), ("reserved", C.c_int32), ("inflated", C.c_void_p)]


class PngBatch(C.Structure):
    """must3r_hip_png_batch: the HOST image table, the DEVICE status words, the scratch and the stream of one decode call (include/must3r_hip.h, ABI 21)."""
    _fields_ = [("images", C.POINTER(PngImage)), ("n_images", C.c_int32), ("reserved", C.c_int32), ("status", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("stream", C.c_void_p)]


class ProfRecord(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("ms", C.c_double), ("flops", C.c_double), ("calls", C.c_int64)]


# every symbol include/must3r_hip.h declares, in its order: name -> (restype, argtypes)
vp, i32, i64, fp, sz, cstr, P = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t, C.c_char_p, C.POINTER
PROTOTYPES = {
    "must3r_hip_last_error": (cstr, []),
    "must3r_hip_has_fp8_attention": (i32, []),
    "must3r_hip_abi_version": (i32, []),
    "must3r_hip_set_option": (i32, [cstr, i64]),
    "must3r_hip_create": (i32, [P(Config), i32, P(vp)]),
    "must3r_hip_destroy": (None, [vp]),
    "must3r_hip_load_weight": (i32, [vp, cstr, vp, i32, i32, P(i64)]),
    "must3r_hip_finalize_weights": (i32, [vp, i32]),
    "must3r_hip_encode": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp]),
    "must3r_hip_cp_slot_bytes": (sz, [vp, i32]),
    "must3r_hip_cp_slot_bytes16": (sz, [vp, i32]),
    "must3r_hip_decode": (i32, [vp, P(DecodeArgs), vp]),
    "must3r_hip_postprocess": (i32, [vp, vp, vp, vp, sz, vp]),
    "must3r_hip_postprocess_act": (i32, [vp, i32, vp, vp, vp, sz, vp]),
    "must3r_hip_postprocess_act_grad": (i32, [vp, i32, vp, vp, vp, vp, sz, vp]),
    "must3r_hip_postprocess_cam_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_postprocess_cam": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "must3r_hip_postprocess_cam_act": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "must3r_hip_affine": (i32, [i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp]),
    "must3r_hip_row_norm": (i32, [vp, i32, i32, vp, vp]),
    "must3r_hip_l2_normalize": (i32, [vp, i64, i32, i64, vp, vp]),
    "must3r_hip_layernorm_act_f32": (i32, [vp, vp, vp, fp, i32, i32, i32, vp, vp]),
    "must3r_hip_topk_gather": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "must3r_hip_weighted_spoc": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "must3r_hip_asmk_quantize_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_asmk_centroid_sqnorm": (i32, [vp, i32, i32, vp, vp]),
    "must3r_hip_asmk_quantize": (i32, [vp, i32, vp, vp, i32, i32, i32, vp, vp, sz, vp]),
    "must3r_hip_asmk_aggregate": (i32, [vp, vp, i32, i32, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp]),
    "must3r_hip_asmk_scores": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, fp, fp, i32, vp, vp]),
    "must3r_hip_kmeans_update_scratch_bytes": (sz, [i32, i32]),
    "must3r_hip_kmeans_update": (i32, [vp, i32, i32, vp, i32, vp, i64, vp, vp, vp, vp, vp, P(C.c_double), vp, vp, sz]),
    "must3r_hip_cov_accumulate_scratch_bytes": (sz, [i32, i32]),
    "must3r_hip_cov_accumulate": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, sz]),
    "must3r_hip_nn_query": (i32, [vp, i64, vp, i64, vp, vp]),
    "must3r_hip_quadrant_ids": (i32, [vp, i64, P(fp), i32, vp, vp]),
    "must3r_hip_nn_index_bytes": (sz, [i64, i32]),
    "must3r_hip_nn_index_scratch_bytes": (sz, [i64]),
    "must3r_hip_nn_index_build": (i32, [vp, vp, i64, i32, vp, vp, vp]),
    "must3r_hip_nn_index_query": (i32, [vp, vp, i64, P(fp), i32, vp, vp]),
    "must3r_hip_export_scratch_bytes": (sz, [P(ExportView), i32, i32, i32]),
    "must3r_hip_export_count": (i32, [P(ExportView), i32, P(fp), i32, i32, vp, sz, P(i64), vp]),
    "must3r_hip_export_scatter_points": (i32, [P(ExportView), i32, P(fp), i32, i32, i32, vp, vp, vp, vp, vp]),
    "must3r_hip_export_vertices": (i32, [P(ExportView), i32, i32, vp, vp, vp, vp, vp]),
    "must3r_hip_export_scatter_faces": (i32, [P(ExportView), i32, P(fp), i32, i32, vp, vp, vp]),
    "must3r_hip_metrics_loss_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "must3r_hip_metrics_loss": (i32, [P(MetricsLossArgs), vp, sz, vp]),
    "must3r_hip_metrics_factor_scratch_bytes": (sz, [i32, i32, i32, i32, i32]),
    "must3r_hip_metrics_factor": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    "must3r_hip_metrics_loss_grad_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "must3r_hip_metrics_loss_grad": (i32, [P(MetricsLossArgs), P(MetricsLossGradArgs), vp, sz, vp]),
    "must3r_hip_resample_coeffs": (i32, [i32, i32, i32, P(i32), vp, vp]),
    "must3r_hip_image_scratch_bytes": (sz, [i32, P(ImageDesc), i32]),
    "must3r_hip_resample": (i32, [i32, P(ImageDesc), i32, vp, vp, sz, vp]),
    "must3r_hip_op_gemm": (i32, [i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "must3r_hip_op_sparse24_pack": (i32, [vp, i32, i32, vp, vp, vp]),
    "must3r_hip_op_gemm_sp": (i32, [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp]),
    "must3r_hip_op_gemm_lnfold": (i32, [i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, fp, vp, i32, vp, vp, i32, i32, fp, i32, vp]),
    "must3r_hip_op_gemm_lnfold_ex": (i32, [P(LnFoldOp), vp]),
    "must3r_hip_op_gemm_fold256": (i32, [i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, fp, vp, vp, vp, i32, i32, fp, i32, vp]),
    "must3r_hip_op_gemm_ex": (i32, [P(GemmOp), vp]),
    "must3r_hip_rope_table": (i32, [fp, fp, i32, vp]),
    "must3r_hip_attention_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_op_attention": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, i32, vp, i32, vp]),
    "must3r_hip_op_attention_ex": (i32, [P(AttnOp), vp]),
    "must3r_hip_op_layernorm": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, fp, vp]),
    "must3r_hip_op_layernorm_ex": (i32, [P(LnOp), vp]),
    "must3r_hip_op_im2col": (i32, [i32, vp, vp, i32, i32, i32, vp]),
    "must3r_hip_op_cast": (i32, [i32, vp, vp, vp, sz, vp]),
    "must3r_hip_head_grad_splits": (i32, [i32]),
    "must3r_hip_head_forward_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "must3r_hip_head_forward": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, fp, vp, vp, sz, vp]),
    "must3r_hip_op_head_linear": (i32, [i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, sz, vp]),
    "must3r_hip_head_grad_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "must3r_hip_head_grad": (i32, [P(HeadGradArgs), vp, sz, vp]),
    "must3r_hip_head_forward_many_ar_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "must3r_hip_head_forward_many_ar": (i32, [P(HeadForwardArArgs), vp, sz]),
    "must3r_hip_head_grad_many_ar_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "must3r_hip_head_grad_many_ar": (i32, [P(HeadGradArArgs), vp, sz]),
    "must3r_hip_op_linear_dgrad_f32": (i32, [vp, i32, vp, vp, i32, i32, i32, vp]),
    "must3r_hip_op_linear_wgrad_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_op_linear_wgrad_f32": (i32, [vp, i32, vp, i32, vp, vp, i32, i32, i32, vp, sz, vp]),
    "must3r_hip_op_layernorm_grad_scratch_bytes": (sz, [i32, i32]),
    "must3r_hip_op_layernorm_grad": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, fp, vp, sz, vp]),
    "must3r_hip_attn_train_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "must3r_hip_attn_train_groups": (i32, [vp, i32]),
    "must3r_hip_attn_forward_f32": (i32, [P(AttnTrainArgs), vp, sz, vp]),
    "must3r_hip_attn_grad": (i32, [P(AttnTrainArgs), vp, sz, vp]),
    "must3r_hip_attn_masked_scratch_bytes": (sz, [i32, i32, i32, i32]),
    "must3r_hip_attn_masked_forward": (i32, [P(AttnMaskedArgs), vp, sz]),
    "must3r_hip_attn_masked_grad": (i32, [P(AttnMaskedArgs), vp, sz]),
    "must3r_hip_op_linear_f32": (i32, [i32, vp, i32, vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, vp]),
    "must3r_hip_op_layernorm_f32": (i32, [vp, vp, vp, vp, i32, i32, fp, vp]),
    "must3r_hip_op_gelu_f32": (i32, [vp, vp, vp, C.c_longlong, vp]),
    "must3r_hip_op_gelu_grad_f32": (i32, [vp, i32, vp, i32, vp, i32, i32, i32, vp]),
    "must3r_hip_op_rope_f32": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, vp]),
    "must3r_hip_op_layernorm_grad_add": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, fp, vp, sz, vp]),
    "must3r_hip_mlp_sublayer_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_mlp_sublayer_forward": (i32, [P(MlpSublayerArgs), vp, sz, vp]),
    "must3r_hip_mlp_sublayer_grad": (i32, [P(MlpSublayerArgs), vp, sz, vp]),
    "must3r_hip_attn_sublayer_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_attn_sublayer_forward": (i32, [P(AttnSublayerArgs), vp, sz, vp]),
    "must3r_hip_attn_sublayer_grad": (i32, [P(AttnSublayerArgs), vp, sz, vp]),
    "must3r_hip_cross_sublayer_scratch_bytes": (sz, [i32, i32, i32, i32, i32]),
    "must3r_hip_cross_sublayer_forward": (i32, [P(CrossSublayerArgs), vp, sz]),
    "must3r_hip_cross_sublayer_grad": (i32, [P(CrossSublayerArgs), vp, sz]),
    "must3r_hip_cross_sublayer_masked_scratch_bytes": (sz, [i32, i32, i32, i32, i32]),
    "must3r_hip_cross_sublayer_masked_forward": (i32, [P(CrossSublayerMaskedArgs), vp, sz]),
    "must3r_hip_cross_sublayer_masked_grad": (i32, [P(CrossSublayerMaskedArgs), vp, sz]),
    "must3r_hip_feedback_prepare_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_feedback_prepare_forward": (i32, [P(FeedbackPrepareArgs), vp, sz]),
    "must3r_hip_feedback_prepare_grad": (i32, [P(FeedbackPrepareArgs), vp, sz]),
    "must3r_hip_optim_scratch_bytes": (sz, [i64, i64]),
    "must3r_hip_optim_norm": (i32, [P(OptimArgs), vp, sz]),
    "must3r_hip_optim_adamw": (i32, [P(OptimArgs), vp, sz]),
    "must3r_hip_train_linear_mode": (i32, [i32]),
    "must3r_hip_train_attention_mode": (i32, [i32]),
    "must3r_hip_patch_rows": (i32, [P(PatchRowsArgs)]),
    "must3r_hip_gt_from_depth": (i32, [P(GtArgs)]),
    "must3r_hip_augment_color_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_augment_color": (i32, [P(AugmentColorArgs)]),
    "must3r_hip_augment_depth_scratch_bytes": (sz, [i32]),
    "must3r_hip_augment_depth": (i32, [P(AugmentDepthArgs)]),
    "must3r_hip_jpeg_parse": (i32, [vp, sz, P(JpegInfo), P(C.c_uint32), sz, vp, sz]),
    "must3r_hip_jpeg_scratch_bytes": (sz, [P(JpegImage), i32]),
    "must3r_hip_jpeg_decode": (i32, [P(JpegBatch)]),
    "must3r_hip_png_parse": (i32, [vp, sz, P(PngInfo), P(PngRange), sz, vp, sz]),
    "must3r_hip_png_scratch_bytes": (sz, [P(PngImage), i32]),
    "must3r_hip_png_decode": (i32, [P(PngBatch)]),
    "must3r_hip_slam_pose_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_slam_pose": (i32, [P(SlamPoseArgs)]),
    "must3r_hip_slam_keyframe_scratch_bytes": (sz, [i32, i32, i32]),
    "must3r_hip_slam_keyframe": (i32, [P(SlamKeyframeArgs)]),
    "must3r_hip_render_scratch_bytes": (sz, [P(RenderDesc)]),
    "must3r_hip_render": (i32, [P(RenderDesc)]),
    "must3r_hip_render_mesh_scratch_bytes": (sz, [P(RenderMeshDesc)]),
    "must3r_hip_render_mesh": (i32, [P(RenderMeshDesc)]),
    "must3r_hip_debug_tr_probe": (i32, [vp, vp]),
    "must3r_hip_set_profiling": (i32, [vp, i32]),
    "must3r_hip_get_profile": (i32, [vp, P(ProfRecord), i32, i32]),
}
EXPORTS = tuple(PROTOTYPES)


class HipError(RuntimeError):
    pass


_lib = None


def load():
    """dlopen the library (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C must3r_amd/csrc). must3r_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.must3r_hip_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.must3r_hip_abi_version()} != {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def stream_ptr(device):
    """Handle of the current stream of ``device``, as the ``stream`` arguments of the library take it."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def check(rc):
    if rc != 0:
        raise HipError(load().must3r_hip_last_error().decode("utf-8", "replace"))


def has_fp8_attention():
    """Was the library built with the parked e4m3 attention path (make EXTRA=-DM3R_ATTN_FP8; include/must3r_hip.h MUST3R_ATTN_FP8)?"""
    return bool(load().must3r_hip_has_fp8_attention())


def set_option(name, value):
    """Process-wide A/B switch of the library (include/must3r_hip.h ``must3r_hip_set_option``): raises on an unknown
    name or a value outside the switch's range."""
    check(load().must3r_hip_set_option(name.encode(), int(value)))


def make_config(cfg):
    return Config(cfg.img_size, cfg.patch_size, cfg.enc_dim, cfg.enc_depth, cfg.enc_heads,
                  cfg.dec_dim, cfg.dec_depth, cfg.dec_heads, cfg.mlp_ratio, cfg.rope_freq, cfg.rope_f0)


class Context:
    """Owner of one ``must3r_hip_ctx`` (one device, one forward in flight)."""

    def __init__(self, cfg, device_index):
        self.lib = load()
        self.handle = C.c_void_p()
        c = make_config(cfg)
        check(self.lib.must3r_hip_create(C.byref(c), int(device_index), C.byref(self.handle)))
        self.device_index = int(device_index)

    def load_weight(self, name, tensor):
        """tensor: contiguous fp32 torch tensor (host or the context's device)."""
        import torch
        t = tensor.detach()
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.float().contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        check(self.lib.must3r_hip_load_weight(self.handle, name.encode(), C.c_void_p(t.data_ptr()),
                                              1 if t.is_cuda else 0, t.dim(), shape))

    def finalize(self, parts):
        check(self.lib.must3r_hip_finalize_weights(self.handle, parts))

    def set_profiling(self, on):
        check(self.lib.must3r_hip_set_profiling(self.handle, 1 if on else 0))

    def get_profile(self, reset=True):
        recs = (ProfRecord * 160)()   # 7 class rows + one row per kernel symbol (names prefixed "k:")
        n = self.lib.must3r_hip_get_profile(self.handle, recs, 160, 1 if reset else 0)
        return {recs[i].name.decode(): {"ms": recs[i].ms, "flops": recs[i].flops, "calls": recs[i].calls}
                for i in range(n)}

    def close(self):
        if self.handle:
            self.lib.must3r_hip_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

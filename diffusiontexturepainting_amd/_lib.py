"""ctypes binding of libdtp.so (include/dtp.h).  There is no fallback: if the HIP library is
missing or an entry point fails, the caller gets an exception."""
import ctypes as C
import os

import torch  # noqa: F401  -- must come first: libdtp.so has to bind to the HIP runtime torch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DTP_LIB") or os.path.join(_HERE, "libdtp.so")  # DTP_LIB: A/B another build of the same ABI
_lib = None
MAX_SLOTS = 16  # DTP_MAX_SLOTS
# samplers of the stamp loop by the reference's names (stable_diffusion_pipeline.py:115-127): DTP_SCHED_* of include/dtp.h
SCHEDULERS = {"DDIM": 0, "DPM": 1, "LMSD": 2}
SCHED_ROW = 8  # DTP_SCHED_ROW


def scheduler_id(name):
    """DTP_SCHED_* of a scheduler name; ValueError naming the supported set for anything else (EulerA and PNDM are not ported)."""
    if name not in SCHEDULERS:
        raise ValueError(f"scheduler {name!r} is not supported: choose one of {', '.join(SCHEDULERS)}")
    return SCHEDULERS[name]


class DtpError(RuntimeError):
    pass


class Settings(C.Structure):
    _fields_ = [("steps", C.c_int), ("context_pad", C.c_int), ("tg_steps", C.c_int), ("cfg_weight", C.c_float),
                ("tg_weight", C.c_float), ("composite", C.c_int), ("output_u8", C.c_int)]


STROKE_MODES = {"inpaint": 0, "erase": 1, "overpaint": 2}  # DTP_STROKE_*: the Kit app's brush modes (manager.py:70)


class StrokeStamp(C.Structure):  # dtp_stroke_stamp
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("mode", C.c_int), ("slot", C.c_int), ("seed", C.c_uint64)]


class StrokeOpts(C.Structure):  # dtp_stroke_opts
    _fields_ = [("wrap", C.c_int), ("margin", C.c_int), ("over_y", C.c_int), ("over_x", C.c_int), ("max_group", C.c_int),
                ("sample_vae", C.c_int), ("strength", C.c_double)]


class MeshStamp(C.Structure):  # dtp_mesh_stamp
    _fields_ = [("pos", C.c_float * 3), ("normal", C.c_float * 3), ("prev", C.c_float * 3), ("fov", C.c_float), ("mode", C.c_int),
                ("slot", C.c_int), ("seed", C.c_uint64)]


class MeshStrokeOpts(C.Structure):  # dtp_mesh_stroke_opts
    _fields_ = [("flip_normals", C.c_int), ("margin", C.c_int), ("over_y", C.c_int), ("over_x", C.c_int), ("sample_vae", C.c_int),
                ("strength", C.c_double)]


class Ray(C.Structure):  # dtp_ray
    _fields_ = [("origin", C.c_float * 3), ("dir", C.c_float * 3)]


class MeshHit(C.Structure):  # dtp_mesh_hit
    _fields_ = [("face", C.c_int), ("w", C.c_float * 3), ("pos", C.c_float * 3), ("normal", C.c_float * 3), ("uv", C.c_float * 2),
                ("t", C.c_float)]


class PathState(C.Structure):  # dtp_path_state
    _fields_ = [("has_prev", C.c_int), ("prev", C.c_float * 3)]


PICK_MAX_RAYS = 4096


class ViewCam(C.Structure):  # dtp_view_cam
    _fields_ = [("m", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("near", C.c_float)]


class ViewOpts(C.Structure):  # dtp_view_opts
    _fields_ = [("cull", C.c_int), ("flip_normals", C.c_int), ("shade", C.c_int), ("ambient", C.c_float), ("unpainted", C.c_uint8 * 3),
                ("background", C.c_uint8 * 4)]


VIEW_MAX = 4096  # the largest side of a view's frame
VIEW_SAMPLES = (1, 2, 4)  # the sides of the sample grid of a pixel (dtp_mesh_view_aa); samples * side <= VIEW_MAX


def view_samples_check(samples, H, W):
    """ValueError for a `samples` that dtp_mesh_view_aa refuses at H x W; -> samples as an int."""
    if isinstance(samples, bool) or not isinstance(samples, int) or samples not in VIEW_SAMPLES:
        raise ValueError(f"samples = {samples!r}: choose 1, 2 or 4 (the side of the sample grid of a pixel)")
    if samples * H > VIEW_MAX or samples * W > VIEW_MAX:
        raise ValueError(f"samples = {samples} at size ({H}, {W}): samples * side must not exceed {VIEW_MAX}")
    return samples


VIEW_MAX_ANISO = 16  # the most taps of an anisotropic sample (dtp_mesh_view_aniso)


def view_anisotropy_check(anisotropy, filter, want_taps, least=1):
    """ValueError for what render_view / ops.mesh_view refuse of `anisotropy` and `want_taps`; -> anisotropy as an int.  least: the
    smallest anisotropy that goes to dtp_mesh_view_aniso (below it, want_taps has no map to return)."""
    if isinstance(anisotropy, bool) or not isinstance(anisotropy, int) or not 1 <= anisotropy <= VIEW_MAX_ANISO:
        raise ValueError(f"anisotropy = {anisotropy!r}: an integer in 1..{VIEW_MAX_ANISO} (the most taps along the footprint)")
    if anisotropy >= least and filter != "trilinear":
        raise ValueError(f"anisotropy = {anisotropy} needs filter='trilinear' (the taps are trilinear samples)")
    if want_taps and anisotropy < least:
        raise ValueError("want_taps needs anisotropy > 1")
    return anisotropy


SELECT_OPS = {"replace": 0, "add": 1, "subtract": 2}  # DTP_SELECT_*
EXTEND_HOWS = {"rings": 0, "shrink": 1, "linked": 2, "charts": 3}  # DTP_EXTEND_*


class MipLevels(C.Structure):  # dtp_mip_levels
    _fields_ = [("levels", C.c_int), ("h", C.c_int * 16), ("w", C.c_int * 16), ("offset", C.c_uint64 * 16), ("bytes", C.c_uint64)]


class DeltaSizes(C.Structure):  # dtp_delta_sizes
    _fields_ = [(n, C.c_int) for n in ("tiles_x", "tiles_y", "n_tiles", "n_groups", "capacity")] + \
        [(n, C.c_uint64) for n in ("shadow_bytes", "stale_bytes", "flag_bytes", "group_bytes", "ids_bytes", "tiles_bytes", "counts_bytes",
                                   "host_ids_offset", "host_tiles_offset", "host_bytes")]


class ProfRow(C.Structure):
    _fields_ = [("kind", C.c_int), ("launches", C.c_int), ("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


_SHAPES = [(128, 128), (128, 64), (64, 64), (64, 128)]
PROF_KINDS = [f"gemm_kernel<{_SHAPES[i & 3][0]}, {_SHAPES[i & 3][1]}, {2 + i // 4}>" for i in range(12)] + \
    ["attention_kernel", "groupnorm (gn_stats+gn_apply | gn_fused)", "layernorm_kernel", "concat_kernel / small elementwise",
     "softmax_rows_kernel", "conv_halo_kernel<8, 16, 64>", "conv_halo_kernel<8, 16, 128>", "conv_halo_kernel<8, 8, 64>",
     "conv_halo_kernel<8, 8, 128>", "gemm_kernel<256, 128, 2>", "gemm_kernel<256, 128, 3>", "gemm_kernel<128, 256, 2>",
     "gemm_kernel<128, 256, 3>", "gemm_wide_kernel<256, 256>", "gemm_wide_kernel<256, 320>", "gemm_fp8_kernel"] + \
    [f"gemm_kernel<{_SHAPES[i & 3][0]}, {_SHAPES[i & 3][1]}, {2 + i // 4}, 2>" for i in range(8)] + \
    [f"gemm_kernel<{_SHAPES[i & 3][0]}, {_SHAPES[i & 3][1]}, 3, 1, {(4, 8)[i // 4]}>" for i in range(8)] + \
    ["xattn_kernel (cross-attention GEMM pair)", "conv_halo_kernel<8, 8, 64, 3 images>", "conv_halo_kernel<8, 8, 128, 3 images>",
     "lnlin_kernel (activation-stationary LayerNorm-folded Linear / GEGLU)", "convws_kernel<8, 8, 3 images>", "convws_kernel<16, 16>", "convws_kernel<8, 16, 2 n-tiles>", "convws_kernel<8, 16, 2 n-tiles, 2 workgroups per CU>",
     "gemmws_kernel (weight-streaming dense GEMM)", "gemm_f8f8_kernel (two-operand e4m3 GEMM)", "quant8_kernel (e4m3 quantise pass)"]


class GemmDesc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("W", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p), ("R", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("lda", C.c_int), ("ldw", C.c_int), ("ldc", C.c_int), ("ldr", C.c_int),
                ("conv", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int), ("Cin", C.c_int),
                ("stride", C.c_int), ("pad", C.c_int), ("upsample2x", C.c_int),
                ("flags", C.c_int), ("tile", C.c_int), ("splits", C.c_int), ("lns", C.c_void_p), ("ln_eps", C.c_float),
                ("A2", C.c_void_p), ("lda2", C.c_int), ("Cin2", C.c_int), ("Wcb", C.c_void_p),
                ("batch", C.c_int), ("a_bs", C.c_int64), ("w_bs", C.c_int64), ("c_bs", C.c_int64), ("r_bs", C.c_int64),
                ("bias_bs", C.c_int), ("lns_bs", C.c_int), ("sm_valid", C.c_int),
                ("st_out", C.c_void_p), ("st_in", C.c_void_p), ("st_parts", C.c_int), ("st_parts_out", C.c_int),
                ("W8", C.c_void_p), ("ldw8", C.c_int), ("a_scale", C.c_float), ("w_scale", C.c_float), ("gn_cpg", C.c_int), ("Wfr", C.c_void_p),
                ("A8", C.c_void_p), ("lda8", C.c_int), ("A2_8", C.c_void_p), ("lda2_8", C.c_int), ("C8", C.c_void_p), ("ldc8", C.c_int),
                ("c_scale", C.c_float), ("a2_scale", C.c_float)]


GF_BIAS, GF_BIAS_M, GF_RESID, GF_GEGLU, GF_GELU, GF_QUICKGELU, GF_OUT_F32, GF_SILU, GF_LNFOLD = 1, 2, 4, 8, 64, 128, 256, 512, 1024
GF_SOFTMAX16 = 4096
GF_ROWSTATS = 2048
GF_GNSTATS = 1 << 24
GF_RAGGED = 1 << 25  # convws tiles 53 / 54: partial 8 x 16 pixel tiles, cropped upsample window

# every symbol include/dtp.h declares: name -> (restype, argtypes)
_vp, _i, _f, _i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
SYMBOLS = {
    "dtp_abi_version": (_i, []),
    "dtp_last_error": (C.c_char_p, []),
    "dtp_create": (_i, [_i, _i, _i, C.POINTER(_vp)]),
    "dtp_destroy": (None, [_vp]),
    "dtp_load_tensor": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(_i64), _i]),
    "dtp_finalize_weights": (_i, [_vp]),
    "dtp_vae_encode": (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
    "dtp_unet": (_i, [_vp, _vp, _f, _vp, _vp, _i, _vp]),
    "dtp_vae_decode": (_i, [_vp, _vp, _vp, _i, _vp]),
    "dtp_set_brush": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "dtp_set_conditioning": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "dtp_get_conditioning": (_i, [_vp, _vp, _vp, _vp]),
    "dtp_stamp": (_i, [_vp, _vp, C.POINTER(Settings), _vp, _vp, _vp, _i, _vp]),
    "dtp_stamp_slots": (_i, [_vp, _vp, C.POINTER(Settings), _vp, _vp, _vp, _i, C.POINTER(_i), _vp]),
    "dtp_stamp_mixed": (_i, [_vp, _vp, C.POINTER(Settings), _vp, _vp, _vp, _i, C.POINTER(_i), _vp]),
    "dtp_set_brush_slot": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp]),
    "dtp_set_conditioning_slot": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "dtp_get_conditioning_slot": (_i, [_vp, _i, _vp, _vp, _vp]),
    "dtp_ddim_tables": (_i, [_i, C.POINTER(_i64), C.POINTER(_f), C.POINTER(_f)]),
    "dtp_last_stamp_times": (_i, [_vp, C.POINTER(_f * 3)]),
    "dtp_last_stamp_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "dtp_last_stamp_unet_rows": (_i, [_vp, C.POINTER(_i)]),
    "dtp_profile": (_i, [_vp, _i]),
    "dtp_profile_rows": (_i, [_vp, C.POINTER(ProfRow), _i, C.POINTER(_i)]),
    "dtp_profile_dump": (_i, [_vp, C.c_char_p]),
    "dtp_set_option": (_i, [_vp, C.c_char_p, _i]),
    "dtp_last_stamp_finite": (_i, [_vp, C.POINTER(_i)]),
    "dtp_op_gemm": (_i, [C.POINTER(GemmDesc), _vp]),
    "dtp_op_gemm_f8f8": (_i, [C.POINTER(GemmDesc), _vp]),
    "dtp_op_quant_e4m3": (_i, [_vp, _i, _vp, _i, _i, _f, _i, _vp, _i, _vp, _i, _i, _f, _i, _i, _vp, _i, _f, _vp]),
    "dtp_op_pack_linear": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "dtp_op_pack_conv": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "dtp_op_rowsum": (_i, [_vp, _i, _i, _vp, _i, _vp]),
    "dtp_op_quantize_w8": (_i, [_vp, _i, _i, _i, _vp, _i, C.POINTER(_f), _vp]),
    "dtp_op_pack_conv_cb": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "dtp_op_groupnorm_apply": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "dtp_op_groupnorm_stats_apply": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "dtp_op_pack_conv_ws": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "dtp_op_pack_conv_ws_elems": (C.c_longlong, [_i, _i, _i]),
    "dtp_op_pack_conv_ws_ups4": (_i, [_vp, _vp, _i, _i, _vp]),
    "dtp_op_pack_conv_ws_ups4_elems": (C.c_longlong, [_i, _i]),
    "dtp_op_conv_ups4": (_i, [C.POINTER(GemmDesc), _vp, _vp]),
    "dtp_op_conv_ws_supported": (_i, [C.POINTER(GemmDesc), _vp, _i, _i]),
    "dtp_op_pack_linear_ws": (_i, [_vp, _i, _vp, _i, _i, _vp]),
    "dtp_op_pack_linear_ws_elems": (C.c_longlong, [_i, _i]),
    "dtp_op_groupnorm": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "dtp_op_measure_peaks": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dtp_op_reduce_groupnorm": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "dtp_op_xattn": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "dtp_op_reduce_groupnorm_cx": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _i, _vp]),
    "dtp_op_xattn_ct": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "dtp_op_gn_fold_weights": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "dtp_op_ffchain": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "dtp_op_xchain": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "dtp_op_gn_linear": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp]),
    "dtp_op_layernorm": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _f, _vp]),
    "dtp_op_attention": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i64, _i64, _i64, _i64, _f, _vp]),
    "dtp_op_attention_dma": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i64, _i64, _i64, _i64, _f, _i, _vp]),
    "dtp_op_softmax_rows": (_i, [_vp, _i, _vp, _i, _i, _i, _f, _vp]),
    "dtp_op_attention_fp8": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i64, _i64, _i64, _i64, _f, _f, _f, _vp]),
    "dtp_op_dilate": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "dtp_op_dilate_pads": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(_i), _vp]),
    "dtp_scheduler_tables": (_i, [_i, _i, C.POINTER(_i), C.POINTER(_f), C.POINTER(_f), C.POINTER(_f), C.POINTER(_f)]),
    "dtp_op_sched_step": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "dtp_stamp_strength": (_i, [_vp, _vp, C.POINTER(Settings), _vp, _vp, _vp, C.c_double, _vp, _i, C.POINTER(_i), _vp]),
    "dtp_strength_schedule": (_i, [_i, _i, C.c_double, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f)]),
    "dtp_op_strength_init": (_i, [_vp, _vp, _f, _f, _vp, C.c_longlong, _vp]),
    "dtp_stamp_seeded": (_i, [_vp, _vp, C.POINTER(Settings), C.POINTER(C.c_uint64), _i, C.c_double, _vp, _i, C.POINTER(_i), _vp]),
    "dtp_op_stamp_noise": (_i, [C.c_uint64, _i, _vp, C.c_longlong, _vp]),
    "dtp_philox4x32": (_i, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "dtp_refit_stage": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(_i64), _i]),
    "dtp_refit_lora": (_i, [_vp, _f]),
    "dtp_last_refit_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f)]),
    "dtp_op_lora_refit": (_i, [_vp, _vp, _vp, _i, _f, _vp, _vp, _i, _i, _i, _i, _vp]),
    "dtp_stroke": (_i, [_vp, _vp, _i, _i, C.POINTER(StrokeStamp), _i, C.POINTER(Settings), C.POINTER(StrokeOpts), _vp, _vp]),
    "dtp_stroke_plan": (_i, [_i, _i, _i, _i, C.POINTER(StrokeStamp), _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "dtp_last_stroke_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "dtp_op_stroke_gather": (_i, [_vp, _i, _i, _vp, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i, _i, _i, _vp]),
    "dtp_op_stroke_paste": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i, _vp]),
    "dtp_mesh_create": (_i, [_vp, _vp, _i, _vp, _i, _vp, C.POINTER(_vp)]),
    "dtp_mesh_destroy": (_i, [_vp]),
    "dtp_mesh_camera": (_i, [C.POINTER(_f * 3), C.POINTER(_f * 3), C.POINTER(_f * 3), _f, C.POINTER(_f * 12)]),
    "dtp_mesh_stroke": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(MeshStamp), _i, C.POINTER(Settings), C.POINTER(MeshStrokeOpts), _vp, _vp]),
    "dtp_op_mesh_render": (_i, [_vp, C.POINTER(_f * 12), _f, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "dtp_op_mesh_backproject": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp]),
    "dtp_mesh_stroke_bleed": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(MeshStamp), _i, C.POINTER(Settings), C.POINTER(MeshStrokeOpts), _vp, _i, _vp]),
    "dtp_mesh_bleed": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_i * 4), _vp]),
    "dtp_op_mesh_coverage": (_i, [_vp, _i, _i, _vp, _vp]),
    "dtp_mesh_bleed_offsets": (_i, [_i, C.POINTER(_i), C.POINTER(C.c_byte)]),
    "dtp_mesh_pick": (_i, [_vp, C.POINTER(Ray), _i, _vp, _vp]),
    "dtp_mesh_ray_frame": (_i, [C.POINTER(_f * 3), C.POINTER(_f * 3), C.POINTER(_f * 12)]),
    "dtp_mesh_path_plan": (_i, [_vp, _i, _f, C.POINTER(PathState), _vp, _vp, _vp, _i, C.POINTER(_i)]),
    "dtp_op_mesh_pick": (_i, [_vp, C.POINTER(Ray), _i, _vp, _vp]),
    "dtp_view_camera": (_i, [C.POINTER(_f * 3), C.POINTER(_f * 3), C.POINTER(_f * 3), _f, _i, _i, _f, C.POINTER(ViewCam)]),
    "dtp_view_rays": (_i, [C.POINTER(ViewCam), _i, _i, _vp, _i, _vp]),
    "dtp_mesh_view": (_i, [_vp, _vp, _i, _i, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _vp, _vp, _vp, _vp]),
    "dtp_op_mesh_view": (_i, [_vp, _vp, _i, _i, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _vp, _vp, _vp, _i, _vp]),
    "dtp_mip_layout": (_i, [_i, _i, C.POINTER(MipLevels)]),
    "dtp_texture_mips": (_i, [_vp, _i, _i, _vp, C.c_uint64, _vp]),
    "dtp_mesh_view_mips": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _vp, _vp, _vp, _vp, _vp]),
    "dtp_mesh_view_clip": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _i, _vp, _vp, _vp, _vp, _vp]),
    "dtp_op_mesh_view_clip": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "dtp_mesh_view_aa": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dtp_op_mesh_view_aa": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i,
                                 _vp]),
    "dtp_mesh_view_aniso": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp]),
    "dtp_op_mesh_view_aniso": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(ViewCam), _i, _i, C.POINTER(ViewOpts), _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _i, _vp]),
    "dtp_mesh_select": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp]),
    "dtp_mesh_stroke_masked": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(MeshStamp), _i, C.POINTER(Settings), C.POINTER(MeshStrokeOpts), _vp, _i, _vp, _i,
                                    _vp]),
    "dtp_view_tint": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, C.POINTER(C.c_uint8 * 3), _i, _vp]),
    "dtp_op_mesh_backproject_masked": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _i, _vp]),
    "dtp_topology_build": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, C.POINTER(_i * 3)]),
    "dtp_mesh_topology": (_i, [_vp, C.POINTER(_i * 3), _vp]),
    "dtp_mesh_topology_labels": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "dtp_mesh_select_extend": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "dtp_mesh_stroke_occluded": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(MeshStamp), _i, C.POINTER(Settings), C.POINTER(MeshStrokeOpts), _vp, _i, _vp, _i,
                                      _f, _vp]),
    "dtp_op_mesh_backproject_occluded": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _i, _f, _f, _vp]),
    "dtp_journal_create": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(_vp)]),
    "dtp_journal_destroy": (_i, [_vp]),
    "dtp_journal_begin": (_i, [_vp, _vp]),
    "dtp_journal_end": (_i, [_vp, _vp]),
    "dtp_journal_touch": (_i, [_vp, C.POINTER(_i), _i, _vp]),
    "dtp_journal_undo": (_i, [_vp, _vp]),
    "dtp_journal_redo": (_i, [_vp, _vp]),
    "dtp_journal_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_uint64)]),
    "dtp_journal_record_info": (_i, [_vp, _i, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(_i)]),
    "dtp_op_journal_tiles": (_i, [_vp, _i, C.POINTER(_i), _i, C.POINTER(_i)]),
    "dtp_journal_window_tiles": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_i), _i, C.POINTER(_i)]),
    "dtp_delta_layout": (_i, [_i, _i, _i, C.POINTER(DeltaSizes)]),
    "dtp_delta_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "dtp_delta_destroy": (_i, [_vp]),
    "dtp_delta_reset": (_i, [_vp, _vp]),
    "dtp_delta_scan": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "dtp_delta_device": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "dtp_delta_host": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "dtp_delta_pull": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    "dtp_op_delta_state": (_i, [_vp, _vp, _vp, _vp]),
}


def load():
    """Load libdtp.so and bind every declared symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DtpError(f"{LIB_PATH} not found -- run `python -m diffusiontexturepainting_amd.build` "
                       "(there is no CPU or PyTorch fallback for the stamp path)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        if os.environ.get("DTP_LIB") and not hasattr(lib, name):
            continue  # A/B against an older build of the ABI: entry points it lacks simply stay unbound
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().dtp_last_error()
        raise DtpError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device/host pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())

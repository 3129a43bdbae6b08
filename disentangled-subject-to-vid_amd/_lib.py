"""ctypes binding of libs2v_hip.so (C ABI: include/s2v_hip.h).  There is NO fallback: if the HIP library is
missing or a call fails, this module raises."""
import ctypes
import os

import torch  # noqa: F401  (must be imported first so the process-wide HIP runtime is torch's libamdhip64)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("S2V_LIB") or os.path.join(_HERE, "libs2v_hip.so")  # S2V_LIB: an experiment build of the SAME library (tools/ab_step.sh)

DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
TORCH_DTYPE = {DTYPE_F32: torch.float32, DTYPE_BF16: torch.bfloat16, DTYPE_F16: torch.float16}
DTYPE_OF = {torch.float32: DTYPE_F32, torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_F16}
# ModelConfigC.reserved[0]: the kind of context s2v_create makes (include/s2v_hip.h, S2V_CTX_*)
CTX_MODEL, CTX_ATTN_WEIGHTS, CTX_ATTN_WORKSPACE = 0, 1, 2
# ModelConfigC.reserved[1]: lora_runtime_rank in the low 16 bits; bit 16 asks an fp8 weight_format for the 16-bit adapter branch beside its
# e4m3 weights (include/s2v_hip.h, S2V_LORA_RANK_MASK / S2V_LORA_FP8_BRANCH)
LORA_RANK_MASK, LORA_FP8_BRANCH = 0xFFFF, 1 << 16


class ModelConfigC(ctypes.Structure):
    _fields_ = [
        ("num_layers", ctypes.c_int32), ("num_heads", ctypes.c_int32), ("in_channels", ctypes.c_int32),
        ("out_channels", ctypes.c_int32), ("patch_size", ctypes.c_int32), ("time_embed_dim", ctypes.c_int32),
        ("text_embed_dim", ctypes.c_int32), ("use_rope", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("norm_eps", ctypes.c_float), ("force_simple", ctypes.c_int32), ("weight_format", ctypes.c_int32),
        ("lora_adaln_scope", ctypes.c_int32), ("attn_p_format", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2),
    ]


class SchedCoefC(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("guidance", ctypes.c_float)] + [
        (n, ctypes.c_float) for n in ("c_x0_x", "c_x0_v", "a_t", "b_t", "m1", "m2", "m3", "m4", "mn", "guidance_subject")
    ]


class BlendC(ctypes.Structure):
    """s2v_blend: the masked step's record per video (add_noise scalars of its next timestep, last-step flag, the level up to which cells
    are kept: 0 for a 0 / 1 mask)"""
    _fields_ = [("sqrt_alpha", ctypes.c_float), ("sqrt_one_minus_alpha", ctypes.c_float), ("last", ctypes.c_int32), ("keep_max", ctypes.c_int32)]


SCHED_CFG_PAIR, SCHED_NP_F32, SCHED_OUT_F32, SCHED_TRIPLE = 1, 2, 4, 8   # s2v_sched_step flags (bit3: the subject-guidance triple [3, n])
MASK_DTYPE_U8 = 3   # S2V_MASK_DTYPE_U8: a uint8 pixel mask, non-zero = repaint; for s2v_map_to_latent: levels 0..255


class S2VError(RuntimeError):
    pass


_lib = None

_P, _I32, _I64, _F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
_SIGS = {
    "s2v_create": [ctypes.POINTER(ModelConfigC), ctypes.POINTER(_P)],
    "s2v_load_weight": [_P, ctypes.c_char_p, _P, ctypes.POINTER(_I64), _I32, _I32, _P],
    "s2v_merge_lora": [_P, ctypes.c_char_p, _P, _P, _I32, _F, _P],
    "s2v_finalize_weights": [_P, _P],
    "s2v_lora_attach": [_P, ctypes.c_char_p, _P, _P, _I32, _F, _P],
    "s2v_lora_set_scale": [_P, ctypes.c_char_p, _P, _P, _I32, _F, _P],
    "s2v_lora_detach": [_P, _P],
    "s2v_lora_state": [_P, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_F), ctypes.POINTER(_I64)],
    "s2v_weight_arena": [_P, ctypes.POINTER(_P), ctypes.POINTER(_I64)],
    "s2v_weight_slot": [_P, ctypes.c_char_p, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)],
    "s2v_mark_weights_loaded": [_P],
    "s2v_set_geometry": [_P, _I32, _I32, _I32, _I32, _I32],
    "s2v_fp8_qk_active": [_P, ctypes.POINTER(_I32)],
    "s2v_set_rope": [_P, _P, _P, _P],
    "s2v_set_pos_embed": [_P, _P, _P],
    "s2v_set_conditioning": [_P, _P, _P, _P],
    "s2v_set_conditioning_refs": [_P, _P, _P, _I32, _P],
    "s2v_transformer_forward": [_P, _P, _I64, _P, _P, _P],
    "s2v_transformer_forward_videos": [_P, _P, _I32, _P, _P, _P],
    "s2v_block_forward": [_P, _I32, _P, _P, _P, _P, _P, _P, _P, _P],
    "s2v_attn_forward": [_P, _I32, _P, _P, _P, _P, _P],
    "s2v_attn_forward_with": [_P, _P, _I32, _P, _P, _P, _P, _P],
    "s2v_device_bytes": [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)],
    "s2v_sched_step": [_P, ctypes.POINTER(SchedCoefC), _P, _I32, _P, _P, _P, _P, _I64, _I32, _P],
    "s2v_add_noise": [_P, _P, _I64, _F, _F, _P, _I32, _P],
    "s2v_denoise_step": [_P, _P, _F, ctypes.POINTER(SchedCoefC), _P, _P, _I32, _P],
    "s2v_denoise_step_videos": [_P, _P, ctypes.POINTER(_F), ctypes.POINTER(SchedCoefC), _P, _P, _I32, _P],
    "s2v_mask_to_latent": [_P, _I32, _I32, _I32, _I32, _P, _P, _P],
    "s2v_map_to_latent": [_P, _I32, _I32, _I32, _I32, _P, _P, _P],
    "s2v_set_blend": [_P, _P, _P, _P, _I32],
    "s2v_denoise_step_masked": [_P, _P, ctypes.POINTER(_F), ctypes.POINTER(SchedCoefC), ctypes.POINTER(BlendC), _P, _P, _I32, _P],
    "s2v_sched_step_masked": [_P, ctypes.POINTER(SchedCoefC), ctypes.POINTER(BlendC), _P, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32,
                              _I32, _P],
    "s2v_last_noise_pred": [_P, ctypes.POINTER(_P)],
    "s2v_set_conditioning_triples": [_P, _P, _P, _P, _I32, _P],
    "s2v_denoise_step_guided": [_P, _P, ctypes.POINTER(_F), ctypes.POINTER(SchedCoefC), ctypes.POINTER(BlendC), _P, _P, _I32, _P],
    "s2v_denoise_split_begin": [_P, _P, _F, ctypes.POINTER(SchedCoefC), _I32, _I32, _P],
    "s2v_cfg_pair": [_P, ctypes.POINTER(_P), ctypes.POINTER(_I64)],
    "s2v_denoise_split_end": [_P, _P, _P, _P, _P],
    "s2v_denoise_step_cfg_parallel": [_P, _P, _I32, _P, _F, ctypes.POINTER(SchedCoefC), _P, _P, _I32, _P],
    "s2v_profile_enable": [_P, _I32],
    "s2v_profile_read": [_P, ctypes.POINTER(_F), ctypes.POINTER(_I32), _I32],
    "s2v_profile_read_clocks": [_P, ctypes.POINTER(_F), _I32],
    "s2v_op_linear": [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P],
    "s2v_op_linear_planned": [_P, _I32, _P, _I32, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _I32, _I32, _I64, _P],
    "s2v_op_linear_lora": [_P, _P, _P, _P, _P, _I32, _F, _P, _I32, _I32, _I32, _I32, _P, _P, _I32, _P],
    "s2v_op_ff_fp8": [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P],
    "s2v_op_mod_gemv": [_P, _P, _P, _P, _I32, _I32, _I64, _I32, _I32, _P],
    "s2v_op_ln_modulate": [_P, _I32, _P, _I32, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _I32, _I32, _P],
    "s2v_op_tail_norm": [_P, _I32, _P, _I32, _P, _P, _P, _P, _F, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P],
    "s2v_op_qk_norm_rope": [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _F, _P, _P, _I32, _P],
    "s2v_op_v_transpose": [_P, _I32, _I32, _I32, _I32, _P, _I32, _P, _P],
    "s2v_op_attention": [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P],
    "s2v_attn_slow_stats": [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), _I32],
    "s2v_set_attn_p_format": [_P, _I32],
    "s2v_op_attention_fp8qk": [_P, _P, _P, _I64, _P, _I32, _I32, _I32, _P],
    "s2v_op_attention_fp8qk_p16": [_P, _P, _P, _I64, _P, _I32, _I32, _I32, _P],
    "s2v_op_linear_fp8": [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _I64, _P],
    "s2v_op_linear_fp8_lora": [_P, _P, _P, _P, _P, _I32, _F, _P, _I32, _I32, _I32, _I32, _P, _I64, _P],
    "s2v_op_ff_fp8_lora": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _F, _P, _I32, _I32, _I32, _I32, _P, _I64, _P],
}
# step cache (include/s2v_hip.h: s2v_step_cache_*, s2v_time_embedding)
STEP_FULL, STEP_CAPTURE, STEP_REUSE = 0, 1, 2
_SIGS.update({
    "s2v_step_cache_enable": [_P, _I32],
    "s2v_step_cache_arm": [_P, _I32],
    "s2v_step_cache_state": [_P, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I64)],
    "s2v_step_cache_read": [_P, _I32, _P, _P],
    "s2v_time_embedding": [_P, ctypes.POINTER(_F), _I32, _P, _P],
    "s2v_op_step_cache": [_I32, _P, _I64, _P, _I32, _I64, _I32, _P],
})
# attention map (include/s2v_hip.h: s2v_attn_map_*, s2v_op_attn_mass)
_SIGS.update({
    "s2v_attn_map_enable": [_P, _I32, ctypes.POINTER(_I32), _I32],
    "s2v_attn_map_arm": [_P, ctypes.c_uint64],
    "s2v_attn_map_read": [_P, _I32, _P, ctypes.POINTER(_I64), _P],
    "s2v_attn_map_reset": [_P],
    "s2v_op_attn_mass": [_P, _I32, _I32, _I32, _I32, _I32, ctypes.POINTER(_I32), _I32, _P, _I32, _I32, _I32, _P],
    "s2v_op_attn_mass_mean": [_P, _I32, _I32, _I32, _I32, _I64, _P, _P],
})
# attention steering (include/s2v_hip.h: s2v_attn_steer_*, s2v_op_attention_steer)
STEER_MAX_RANGES = 4


class SteerRangeC(ctypes.Structure):
    """s2v_attn_steer_range: keys [k0, k1) weighted by w on the samples whose bit is set in sample_mask"""
    _fields_ = [("k0", ctypes.c_int32), ("k1", ctypes.c_int32), ("w", ctypes.c_float), ("sample_mask", ctypes.c_uint32)]


class SteerRecordC(ctypes.Structure):
    """s2v_attn_steer_record: the operator-level record, ranges as arrays plus the query range [q0, q1)"""
    _fields_ = [("n", ctypes.c_int32), ("q0", ctypes.c_int32), ("q1", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("k0", ctypes.c_int32 * 4), ("k1", ctypes.c_int32 * 4), ("w", ctypes.c_float * 4), ("sample_mask", ctypes.c_uint32 * 4)]


_SIGS.update({
    "s2v_attn_steer_enable": [_P, _I32],
    "s2v_attn_steer_set": [_P, _I32, ctypes.POINTER(SteerRangeC)],
    "s2v_attn_steer_arm": [_P, ctypes.c_uint64],
    "s2v_op_attention_steer": [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, ctypes.POINTER(SteerRecordC), _P],
})
# local attention in time (include/s2v_hip.h: s2v_attn_local_*, s2v_op_attention_local)
_SIGS.update({
    "s2v_attn_local_enable": [_P, _I32],
    "s2v_attn_local_set": [_P, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)],
    "s2v_attn_local_arm": [_P, ctypes.c_uint64],
    "s2v_op_attention_local": [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32), _P],
    "s2v_attn_local_set_box": [_P, _I32, _I32] + [ctypes.POINTER(_I32)] * 4,
    "s2v_op_attention_box": [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32] + [ctypes.POINTER(_I32)] * 4 + [_P],
})


def i32_array(values):
    """a ctypes int32 array of a sequence or tensor of integers (the row tables of local attention)"""
    vals = [int(v) for v in (values.tolist() if hasattr(values, "tolist") else values)]
    return (_I32 * max(1, len(vals)))(*vals)


# steering maps (include/s2v_hip.h: s2v_attn_steer_set_maps, s2v_op_attention_steer_map)
STEER_MAP_MAX_PLANES = 16
STEER_MAP_BATCH = 8


class SteerMapRangeC(ctypes.Structure):
    """s2v_attn_steer_map_range: keys [k0, k1) weighted per query row by plane[b] on sample b (-1: not on that sample)"""
    _fields_ = [("k0", ctypes.c_int32), ("k1", ctypes.c_int32), ("plane", ctypes.c_int8 * 8)]


class SteerMapRecordC(ctypes.Structure):
    """s2v_attn_steer_map_record: the operator-level record, ranges as arrays plus the query range [q0, q1) and the plane count"""
    _fields_ = [("n", ctypes.c_int32), ("q0", ctypes.c_int32), ("q1", ctypes.c_int32), ("k0", ctypes.c_int32 * 4), ("k1", ctypes.c_int32 * 4),
                ("plane", (ctypes.c_int8 * 8) * 4), ("n_planes", ctypes.c_int32)]


_SIGS.update({
    "s2v_attn_steer_set_maps": [_P, _I32, ctypes.POINTER(SteerMapRangeC), _I32, ctypes.POINTER(_F)],
    "s2v_op_attention_steer_map": [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, ctypes.POINTER(SteerMapRecordC), ctypes.POINTER(_F), _P],
    "s2v_attn_steer_map_wave_flags": [_I32, _I32, _I32, _I32, ctypes.POINTER(ctypes.c_int8), ctypes.POINTER(_F), ctypes.POINTER(_I32)],
})
# temporal windows (include/s2v_hip.h: s2v_set_windows, s2v_denoise_step_windows, s2v_op_window_blend)
_SIGS.update({
    "s2v_set_windows": [_P, _I32, _I32, _I32, ctypes.POINTER(_F)],
    "s2v_denoise_step_windows": [_P, _P, _F, ctypes.POINTER(SchedCoefC), _P, _P, _I32, _P],
    "s2v_op_window_blend": [_P, _P, _P, _P, _F, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P],
})
# guidance rescale (include/s2v_hip.h: s2v_set_guidance_rescale, s2v_guidance_rescale_read, s2v_op_cfg_stats, the RESCALE step forms)
SCHED_RESCALE = 16                                # s2v_sched_step_rescale / s2v_sched_step_masked_rescale flags bit4
CFG_STATS_CHUNK, CFG_LOG_STEPS, CFG_LOG_COLS = 4096, 1024, 4   # S2V_CFG_STATS_CHUNK, S2V_CFG_LOG_STEPS, S2V_MAX_BATCH / 2
_SIGS.update({
    "s2v_set_guidance_rescale": [_P, ctypes.POINTER(_F), _I32],
    "s2v_guidance_rescale_read": [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_F), ctypes.POINTER(_F), ctypes.POINTER(_I32)],
    "s2v_op_cfg_stats": [_P, _I32, _I32, _I64, ctypes.POINTER(_F), ctypes.POINTER(_F), ctypes.POINTER(_F), ctypes.POINTER(ctypes.c_double),
                         ctypes.POINTER(_F), _I32, _P],
    "s2v_sched_step_rescale": [_P, ctypes.POINTER(SchedCoefC), _P, _I32, _P, _P, _P, _P, _I64, _I32, _P, _P],
    "s2v_sched_step_masked_rescale": [_P, ctypes.POINTER(SchedCoefC), ctypes.POINTER(BlendC), _P, _I32, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32,
                                      _I32, _I32, _P, _P],
})
# replicas over RCCL behind the C ABI (csrc/rccl.hip); RCCL itself is bound at first use
_SIGS.update({
    "s2v_rccl_available": [],
    "s2v_rccl_unique_id": [_P],
    "s2v_rccl_comm_create": [_P, _I32, _I32, ctypes.POINTER(_P)],
    "s2v_rccl_bcast": [_P, _P, _I64, _I32, _P],
    "s2v_rccl_allgather": [_P, _P, _P, _I64, _P],
    "s2v_bcast_weights": [_P, _P, _I32, _P],
    "s2v_rccl_alltoallv": [_P, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), _P],
})
# Ulysses sequence parallelism (include/s2v_hip.h: s2v_set_shard ... s2v_denoise_step_ulysses)
SHARD_QKV_EXCHANGE, SHARD_O_EXCHANGE, SHARD_NOISE_GATHER = 1, 2, 3
_SIGS.update({
    "s2v_set_shard": [_P, _I32, _I32],
    "s2v_shard_layout": [_P, ctypes.POINTER(_I32)],
    "s2v_shard_buffers": [_P, _I32, ctypes.POINTER(_P), ctypes.POINTER(_P)] + [ctypes.POINTER(_I64)] * 4,
    "s2v_shard_step_begin": [_P, _P, _F, ctypes.POINTER(SchedCoefC), ctypes.POINTER(_I32), _P],
    "s2v_shard_step_resume": [_P, ctypes.POINTER(_I32), _P],
    "s2v_shard_step_end": [_P, _P, _P, _P, _P],
    "s2v_denoise_step_ulysses": [_P, _P, _P, _F, ctypes.POINTER(SchedCoefC), _P, _P, _P],
})
# VAE entry points are registered by vae.py through register_sigs()


def register_sigs(sigs):
    _SIGS.update(sigs)
    if _lib is not None:
        _apply_sigs(_lib, sigs)


def _apply_sigs(lib, sigs):
    for name, argtypes in sigs.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int


def lib():
    """Load the shared library (once).  Raises S2VError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise S2VError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
                           "There is no CPU fallback.")
        l = ctypes.CDLL(LIB_PATH)
        _apply_sigs(l, _SIGS)
        l.s2v_last_error.restype = ctypes.c_char_p
        l.s2v_version.restype = ctypes.c_char_p
        l.s2v_destroy.argtypes = [_P]
        l.s2v_destroy.restype = None
        l.s2v_rccl_comm_destroy.argtypes = [_P]
        l.s2v_rccl_comm_destroy.restype = None
        _lib = l
    return _lib


_diag = None
DIAG_LIB_PATH = os.path.join(_HERE, "libs2v_hip_diag.so")


def diag_lib():
    """libs2v_hip_diag.so: the same sources built with -DS2V_DIAG (A/B reference kernels, stall accounting, ablations and their
    knobs s2v_set_gemm_impl / s2v_set_attn_variant / s2v_debug_read / s2v_attn_debug_read).  Only tools/ and the race-screen
    test load it (`python disentangled-subject-to-vid_amd/build.py --diag`); the product never does."""
    global _diag
    if _diag is None:
        if not os.path.exists(DIAG_LIB_PATH):
            raise S2VError(f"{DIAG_LIB_PATH} is missing: build it with `python {os.path.join(_HERE, 'build.py')} --diag`")
        l = ctypes.CDLL(os.environ.get("S2V_DIAG_LIB", DIAG_LIB_PATH))  # S2V_DIAG_LIB: an experiment build (tools/g4_ablate.sh)
        _apply_sigs(l, {k: v for k, v in _SIGS.items() if k.startswith("s2v_op_")})
        l.s2v_last_error.restype = ctypes.c_char_p
        for name in ("s2v_set_gemm_impl", "s2v_set_attn_variant"):
            getattr(l, name).argtypes = [ctypes.c_int]
        _diag = l
    return _diag


def check(rc):
    if rc != 0:
        raise S2VError(f"s2v call failed ({rc}): {lib().s2v_last_error().decode()}")


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise S2VError("tensor must live on the GPU")
    if not t.is_contiguous():
        raise S2VError("tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())

"""Loader of the HIP shared library (the only compute path; there is no CPU fallback)."""
from __future__ import annotations

import ctypes
import os

from . import LIB_PATH, TEST_LIB_PATH

_lib = None
_test_lib = None

c_void_p, c_int, c_float, c_char_p = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_char_p
f32p = ctypes.POINTER(ctypes.c_float)
i32p = ctypes.POINTER(ctypes.c_int32)
i64p = ctypes.POINTER(ctypes.c_int64)
u16p = ctypes.POINTER(ctypes.c_uint16)
i16p = ctypes.POINTER(ctypes.c_int16)


class SlotParamsC(ctypes.Structure):
    """q3e_slot_params (include/qwen3tts_engine.h)."""
    _fields_ = [("max_frames", ctypes.c_int32), ("temperature", ctypes.c_float), ("top_k", ctypes.c_int32),
                ("top_p", ctypes.c_float), ("cp_temperature", ctypes.c_float), ("cp_top_k", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("utt", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class KernelSlotParamsC(ctypes.Structure):
    """q3::SlotParams (csrc/q3_kernels.h): the entry the sampling kernels read per row; test hooks only."""
    _fields_ = [("max_frames", ctypes.c_int32), ("t_temp", ctypes.c_float), ("t_top_k", ctypes.c_int32),
                ("t_top_p", ctypes.c_float), ("c_temp", ctypes.c_float), ("c_top_k", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("no_row", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("prompt", ctypes.c_int32)]


class SlotRulesC(ctypes.Structure):
    """q3e_slot_rules (include/qwen3tts_engine.h)."""
    _fields_ = [("rep_penalty", ctypes.c_float), ("rep_window", ctypes.c_int32), ("eos_boost", ctypes.c_float),
                ("eos_force", ctypes.c_float), ("min_frames", ctypes.c_int32), ("cp_top_p", ctypes.c_float),
                ("reserved", ctypes.c_int32 * 2)]


class KernelSlotRulesC(ctypes.Structure):
    """q3::SlotRules (csrc/q3_kernels.h): the entry the sampling kernels read per row; test hooks only."""
    _fields_ = [("rep_penalty", ctypes.c_float), ("rep_window", ctypes.c_int32), ("eos_boost", ctypes.c_float),
                ("eos_force", ctypes.c_float), ("min_past", ctypes.c_int32), ("cp_top_p", ctypes.c_float)]


def _sig(lib, name, restype, argtypes):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = restype, argtypes


def load(path: str | None = None):
    """dlopen libqwen3tts.so and declare every C-ABI signature of include/*.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("QWEN3TTS_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: build it with `python -m qwen3_tts_axera_russian_amd.build` "
                           "(the HIP library is the only compute path)")
    # One HIP hardware queue for this process (csrc/q3_common.cpp): a process-wide runtime policy, so the
    # entry point exports it -- before the first HIP call of the process; a value the user exported wins.
    if os.environ.get("Q3_KEEP_HW_QUEUES", "0") in ("", "0"):
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "1")
    lib = ctypes.CDLL(p)
    # include/qwen3tts_talker.h
    _sig(lib, "wrapper_backend_init", None, [])
    _sig(lib, "wrapper_backend_free", None, [])
    _sig(lib, "wrapper_load_model", c_void_p, [c_char_p, c_int])
    _sig(lib, "wrapper_load_model_aux", c_void_p, [c_char_p, c_char_p, c_int])
    _sig(lib, "wrapper_free_model", None, [c_void_p])
    _sig(lib, "wrapper_model_n_embd", c_int, [c_void_p])
    _sig(lib, "wrapper_create_context", c_void_p, [c_void_p, c_int, c_int, c_int, c_int])
    _sig(lib, "wrapper_create_context_slots", c_void_p, [c_void_p, c_int, c_int, c_int])
    _sig(lib, "wrapper_free_context", None, [c_void_p])
    _sig(lib, "wrapper_ctx_n_slots", c_int, [c_void_p])
    _sig(lib, "wrapper_kv_clear", None, [c_void_p])
    _sig(lib, "wrapper_decode_embd", c_int, [c_void_p, f32p, c_int, c_int, c_int, f32p])
    _sig(lib, "wrapper_decode_embd_slot", c_int, [c_void_p, c_int, f32p, c_int, c_int, c_int, f32p])
    _sig(lib, "wrapper_decode_embd_batch", c_int, [c_void_p, f32p, c_int, c_int, i32p, i32p, f32p])
    _sig(lib, "wrapper_codec_head", c_int, [c_void_p, f32p, c_int, f32p])
    _sig(lib, "wrapper_state_get_size", ctypes.c_size_t, [c_void_p])
    _sig(lib, "wrapper_state_save_file", c_int, [c_void_p, c_char_p])
    _sig(lib, "wrapper_state_load_file", c_int, [c_void_p, c_char_p])
    # include/qwen3tts_cp.h
    _sig(lib, "cp_load", c_void_p, [c_char_p, c_char_p, c_int])
    _sig(lib, "cp_free", None, [c_void_p])
    _sig(lib, "cp_hidden_size", c_int, [c_void_p])
    _sig(lib, "cp_predict", c_int, [c_void_p, f32p, ctypes.c_int32, c_float, c_int, ctypes.c_uint64, i32p])
    _sig(lib, "cp_predict_batch", c_int, [c_void_p, f32p, i32p, c_int, c_float, c_int, ctypes.c_uint64, i32p])
    _sig(lib, "cp_step", c_int, [c_void_p, f32p, c_int, f32p])
    _sig(lib, "cp_lm_head", c_int, [c_void_p, c_int, f32p, f32p])
    # include/qwen3tts_engine.h
    _sig(lib, "q3e_create", c_void_p, [c_char_p, c_int, c_int, c_int])
    _sig(lib, "q3e_free", None, [c_void_p])
    _sig(lib, "q3e_set_pad_embed", c_int, [c_void_p, f32p])
    _sig(lib, "q3e_set_chains", c_int, [c_void_p, c_int])
    _sig(lib, "q3e_set_sampling", c_int, [c_void_p, c_float, c_int, c_float, c_float, c_int, ctypes.c_uint64])
    _sig(lib, "q3e_set_forced_codes", c_int, [c_void_p, i32p, c_int])
    _sig(lib, "q3e_start", c_int, [c_void_p, c_int, f32p, i32p, i32p, c_int, c_int])
    _sig(lib, "q3e_run", c_int, [c_void_p, c_int])
    _sig(lib, "q3e_graph_nodes", c_int, [c_void_p])
    _sig(lib, "q3e_last_run_ms", c_float, [c_void_p])
    _sig(lib, "q3e_last_prefill_ms", c_float, [c_void_p])
    _sig(lib, "q3e_get_codes", c_int, [c_void_p, i32p, c_int, i32p])
    _sig(lib, "q3e_scores_reserve", c_int, [c_void_p, c_int])
    _sig(lib, "q3e_get_scores", c_int, [c_void_p, f32p, c_int, i32p])
    _sig(lib, "q3e_get_done", c_int, [c_void_p, i32p, i32p])
    _sig(lib, "q3e_refill", c_int, [c_void_p, c_int, i32p, f32p, i32p, i32p])
    _sig(lib, "q3e_open", c_int, [c_void_p, c_int, c_int])
    _sig(lib, "q3e_admit", c_int, [c_void_p, c_int, i32p, f32p, i32p, i32p, ctypes.POINTER(SlotParamsC)])
    _sig(lib, "q3e_release", c_int, [c_void_p, c_int, i32p])
    _sig(lib, "q3e_prefix_cache", c_int, [c_void_p, c_int, c_int])
    _sig(lib, "q3e_admit_keyed", c_int, [c_void_p, c_int, i32p, f32p, i32p, i32p, ctypes.POINTER(SlotParamsC),
                                         ctypes.POINTER(ctypes.c_uint64), i32p])
    _sig(lib, "q3e_prefix_stats", c_int, [c_void_p, i64p])
    _sig(lib, "q3e_admit_prompted", c_int, [c_void_p, c_int, i32p, f32p, i32p, i32p, ctypes.POINTER(SlotParamsC),
                                            ctypes.POINTER(ctypes.c_uint64), i32p, i32p, i32p])
    _sig(lib, "q3e_default_rules", None, [ctypes.POINTER(SlotRulesC)])
    _sig(lib, "q3e_rules_reserve", c_int, [c_void_p, c_int])
    _sig(lib, "q3e_admit_ruled", c_int, [c_void_p, c_int, i32p, f32p, i32p, i32p, ctypes.POINTER(SlotParamsC),
                                         ctypes.POINTER(ctypes.c_uint64), i32p, i32p, i32p, ctypes.POINTER(SlotRulesC)])
    _sig(lib, "q3e_text_reserve", c_int, [c_void_p, c_int])
    _sig(lib, "q3e_push_text", c_int, [c_void_p, c_int, f32p, c_int, c_int, c_int])
    _sig(lib, "q3e_text_state", c_int, [c_void_p, i32p, i32p])
    _sig(lib, "q3e_text_hold", c_int, [c_void_p, c_int])
    _sig(lib, "q3e_text_held", c_int, [c_void_p, i64p])
    _sig(lib, "q3e_get_hidden", c_int, [c_void_p, f32p])
    _sig(lib, "q3e_step_weight_bytes", ctypes.c_double, [c_void_p])
    # include/qwen3tts_voc.h
    _sig(lib, "voc_load", c_void_p, [c_char_p, c_int, c_int])
    _sig(lib, "voc_free", None, [c_void_p])
    _sig(lib, "voc_chunk_tokens", c_int, [c_void_p])
    _sig(lib, "voc_samples_per_token", c_int, [c_void_p])
    _sig(lib, "voc_chunk_samples", c_int, [c_void_p])
    _sig(lib, "voc_decode", c_int, [c_void_p, i64p, c_int, f32p])
    _sig(lib, "voc_synthesize", c_int, [c_void_p, i64p, c_int, i16p, i32p])
    _sig(lib, "voc_synthesize_f32", c_int, [c_void_p, i64p, c_int, f32p, i32p])
    _sig(lib, "voc_synthesize_max_samples", c_int, [c_void_p, c_int])
    _sig(lib, "voc_set_max_workgroups", c_int, [c_int])
    _sig(lib, "voc_set_exact_fp32", c_int, [c_int])
    _sig(lib, "voc_set_fused_units", c_int, [c_int])
    _sig(lib, "voc_last_decode_ms", c_float, [c_void_p])
    _sig(lib, "voc_decode_flops", ctypes.c_double, [c_void_p, c_int])
    i64p_ = ctypes.POINTER(ctypes.c_int64)
    _sig(lib, "voc_synthesize_batch", c_int, [c_void_p, i64p, i32p, c_int, i16p, ctypes.c_int64, i64p_])
    _sig(lib, "voc_synthesize_batch_f32", c_int, [c_void_p, i64p, i32p, c_int, f32p, ctypes.c_int64, i64p_])
    _sig(lib, "voc_synthesize_batch_max_samples", ctypes.c_int64, [c_void_p, i32p, c_int])
    _sig(lib, "voc_last_batch_ms", c_float, [c_void_p])
    _sig(lib, "voc_last_batch_chunks", c_int, [c_void_p])
    _sig(lib, "voc_stream_create", c_void_p, [c_void_p, c_int])
    _sig(lib, "voc_stream_free", None, [c_void_p])
    _sig(lib, "voc_stream_reset", c_int, [c_void_p, c_int])
    _sig(lib, "voc_stream_push_max_samples", ctypes.c_int64, [c_void_p, c_int, i32p, i32p, i32p])
    _sig(lib, "voc_stream_push", c_int, [c_void_p, c_int, i32p, i64p, i32p, i32p, i16p, ctypes.c_int64, i64p_])
    _sig(lib, "voc_stream_push_f32", c_int, [c_void_p, c_int, i32p, i64p, i32p, i32p, f32p, ctypes.c_int64, i64p_])
    _sig(lib, "voc_stream_last_decodes", c_int, [c_void_p])
    _sig(lib, "voc_stream_last_chunks", c_int, [c_void_p])
    _sig(lib, "voc_stream_last_ms", c_float, [c_void_p])
    _sig(lib, "voc_incr_create", c_void_p, [c_void_p, c_int])
    _sig(lib, "voc_incr_free", None, [c_void_p])
    _sig(lib, "voc_incr_reset", c_int, [c_void_p, c_int])
    _sig(lib, "voc_incr_push_max_samples", ctypes.c_int64, [c_void_p, c_int, i32p, i32p, i32p])
    _sig(lib, "voc_incr_push", c_int, [c_void_p, c_int, i32p, i64p, i32p, i32p, i16p, ctypes.c_int64, i64p_])
    _sig(lib, "voc_incr_push_f32", c_int, [c_void_p, c_int, i32p, i64p, i32p, i32p, f32p, ctypes.c_int64, i64p_])
    _sig(lib, "voc_incr_last_ms", c_float, [c_void_p])
    _sig(lib, "voc_incr_last_launches", c_int, [c_void_p])
    _sig(lib, "voc_incr_samples", ctypes.c_int64, [c_void_p, ctypes.c_int64])
    _sig(lib, "voc_incr_state_bytes", ctypes.c_int64, [c_void_p])
    _sig(lib, "voc_incr_device_bytes", ctypes.c_int64, [c_void_p])
    _sig(lib, "voc_incr_set_arithmetic", c_int, [c_void_p, c_int])
    _sig(lib, "voc_incr_arithmetic", c_int, [c_void_p])
    _sig(lib, "voc_incr_last_split_launches", c_int, [c_void_p])
    _sig(lib, "voc_incr_last_redone", c_int, [c_void_p])
    _sig(lib, "voc_incr_snapshots", c_int, [c_void_p, c_int])
    _sig(lib, "voc_incr_save", c_int, [c_void_p, c_int, c_int])
    _sig(lib, "voc_incr_restore", c_int, [c_void_p, c_int, i32p, i32p])
    _sig(lib, "voc_incr_snapshot_frames", ctypes.c_int64, [c_void_p, c_int])
    _sig(lib, "voc_incr_last_restore_ms", c_float, [c_void_p])
    # include/qwen3tts_enc.h
    _sig(lib, "enc_load", c_void_p, [c_char_p, c_int, c_int])
    _sig(lib, "enc_free", None, [c_void_p])
    _sig(lib, "enc_num_quantizers", c_int, [c_void_p])
    _sig(lib, "enc_sample_rate", c_int, [c_void_p])
    _sig(lib, "enc_samples_per_frame", c_int, [c_void_p])
    _sig(lib, "enc_frames", c_int, [c_void_p, c_int])
    _sig(lib, "enc_encode", c_int, [c_void_p, f32p, i32p, c_int, i64p_, c_int, i32p])
    _sig(lib, "enc_last_ms", c_float, [c_void_p])
    _sig(lib, "enc_pcm_frames", c_int, [c_void_p, c_int, c_int])
    _sig(lib, "enc_encode_pcm", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, i32p, c_int, i64p_, c_int, i32p])
    _sig(lib, "enc_debug_pcm", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, i32p, c_int, f32p, i32p, i32p])
    _sig(lib, "enc_debug_shape", c_int, [c_void_p, i32p, c_int, c_int, i32p, i32p])
    _sig(lib, "enc_debug_run", c_int, [c_void_p, f32p, i32p, c_int, c_int, f32p, i32p, i32p])
    _sig(lib, "enc_resample_pcm", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, i32p, c_int, f32p, c_int, i32p])
    # include/qwen3tts_spk.h
    _sig(lib, "spk_load", c_void_p, [c_char_p, c_int, c_int])
    _sig(lib, "spk_free", None, [c_void_p])
    _sig(lib, "spk_dim", c_int, [c_void_p])
    _sig(lib, "spk_sample_rate", c_int, [c_void_p])
    _sig(lib, "spk_min_samples", c_int, [c_void_p])
    _sig(lib, "spk_frames", c_int, [c_void_p, c_int])
    _sig(lib, "spk_embed", c_int, [c_void_p, f32p, i32p, c_int, f32p])
    _sig(lib, "spk_last_ms", c_float, [c_void_p])
    _sig(lib, "spk_last_launches", c_int, [c_void_p])
    # include/qwen3tts_enc_stream.h
    _sig(lib, "enc_stream_create", c_void_p, [c_void_p, c_int, c_int])
    _sig(lib, "enc_stream_free", None, [c_void_p])
    _sig(lib, "enc_stream_reset", c_int, [c_void_p, c_int])
    _sig(lib, "enc_stream_push_max_frames", c_int, [c_void_p, c_int, i32p, i32p, i32p])
    _sig(lib, "enc_stream_push", c_int, [c_void_p, c_int, i32p, f32p, i32p, i32p, i64p_, ctypes.c_int64, i64p_])
    _sig(lib, "enc_stream_last_ms", c_float, [c_void_p])
    _sig(lib, "enc_stream_last_launches", c_int, [c_void_p])
    _sig(lib, "enc_stream_state_bytes", ctypes.c_int64, [c_void_p])
    _sig(lib, "enc_stream_device_bytes", ctypes.c_int64, [c_void_p])
    # include/qwen3tts_enc_stream_pcm.h (and the hook enc_stream_debug_push_pcm beside enc_debug_pcm)
    _sig(lib, "enc_stream_pcm_samples", ctypes.c_int64, [c_void_p, c_int, ctypes.c_int64, c_int])
    _sig(lib, "enc_stream_pcm_max_frames_in", c_int, [c_void_p, c_int])
    _sig(lib, "enc_stream_push_pcm_max_frames", c_int, [c_void_p, c_int, i32p, c_int, c_int, c_int, i32p, i32p])
    _sig(lib, "enc_stream_push_pcm", c_int, [c_void_p, c_int, i32p, c_void_p, c_int, c_int, c_int, i32p, i32p, i64p_, ctypes.c_int64,
                                             i64p_])
    _sig(lib, "enc_stream_pcm_device_bytes", ctypes.c_int64, [c_void_p])
    _sig(lib, "enc_stream_debug_push_pcm", c_int, [c_void_p, c_int, i32p, c_void_p, c_int, c_int, c_int, i32p, i32p, i64p_,
                                                   ctypes.c_int64, i64p_, f32p, i64p_])
    # include/qwen3tts_text.h
    _sig(lib, "tfe_load", c_void_p, [c_char_p, c_char_p, c_int])
    _sig(lib, "tfe_free", None, [c_void_p])
    _sig(lib, "tfe_hidden_size", c_int, [c_void_p])
    _sig(lib, "tfe_text_vocab", c_int, [c_void_p])
    _sig(lib, "tfe_embed_text", c_int, [c_void_p, i32p, c_int, f32p])
    _sig(lib, "tfe_build_prefix", c_int, [c_void_p, i32p, c_int, i32p, f32p])
    _sig(lib, "tfe_tts_pad_embed", c_int, [c_void_p, f32p])
    _sig(lib, "tfe_build_prefix_stream", c_int, [c_void_p, ctypes.c_int32, i32p, f32p])
    _sig(lib, "tfe_tts_eos_embed", c_int, [c_void_p, f32p])
    _sig(lib, "tfe_build_prefix_spk", c_int, [c_void_p, i32p, c_int, i32p, f32p, f32p])
    _sig(lib, "tfe_build_prefix_stream_spk", c_int, [c_void_p, ctypes.c_int32, i32p, f32p, f32p])
    # test hook of csrc/q3_text_api.hip (not in the header): ids, n -> x16, h1, a16, h2 in fragment order, dims[4]
    _sig(lib, "tfe_debug_stages", c_int, [c_void_p, i32p, c_int, u16p, f32p, u16p, f32p, i32p])
    _sig(lib, "q3_device_count", c_int, [])
    _sig(lib, "q3_device_compute_units", c_int, [])
    _sig(lib, "q3_set_device", c_int, [c_int])
    if path is None:
        _lib = lib
    return lib


def load_test():
    """dlopen libqwen3tts_test.so: kernel-level hooks (csrc/q3_test_api.hip) for tests/ and bench.py.  The
    product never calls this."""
    global _test_lib
    if _test_lib is not None:
        return _test_lib
    load()   # the product library first: the test library links against it
    if not os.path.exists(TEST_LIB_PATH):
        raise RuntimeError(f"{TEST_LIB_PATH} not found: build it with `python -m qwen3_tts_axera_russian_amd.build`")
    lib = ctypes.CDLL(TEST_LIB_PATH)
    _sig(lib, "q3t_set_linear_tuning", c_int, [c_int, c_int, c_int])
    _sig(lib, "q3t_linear", c_int, [c_int, c_int, c_int, u16p, c_int, c_int, c_int, u16p, f32p, f32p, c_float,
                                    f32p, f32p, u16p, c_int])
    _sig(lib, "q3t_linear_case", c_int, [c_int, c_int, c_int, c_int, u16p, c_int, c_int, c_int, c_int, c_float, c_int,
                                         u16p, f32p, f32p, f32p, f32p, f32p, u16p, f32p, f32p, f32p, u16p, u16p])
    _sig(lib, "q3t_reset_linear_knobs", c_int, [])
    _sig(lib, "q3t_last_linear_variant", c_char_p, [])
    _sig(lib, "q3t_talker_sample", c_int, [f32p, c_int, i32p, c_int, c_int, c_int])
    u64, u64p = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    _sig(lib, "q3t_talker_sample_case", c_int, [f32p, c_int, c_int, c_int, c_int, i32p, i32p, i32p, i32p, i32p, i32p, i32p,
                                                i32p, c_int, i32p, c_int, c_int, c_int, c_int, c_float, c_float, c_int,
                                                c_float, u64, u64p, c_void_p])
    _sig(lib, "q3t_cp_sample_case", c_int, [f32p, c_int, c_int, c_int, c_int, c_int, i32p, i32p, c_int, i32p, c_float, c_int,
                                            u64, u64p, c_void_p, c_int, c_int, f32p, f32p, c_int, f32p, f32p, c_int, f32p,
                                            c_int, f32p, f32p, f32p, ctypes.POINTER(ctypes.c_uint16), f32p])
    talker_case = [f32p, c_int, c_int, c_int, c_int, i32p, i32p, i32p, i32p, i32p, i32p, i32p, i32p, c_int, i32p, c_int, c_int,
                   c_int, c_int, c_float, c_float, c_int, c_float, u64, u64p, c_void_p]
    cp_case = [f32p, c_int, c_int, c_int, c_int, c_int, i32p, i32p, c_int, i32p, c_float, c_int, u64, u64p, c_void_p, c_int,
               c_int, f32p, f32p, c_int, f32p, f32p, c_int, f32p, c_int, f32p, f32p, f32p, u16p, f32p]
    _sig(lib, "q3t_talker_sample_text_case", c_int, talker_case + [i32p, i32p])
    _sig(lib, "q3t_cp_sample_text_case", c_int, cp_case + [f32p, i32p, c_int, i32p])
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _sig(lib, "q3t_talker_sample_rules_case", c_int, talker_case + [i32p, i32p, c_void_p, u32p])
    _sig(lib, "q3t_cp_sample_rules_case", c_int, cp_case + [f32p, i32p, c_int, i32p, c_void_p])
    _sig(lib, "q3t_talker_score_case", c_int, talker_case + [i32p, i32p, c_void_p, u32p, f32p])
    _sig(lib, "q3t_cp_score_case", c_int, cp_case + [f32p, i32p, c_int, i32p, c_void_p, f32p])
    _sig(lib, "q3t_prompt_rows_seen_case", c_int, [i32p, c_int, i32p, i32p, f32p, c_int, f32p, c_int, c_int, c_int, f32p, c_int,
                                                   c_int, c_int, c_int, c_int, f32p, f32p, f32p, u16p, c_int, u32p, c_int])
    _sig(lib, "q3t_final_norm_case", c_int, [f32p, f32p, c_int, c_int, c_int, f32p, c_float, c_int, c_int, i32p, c_int, c_int,
                                             c_int, c_int, c_int, f32p, f32p, u16p, f32p, f32p, u16p])
    _sig(lib, "q3t_gather_embed_case", c_int, [f32p, c_int, c_int, i32p, c_int, i32p, c_int, c_int, i32p, c_int, c_int, c_int,
                                               f32p, f32p, f32p, u16p])
    _sig(lib, "q3t_feedback_case", c_int, [i32p, c_int, f32p, c_int, f32p, c_int, c_int, f32p, c_int, f32p, f32p, f32p, u16p])
    _sig(lib, "q3t_prompt_rows_case", c_int, [i32p, c_int, i32p, i32p, f32p, c_int, f32p, c_int, c_int, c_int, f32p, c_int,
                                              c_int, c_int, c_int, c_int, f32p, f32p, f32p, u16p, c_int])
    _sig(lib, "q3t_prefix_move_case", c_int, [u16p, u16p, c_int, c_int, c_int, c_int, u16p, c_int, c_int, f32p, f32p, f32p,
                                              c_int, c_int, c_int, i32p])
    _sig(lib, "q3t_attn", c_int, [c_int, c_int, c_int, f32p, f32p, f32p, c_float, f32p, f32p, c_int, i32p, i32p, c_int,
                                  c_int, c_int, c_int, u16p, u16p, c_int, c_int, i32p, c_int, c_int, c_int, c_int, u16p])
    _sig(lib, "q3t_voc_attn", c_int, [c_int, f32p, f32p, c_int, c_int, c_int, c_int, c_int, c_float])
    _sig(lib, "q3t_xlane_case", c_int, [c_int, c_int, c_int, f32p, f32p, f32p])
    _sig(lib, "q3t_set_linear_split_rows", c_int, [c_int])
    _sig(lib, "q3t_set_linear_narrow8", c_int, [c_int])
    _sig(lib, "q3t_set_linear_wide_tiles", c_int, [c_int])
    _sig(lib, "q3t_set_attn_short", c_int, [c_int])
    _sig(lib, "q3t_set_gemm_min_rows", c_int, [c_int])
    _sig(lib, "q3t_set_gemm_glds", c_int, [c_int])
    _sig(lib, "q3t_inspect_weights", c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, c_int])
    _sig(lib, "q3t_bench_linear", c_float, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int])
    _sig(lib, "q3t_bench_chain", c_float, [c_int, c_int, c_int, c_int, c_int, c_int])
    _sig(lib, "q3t_cp_model_load", c_void_p, [c_char_p])
    _sig(lib, "q3t_cp_model_free", None, [c_void_p])
    _sig(lib, "q3t_cp_qkv_ld", c_int, [c_void_p])
    _sig(lib, "q3t_cp_qkv_serves", c_int, [c_void_p, c_int])
    _sig(lib, "q3t_cp_qkv_tab", c_int, [c_void_p, c_int, i32p, c_int, f32p])
    _sig(lib, "q3t_cp_qkv_live", c_int, [c_void_p, c_int, i32p, c_int, c_int, f32p])
    _sig(lib, "q3t_enc_stream_embeddings", c_int, [c_void_p, c_int, i32p, f32p, i32p, i32p, i64p, ctypes.c_int64, i64p, f32p, i32p])
    i64s = ctypes.POINTER(ctypes.c_longlong)
    _sig(lib, "q3t_enc_stream_plan", c_int, [i32p, i32p, c_int, ctypes.c_longlong, ctypes.c_longlong, c_int, i64s, i64s, i64s])
    _sig(lib, "q3t_enc_rvq_tile", c_int, [c_int])
    _sig(lib, "q3t_enc_rvq_case", c_int, [f32p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, f32p, i64p])
    _sig(lib, "q3t_enc_conv_in_case", c_int, [f32p, c_int, c_int, f32p, f32p, c_int, c_int, f32p, c_int, i32p, f32p])
    u8p = ctypes.POINTER(ctypes.c_uint8)
    _sig(lib, "q3t_dequant_case", c_int, [c_int, u8p, ctypes.c_longlong, c_int, c_int, c_int, c_int, u16p, f32p, i32p])
    _sig(lib, "q3t_spk_mel", c_int, [c_void_p, f32p, i32p, c_int, f32p, i32p, i32p])
    _sig(lib, "q3t_spk_stage", c_int, [c_void_p, f32p, i32p, c_int, c_int, f32p, i32p, i32p])
    # one launch of each of the speaker encoder's own kernels and of the encoder's unfold / emit kernels
    _sig(lib, "q3t_spk_unfold_case", c_int, [f32p, c_int, c_int, f32p, c_int, c_int, i32p, c_int, c_int, c_int, c_int, f32p])
    _sig(lib, "q3t_spk_place_case", c_int, [f32p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, f32p])
    _sig(lib, "q3t_spk_rowmean_case", c_int, [f32p, c_int, i32p, c_int, f32p])
    _sig(lib, "q3t_spk_rowstat_case", c_int, [f32p, c_int, i32p, c_int, f32p])
    _sig(lib, "q3t_spk_attnpool_case", c_int, [f32p, f32p, c_int, i32p, c_int, f32p])
    _sig(lib, "q3t_spk_matvec_case", c_int, [f32p, f32p, f32p, c_int, c_int, c_int, c_int, f32p])
    _sig(lib, "q3t_spk_se_apply_case", c_int, [f32p, f32p, f32p, c_int, c_int, c_int, c_int, c_int, f32p, f32p])
    _sig(lib, "q3t_spk_att_act_case", c_int, [f32p, f32p, c_int, c_int, c_int, f32p])
    _sig(lib, "q3t_enc_unfold_case", c_int, [f32p, c_int, c_int, i32p, c_int, c_int, c_int, c_int, f32p])
    _sig(lib, "q3t_enc_stream_unfold_case", c_int, [f32p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, f32p, c_int,
                                                    i32p, i32p, f32p])
    _sig(lib, "q3t_enc_stream_emit_case", c_int, [f32p, c_int, c_int, c_int, c_int, i32p, c_int, f32p])
    _test_lib = lib
    return lib


def fptr(a):
    return a.ctypes.data_as(f32p)


def iptr(a):
    return a.ctypes.data_as(i32p)

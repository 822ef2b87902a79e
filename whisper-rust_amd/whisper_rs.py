"""Host-side mirror of the whisper-rs safe API over the C ABI (`include/whisper_amd.h`).

The reference's host layer is Rust (`src/whisper_ctx_wrapper.rs`, `src/whisper_state.rs`,
`src/whisper_params.rs`); there is no Rust toolchain in this image, so tests and the bench drive the
C ABI through this thin ctypes mirror instead.  Names, argument meaning and error behaviour follow
whisper-rs:

  WhisperContext.new_with_params(path, params)   src/whisper_ctx_wrapper.rs:35-47
  WhisperContext.create_state()                  src/whisper_ctx_wrapper.rs:438-454
  WhisperState.full(params, pcm)                 src/whisper_state.rs:289-321
  WhisperState.full_n_segments / full_get_segment_text / _t0 / _t1 / token getters
                                                 src/whisper_state.rs:329-606
  WhisperState.pcm_to_mel / set_mel / encode / decode / get_logits / lang_detect
                                                 src/whisper_state.rs:50-260
  FullParams(strategy) + setters                 src/whisper_params.rs:36-803

The same binding can load EITHER library because both export the same ABI:
  * the product:  whisper-rust_amd/libwhisper.so      (HIP; fails loudly when absent)
  * the checker:  oracle/_ref/libwhisper_ref.so       (reference CPU engine; tests/bench only)
Nothing in this file computes anything: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, "libwhisper.so")

WHISPER_SAMPLING_GREEDY = 0
WHISPER_SAMPLING_BEAM_SEARCH = 1

# enum whisper_alignment_heads_preset (include/whisper_amd.h)
AHEADS_NONE, AHEADS_N_TOP_MOST, AHEADS_CUSTOM = 0, 1, 2


class WhisperError(RuntimeError):
    """Mirror of whisper-rs `WhisperError` (src/error.rs): carries the C return code."""

    def __init__(self, msg: str, code: int = 0):
        super().__init__(msg)
        self.code = code


# ---------------------------------------------------------------------------------------------------
# C structs (layout checked against sizeof/offsetof exported by the library in tests/test_abi.py)
# ---------------------------------------------------------------------------------------------------
class whisper_ahead(C.Structure):
    _fields_ = [("n_text_layer", C.c_int), ("n_head", C.c_int)]


class whisper_aheads(C.Structure):
    _fields_ = [("n_heads", C.c_size_t), ("heads", C.POINTER(whisper_ahead))]


class whisper_context_params(C.Structure):
    _fields_ = [
        ("use_gpu", C.c_bool),
        ("flash_attn", C.c_bool),
        ("gpu_device", C.c_int),
        ("dtw_token_timestamps", C.c_bool),
        ("dtw_aheads_preset", C.c_int),
        ("dtw_n_top", C.c_int),
        ("dtw_aheads", whisper_aheads),
        ("dtw_mem_size", C.c_size_t),
    ]


class whisper_token_data(C.Structure):
    _fields_ = [
        ("id", C.c_int32), ("tid", C.c_int32),
        ("p", C.c_float), ("plog", C.c_float), ("pt", C.c_float), ("ptsum", C.c_float),
        ("t0", C.c_int64), ("t1", C.c_int64), ("t_dtw", C.c_int64),
        ("vlen", C.c_float),
    ]


class whisper_vad_params(C.Structure):
    _fields_ = [
        ("threshold", C.c_float), ("min_speech_duration_ms", C.c_int), ("min_silence_duration_ms", C.c_int),
        ("max_speech_duration_s", C.c_float), ("speech_pad_ms", C.c_int), ("samples_overlap", C.c_float),
    ]


class whisper_amd_align_score(C.Structure):      # 24 bytes (include/whisper_amd.h)
    _fields_ = [("plog", C.c_float), ("p", C.c_float), ("best_id", C.c_int32), ("best_plog", C.c_float), ("rank", C.c_int32), ("best_p", C.c_float)]


class whisper_amd_align_token(C.Structure):      # 32 bytes
    _fields_ = [("id", C.c_int32), ("plog", C.c_float), ("p", C.c_float), ("best_id", C.c_int32), ("best_plog", C.c_float), ("rank", C.c_int32),
                ("t_dtw", C.c_int64)]


# whisper_amd_align's refusal codes (include/whisper_amd.h)
ALIGN_BAD_TOKEN, ALIGN_NO_TOKENS, ALIGN_TOO_LONG, ALIGN_FLASH_ATTN, ALIGN_TOO_SHORT = -21, -22, -23, -24, -25
ALIGN_SCORE_DTYPE = np.dtype([("plog", "<f4"), ("p", "<f4"), ("best_id", "<i4"), ("best_plog", "<f4"), ("rank", "<i4"), ("best_p", "<f4")])


class whisper_amd_channels_params(C.Structure):  # 16 bytes, passed by pointer (include/whisper_amd.h)
    _fields_ = [("max_chunk_ms", C.c_int32), ("n_parallel", C.c_int32), ("crosstalk_ratio", C.c_double)]


class whisper_amd_stream_params(C.Structure):    # 36 bytes, passed by pointer (include/whisper_amd.h)
    _fields_ = [(n, C.c_int32) for n in ("step_ms", "length_ms", "keep_ms", "sample_rate", "channels", "format", "backlog_ms", "carry_prompt", "drop_late")]


class whisper_amd_stream_vad_params(C.Structure):    # passed by pointer (include/whisper_amd.h)
    _fields_ = [(n, C.c_int32) for n in ("sample_rate", "channels", "format", "backlog_ms", "carry_prompt", "max_utterance_ms", "vad_on_feed")] + \
               [("vad", whisper_vad_params)]


class whisper_vad_context_params(C.Structure):
    _fields_ = [("n_threads", C.c_int), ("use_gpu", C.c_bool), ("gpu_device", C.c_int)]


LOADER_READ = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t)
LOADER_EOF = C.CFUNCTYPE(C.c_bool, C.c_void_p)
LOADER_CLOSE = C.CFUNCTYPE(None, C.c_void_p)


class whisper_model_loader(C.Structure):
    _fields_ = [("context", C.c_void_p), ("read", LOADER_READ), ("eof", LOADER_EOF), ("close", LOADER_CLOSE)]


NEW_SEGMENT_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
PROGRESS_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
ENCODER_BEGIN_CB = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_void_p, C.c_void_p)
ABORT_CB = C.CFUNCTYPE(C.c_bool, C.c_void_p)
LOGITS_FILTER_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.POINTER(whisper_token_data), C.c_int,
                               C.POINTER(C.c_float), C.c_void_p)
LOG_CB = C.CFUNCTYPE(None, C.c_int, C.c_char_p, C.c_void_p)


GRETYPE_END, GRETYPE_ALT, GRETYPE_RULE_REF, GRETYPE_CHAR, GRETYPE_CHAR_NOT, GRETYPE_CHAR_RNG_UPPER, GRETYPE_CHAR_ALT = range(7)   # whisper.h:162-185


class whisper_grammar_element(C.Structure):
    _fields_ = [("type", C.c_int), ("value", C.c_uint32)]


class _greedy(C.Structure):
    _fields_ = [("best_of", C.c_int)]


class _beam(C.Structure):
    _fields_ = [("beam_size", C.c_int), ("patience", C.c_float)]


class whisper_full_params(C.Structure):
    _fields_ = [
        ("strategy", C.c_int),
        ("n_threads", C.c_int), ("n_max_text_ctx", C.c_int), ("offset_ms", C.c_int), ("duration_ms", C.c_int),
        ("translate", C.c_bool), ("no_context", C.c_bool), ("no_timestamps", C.c_bool), ("single_segment", C.c_bool),
        ("print_special", C.c_bool), ("print_progress", C.c_bool), ("print_realtime", C.c_bool),
        ("print_timestamps", C.c_bool),
        ("token_timestamps", C.c_bool), ("thold_pt", C.c_float), ("thold_ptsum", C.c_float), ("max_len", C.c_int),
        ("split_on_word", C.c_bool), ("max_tokens", C.c_int),
        ("debug_mode", C.c_bool), ("audio_ctx", C.c_int),
        ("tdrz_enable", C.c_bool),
        ("suppress_regex", C.c_char_p),
        ("initial_prompt", C.c_char_p), ("prompt_tokens", C.POINTER(C.c_int32)), ("prompt_n_tokens", C.c_int),
        ("language", C.c_char_p), ("detect_language", C.c_bool),
        ("suppress_blank", C.c_bool), ("suppress_nst", C.c_bool),
        ("temperature", C.c_float), ("max_initial_ts", C.c_float), ("length_penalty", C.c_float),
        ("temperature_inc", C.c_float), ("entropy_thold", C.c_float), ("logprob_thold", C.c_float),
        ("no_speech_thold", C.c_float),
        ("greedy", _greedy),
        ("beam_search", _beam),
        ("new_segment_callback", NEW_SEGMENT_CB), ("new_segment_callback_user_data", C.c_void_p),
        ("progress_callback", PROGRESS_CB), ("progress_callback_user_data", C.c_void_p),
        ("encoder_begin_callback", ENCODER_BEGIN_CB), ("encoder_begin_callback_user_data", C.c_void_p),
        ("abort_callback", ABORT_CB), ("abort_callback_user_data", C.c_void_p),
        ("logits_filter_callback", LOGITS_FILTER_CB), ("logits_filter_callback_user_data", C.c_void_p),
        ("grammar_rules", C.c_void_p), ("n_grammar_rules", C.c_size_t), ("i_start_rule", C.c_size_t),
        ("grammar_penalty", C.c_float),
        ("vad", C.c_bool), ("vad_model_path", C.c_char_p),
        ("vad_params", whisper_vad_params),
    ]


# ---------------------------------------------------------------------------------------------------
# library loading
# ---------------------------------------------------------------------------------------------------
_LIBS: dict[str, C.CDLL] = {}


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen a whisper C-ABI library and declare the prototypes used by this mirror.

    Fails loudly (OSError) when the library is missing: there is no fallback implementation.
    """
    path = os.path.abspath(path or PRODUCT_LIB)
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise OSError(f"{path} not found - build it first (python -c 'import __graft_entry__ as g; g.build()')")
    lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    P, I, F = C.c_void_p, C.c_int, C.c_float

    def proto(name, res, *args):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = list(args)

    proto("whisper_context_default_params", whisper_context_params)
    proto("whisper_full_default_params", whisper_full_params, I)
    proto("whisper_init_from_file_with_params_no_state", P, C.c_char_p, whisper_context_params)
    proto("whisper_init_from_buffer_with_params_no_state", P, P, C.c_size_t, whisper_context_params)
    proto("whisper_init_state", P, P)
    proto("whisper_free", None, P)
    proto("whisper_free_state", None, P)
    proto("whisper_pcm_to_mel_with_state", I, P, P, C.POINTER(F), I, I)
    proto("whisper_set_mel_with_state", I, P, P, C.POINTER(F), I, I)
    proto("whisper_encode_with_state", I, P, P, I, I)
    proto("whisper_decode_with_state", I, P, P, C.POINTER(C.c_int32), I, I, I)
    proto("whisper_lang_auto_detect_with_state", I, P, P, I, I, C.POINTER(F))
    proto("whisper_get_logits_from_state", C.POINTER(F), P)
    proto("whisper_n_len_from_state", I, P)
    proto("whisper_full_with_state", I, P, P, whisper_full_params, P, I)
    proto("whisper_full_n_segments_from_state", I, P)
    proto("whisper_full_lang_id_from_state", I, P)
    proto("whisper_full_get_segment_t0_from_state", C.c_int64, P, I)
    proto("whisper_full_get_segment_t1_from_state", C.c_int64, P, I)
    proto("whisper_full_get_segment_text_from_state", C.c_char_p, P, I)
    proto("whisper_full_get_segment_speaker_turn_next_from_state", C.c_bool, P, I)
    proto("whisper_full_get_segment_no_speech_prob_from_state", F, P, I)
    proto("whisper_full_n_tokens_from_state", I, P, I)
    proto("whisper_full_get_token_text_from_state", C.c_char_p, P, P, I, I)
    proto("whisper_full_get_token_id_from_state", C.c_int32, P, I, I)
    proto("whisper_full_get_token_data_from_state", whisper_token_data, P, I, I)
    proto("whisper_full_get_token_p_from_state", F, P, I, I)
    proto("whisper_tokenize", I, P, C.c_char_p, C.POINTER(C.c_int32), I)
    for n in ("whisper_n_vocab", "whisper_n_text_ctx", "whisper_n_audio_ctx", "whisper_is_multilingual",
              "whisper_model_n_vocab", "whisper_model_n_audio_ctx", "whisper_model_n_audio_state",
              "whisper_model_n_audio_head", "whisper_model_n_audio_layer", "whisper_model_n_text_ctx",
              "whisper_model_n_text_state", "whisper_model_n_text_head", "whisper_model_n_text_layer",
              "whisper_model_n_mels", "whisper_model_ftype", "whisper_model_type",
              "whisper_token_eot", "whisper_token_sot", "whisper_token_solm", "whisper_token_prev",
              "whisper_token_nosp", "whisper_token_not", "whisper_token_beg", "whisper_token_translate",
              "whisper_token_transcribe"):
        proto(n, I, P)
    proto("whisper_token_lang", I, P, I)
    proto("whisper_token_to_str", C.c_char_p, P, I)
    proto("whisper_model_type_readable", C.c_char_p, P)
    proto("whisper_lang_max_id", I)
    proto("whisper_lang_id", I, C.c_char_p)
    proto("whisper_lang_str", C.c_char_p, I)
    proto("whisper_lang_str_full", C.c_char_p, I)
    proto("whisper_print_system_info", C.c_char_p)
    proto("whisper_print_timings", None, P)
    proto("whisper_reset_timings", None, P)
    proto("whisper_log_set", None, LOG_CB, P)
    # whisper_full / whisper_full_parallel on the context's own state, and the context-level getters
    proto("whisper_init_from_file_with_params", P, C.c_char_p, whisper_context_params)
    proto("whisper_full", I, P, whisper_full_params, C.POINTER(F), I)
    proto("whisper_full_parallel", I, P, whisper_full_params, C.POINTER(F), I, I)
    proto("whisper_full_n_segments", I, P)
    proto("whisper_full_get_segment_t0", C.c_int64, P, I)
    proto("whisper_full_get_segment_t1", C.c_int64, P, I)
    proto("whisper_full_get_segment_text", C.c_char_p, P, I)
    proto("whisper_full_n_tokens", I, P, I)
    proto("whisper_full_get_token_data", whisper_token_data, P, I, I)
    # voice activity detection (whisper.h: whisper_vad_*)
    proto("whisper_vad_default_context_params", whisper_vad_context_params)
    proto("whisper_vad_default_params", whisper_vad_params)
    proto("whisper_vad_init_from_file_with_params", P, C.c_char_p, whisper_vad_context_params)
    proto("whisper_vad_init_with_params", P, C.POINTER(whisper_model_loader), whisper_vad_context_params)
    proto("whisper_vad_detect_speech", C.c_bool, P, C.POINTER(F), I)
    proto("whisper_vad_n_probs", I, P)
    proto("whisper_vad_probs", C.POINTER(F), P)
    proto("whisper_vad_segments_from_probs", P, P, whisper_vad_params)
    proto("whisper_vad_segments_from_samples", P, P, whisper_vad_params, C.POINTER(F), I)
    proto("whisper_vad_segments_n_segments", I, P)
    proto("whisper_vad_segments_get_segment_t0", F, P, I)
    proto("whisper_vad_segments_get_segment_t1", F, P, I)
    proto("whisper_vad_free_segments", None, P)
    proto("whisper_vad_free", None, P)
    if hasattr(lib, "whisper_amd_vad_front"):
        proto("whisper_amd_vad_front", C.c_int64, P, C.POINTER(F), I, C.POINTER(F), C.c_int64)
        proto("whisper_amd_vad_tile", I)
    if hasattr(lib, "whisper_amd_full_batch"):
        proto("whisper_amd_full_batch", I, P, C.POINTER(C.c_void_p), I, whisper_full_params, C.POINTER(C.c_void_p), C.POINTER(C.c_int))
    if hasattr(lib, "whisper_amd_rows_stats"):
        proto("whisper_amd_rows_stats", None, P, C.POINTER(C.c_long))
        proto("whisper_amd_rows_enabled", I, P)
        proto("whisper_amd_batch_one_launch", C.c_long, P)
    if hasattr(lib, "whisper_amd_decode_batch"):
        proto("whisper_amd_decode_batch", I, P, P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int8), I)
        proto("whisper_amd_kv_op", I, P, I, I, I, I, I)
        proto("whisper_amd_rows_fits", I, P, I)
        proto("whisper_amd_rows_debug_rows", I, P, C.POINTER(C.c_void_p), I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(F), C.POINTER(C.c_uint))
    if hasattr(lib, "whisper_amd_batch_served"):
        proto("whisper_amd_batch_served", C.c_long, P)
    if hasattr(lib, "whisper_amd_dtw_path"):
        proto("whisper_amd_dtw_path", I, P, C.POINTER(F), I, I, I, I, I, I, I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), I)
        proto("whisper_amd_dtw_stats", None, P, C.POINTER(C.c_long))
        proto("whisper_amd_dtw_timings", None, P, C.POINTER(C.c_int64))
    if hasattr(lib, "whisper_amd_qgemm_stats"):
        proto("whisper_amd_qgemm_stats", None, P, C.POINTER(C.c_long))
    if hasattr(lib, "whisper_amd_few_rows_stats"):
        proto("whisper_amd_few_rows_stats", None, P, C.POINTER(C.c_long))
    if hasattr(lib, "whisper_amd_arena_read"):
        proto("whisper_amd_arena_read", C.c_int64, P, C.c_int64, P, C.c_int64)
        proto("whisper_amd_load_stats", None, P, C.POINTER(C.c_int64))
    if hasattr(lib, "whisper_amd_audio_to_pcm"):
        proto("whisper_amd_audio_n_samples", C.c_int64, C.c_int64, I)
        proto("whisper_amd_audio_to_pcm", P, P, P, C.c_int64, I, I, I, C.POINTER(C.c_int64))
        proto("whisper_amd_full_audio", I, P, P, whisper_full_params, P, C.c_int64, I, I, I)
        proto("whisper_amd_audio_copy", C.c_int64, P, C.POINTER(F), C.c_int64)
        proto("whisper_amd_audio_taps", C.c_int64, I, C.POINTER(F), C.c_int64, C.POINTER(I), C.POINTER(I), C.POINTER(I))
        proto("whisper_amd_audio_tile", I)
        if hasattr(lib, "whisper_amd_wav_parse"):
            proto("whisper_amd_wav_parse", I, P, C.c_int64, P)
        proto("whisper_amd_audio_stats", None, P, C.POINTER(C.c_long))
    if hasattr(lib, "whisper_amd_full_long"):
        I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        proto("whisper_amd_full_long", I, P, whisper_full_params, P, I, I, I)
        proto("whisper_amd_full_long_audio", I, P, whisper_full_params, P, C.c_int64, I, I, I, I, I)
        proto("whisper_amd_long_n_chunks", I, P)
        proto("whisper_amd_long_chunk_info", I, P, I, I64P)
        proto("whisper_amd_long_chunk_copy", C.c_int64, P, I, C.POINTER(F), C.c_int64)
        proto("whisper_amd_long_stats", None, P, I64P)
        proto("whisper_amd_long_plan", I, I64P, I, I, F, I, I32P, I32P, I64P, I)
        proto("whisper_amd_long_pack", I, P, P, I, I64P, I, F, I32P, I32P, I, I)
        proto("whisper_amd_long_tile", I)
        proto("whisper_amd_context_state", P, P)
        proto("whisper_amd_batch_stats", None, P, C.POINTER(C.c_long), C.POINTER(C.c_long))
    if hasattr(lib, "whisper_amd_audio_split"):
        I64P = C.POINTER(C.c_int64)
        proto("whisper_amd_audio_split", P, P, P, C.c_int64, I, I, I64P, I64P)
        proto("whisper_amd_audio_split_copy", C.c_int64, P, I, C.POINTER(F), C.c_int64)
        proto("whisper_amd_channel_energy", I, P, I64P, I64P, I, I, C.POINTER(C.c_double))
        proto("whisper_amd_channel_speakers", I, P, I64P, I64P, I, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int8))
        proto("whisper_amd_channels_default_params", None, C.POINTER(whisper_amd_channels_params))
        proto("whisper_amd_full_long_channels", I, P, whisper_full_params, C.POINTER(whisper_amd_channels_params), P, C.c_int64, I, I)
        proto("whisper_amd_long_segment_channel", I, P, I)
        proto("whisper_amd_long_chunk_channel", I, P, I)
        proto("whisper_amd_channels_stats", None, P, I64P)
        proto("whisper_amd_channels_tile", I)
        proto("whisper_amd_channels_energy_lanes", I)
    if hasattr(lib, "whisper_amd_align"):
        proto("whisper_amd_align", I, P, P, whisper_full_params, P, I, C.POINTER(C.c_int32), I, C.POINTER(whisper_amd_align_token))
        proto("whisper_amd_align_score", I, P, C.POINTER(F), I, I, C.POINTER(C.c_int32), I, C.POINTER(whisper_amd_align_score))
        proto("whisper_amd_align_stats", None, P, C.POINTER(C.c_long))
        proto("whisper_amd_align_timings", None, P, C.POINTER(C.c_int64))
    if hasattr(lib, "whisper_amd_stream_open"):
        SP, FP = C.POINTER(whisper_amd_stream_params), C.POINTER(whisper_full_params)
        proto("whisper_amd_stream_default_params", None, SP)
        proto("whisper_amd_stream_open", P, P, SP)
        proto("whisper_amd_stream_close", None, P)
        proto("whisper_amd_stream_feed", I, P, P, C.c_int64)
        proto("whisper_amd_stream_flush", I, P)
        proto("whisper_amd_stream_pending", I, P)
        proto("whisper_amd_stream_step", I, P, FP)
        proto("whisper_amd_stream_step_many", I, C.POINTER(C.c_void_p), I, FP)
        proto("whisper_amd_stream_state", P, P)
        proto("whisper_amd_stream_info", I, P, C.POINTER(C.c_int64))
        proto("whisper_amd_stream_window_copy", C.c_int64, P, C.POINTER(F), C.c_int64)
        proto("whisper_amd_stream_prompt_copy", I, P, C.POINTER(C.c_int32), I)
        proto("whisper_amd_stream_reset", None, P)
        proto("whisper_amd_stream_tile", I)
    if hasattr(lib, "whisper_amd_stream_open_vad"):
        VP = C.POINTER(whisper_amd_stream_vad_params)
        proto("whisper_amd_stream_vad_default_params", None, VP)
        proto("whisper_amd_stream_open_vad", P, P, P, VP)
        proto("whisper_amd_stream_vad_poll_many", I, C.POINTER(C.c_void_p), I)
        proto("whisper_amd_stream_utterance_info", I, P, C.POINTER(C.c_int64))
        proto("whisper_amd_stream_vad_probs_copy", C.c_int64, P, C.POINTER(F), C.c_int64)
    _LIBS[path] = lib
    return lib


PCM_I16, PCM_F32 = 0, 1      # WHISPER_AMD_PCM_* (include/whisper_amd.h)
PCM_U8, PCM_S24, PCM_S32, PCM_F64, PCM_ULAW, PCM_ALAW = 3, 4, 5, 6, 7, 8
PCM_SAMPLE_BYTES = {PCM_I16: 2, PCM_F32: 4, PCM_U8: 1, PCM_S24: 3, PCM_S32: 4, PCM_F64: 8, PCM_ULAW: 1, PCM_ALAW: 1}
# what a host array of a format holds: S24 travels as its packed bytes (pack_s24)
PCM_DTYPE = {PCM_I16: np.int16, PCM_F32: np.float32, PCM_U8: np.uint8, PCM_S24: np.uint8, PCM_S32: np.int32, PCM_F64: np.float64,
             PCM_ULAW: np.uint8, PCM_ALAW: np.uint8}
WAV_BAD_ARGS, WAV_NOT_WAVE, WAV_MALFORMED, WAV_UNSUPPORTED, WAV_NO_DATA = -1, -2, -3, -4, -5      # whisper_amd_wav_parse's codes


def pcm_format_of(data, fmt: Optional[int]) -> int:
    """the format of a host array when none is given: int16 is I16, everything else is taken as F32 (the other formats are named)"""
    if fmt is None:
        return PCM_I16 if np.asarray(data).dtype == np.int16 else PCM_F32
    return fmt


def pcm_array(data, fmt: int) -> np.ndarray:
    """`data` as the flat contiguous array of format `fmt` that the C entries read"""
    return np.ascontiguousarray(data, dtype=PCM_DTYPE.get(fmt, np.float32)).reshape(-1)


def pcm_frames(a: np.ndarray, channels: int, fmt: int) -> int:
    """frames in a flat array of format `fmt`: its bytes over the bytes of one frame"""
    return a.nbytes // (PCM_SAMPLE_BYTES.get(fmt, 4) * max(channels, 1))


def pack_s24(samples) -> np.ndarray:
    """integers in [-2^23, 2^23) as packed 3-byte little-endian samples (uint8)"""
    s = np.asarray(samples, dtype=np.int32).reshape(-1)
    return np.ascontiguousarray(s.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


def ulaw_to_linear(codes) -> np.ndarray:
    """G.711 mu-law expansion to int16, the arithmetic of csrc/wa_audio.h (wa_audio_ulaw)"""
    u = ~np.asarray(codes, dtype=np.uint8).astype(np.int32) & 0xFF
    t = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    return np.where(u & 0x80, -t, t).astype(np.int16)


def alaw_to_linear(codes) -> np.ndarray:
    """G.711 A-law expansion to int16 (wa_audio_alaw)"""
    a = np.asarray(codes, dtype=np.uint8).astype(np.int32) ^ 0x55
    x = (a >> 4) & 7
    t = ((a & 15) << 4) + 8
    t = np.where(x > 0, (t + 0x100) << np.maximum(x - 1, 0), t)
    return np.where(a & 0x80, t, -t).astype(np.int16)


def linear_to_ulaw(samples) -> np.ndarray:
    """G.711 mu-law compression of int16 samples (bias 0x84, clip 32635): the code whose expansion lies nearest below in magnitude"""
    s = np.asarray(samples, dtype=np.int16).astype(np.int32)
    sign = np.where(s < 0, 0x80, 0)
    m = np.minimum(np.abs(s), 32635) + 0x84
    seg = np.frexp(m.astype(np.float64))[1].astype(np.int32) - 8       # floor(log2 m) - 7; m in [0x84, 0x7fff]: segments 0 .. 7
    return (~(sign | (seg << 4) | ((m >> (seg + 3)) & 15)) & 0xFF).astype(np.uint8)


def linear_to_alaw(samples) -> np.ndarray:
    """G.711 A-law compression of int16 samples: the code whose expansion lies nearest (the lower code where two are as near)"""
    table = alaw_to_linear(np.arange(256, dtype=np.uint8)).astype(np.int32)
    order = np.argsort(table, kind="stable")
    levels = table[order]
    s = np.asarray(samples, dtype=np.int16).astype(np.int32)
    hi = np.clip(np.searchsorted(levels, s), 1, 255)
    pick = np.where(s - levels[hi - 1] <= levels[hi] - s, hi - 1, hi)
    return order[pick].astype(np.uint8)


class whisper_amd_wav_info(C.Structure):
    _fields_ = [("data_offset", C.c_int64), ("n_frames", C.c_int64), ("channels", C.c_int32), ("sample_rate", C.c_int32), ("format", C.c_int32),
                ("bits", C.c_int32)]


def wav_parse(lib: C.CDLL, image) -> dict:
    """Extension (whisper_amd_wav_parse): the header of a RIFF/WAVE image (bytes or a uint8 array) as a dict of data_offset, n_frames, channels,
    sample_rate, format and bits; raises WhisperError with the entry's code where it refuses."""
    buf = np.frombuffer(bytes(image), np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else np.ascontiguousarray(image, dtype=np.uint8)
    w = whisper_amd_wav_info()
    rc = lib.whisper_amd_wav_parse(C.c_void_p(buf.ctypes.data if len(buf) else None), len(buf), C.byref(w))
    if rc != 0:
        raise WhisperError("WavRefused(%d)" % rc, rc)
    return {k: int(getattr(w, k)) for k, _ in whisper_amd_wav_info._fields_}


# whisper-rs' audio utilities (src/utilities.rs) restated in numpy, every operation rounded to F32 on its own
def convert_integer_to_float_audio(samples) -> np.ndarray:
    """i16 -> f32: s as f32 / 32768.0"""
    return np.asarray(samples, dtype=np.int16).astype(np.float32) / np.float32(32768.0)


def convert_stereo_to_mono_audio(samples) -> np.ndarray:
    """interleaved stereo f32 -> mono f32: (l + r) / 2.0; an odd number of samples is an error as in whisper-rs"""
    samples = np.asarray(samples, dtype=np.float32)
    if len(samples) % 2:
        raise WhisperError("HalfSampleMissing")
    return (samples[0::2] + samples[1::2]) / np.float32(2.0)


def convert_stereo_i16_to_mono_f32(samples) -> np.ndarray:
    """interleaved stereo i16 -> mono f32: (l as f32 + r as f32) / 2.0 / 32768.0"""
    samples = np.asarray(samples, dtype=np.int16)
    if len(samples) % 2:
        raise WhisperError("HalfSampleMissing")
    return (samples[0::2].astype(np.float32) + samples[1::2].astype(np.float32)) / np.float32(2.0) / np.float32(32768.0)


def audio_taps(lib: C.CDLL, sample_rate: int):
    """Extension (whisper_amd_audio_taps): (taps [L][K] F32, L, M, K) of the audio front end's filter for an input rate; None when the rate is refused."""
    L, M, K = C.c_int(), C.c_int(), C.c_int()
    n = lib.whisper_amd_audio_taps(sample_rate, None, 0, C.byref(L), C.byref(M), C.byref(K))
    if n < 0:
        return None
    t = np.zeros(max(n, 1), np.float32)
    lib.whisper_amd_audio_taps(sample_rate, t.ctypes.data_as(C.POINTER(C.c_float)), n, None, None, None)
    return t[:n].reshape(L.value, K.value), L.value, M.value, K.value


DTW_REFUSED, DTW_NOT_TAKEN, DTW_HIP_ERROR = -1, -2, -3      # whisper_amd_dtw_path's codes (include/whisper_amd.h)

_KEEP_LOG_CB = {}


def set_log_callback(lib: C.CDLL, fn=None):
    """Mirror of whisper-rs `install_logging_hooks` (src/lib.rs:67-70): route library logs to `fn(level, text)`.
    With fn=None logs are silenced."""
    cb = LOG_CB((lambda lvl, txt, ud: None) if fn is None else (lambda lvl, txt, ud: fn(lvl, (txt or b"").decode(errors="replace"))))
    _KEEP_LOG_CB[id(lib)] = cb
    lib.whisper_log_set(cb, None)


# ---------------------------------------------------------------------------------------------------
# whisper-rs mirror classes
# ---------------------------------------------------------------------------------------------------
class WhisperContextParameters:
    """src/whisper_ctx.rs:472-657 (`WhisperContextParameters`)."""

    def __init__(self, lib: C.CDLL, use_gpu: bool = True, flash_attn: bool = False, gpu_device: int = 0,
                 dtw_preset: int = AHEADS_NONE, dtw_n_top: int = -1, dtw_heads: Sequence[tuple] = ()):
        p = lib.whisper_context_default_params()
        p.use_gpu = use_gpu
        p.flash_attn = flash_attn
        p.gpu_device = gpu_device
        if dtw_preset != AHEADS_NONE:
            p.dtw_token_timestamps = True
            p.dtw_aheads_preset = dtw_preset
            p.dtw_n_top = dtw_n_top
            if dtw_preset == AHEADS_CUSTOM:
                self._heads = (whisper_ahead * len(dtw_heads))(*[whisper_ahead(a, b) for a, b in dtw_heads])
                p.dtw_aheads.n_heads = len(dtw_heads)
                p.dtw_aheads.heads = self._heads
        self.c = p


class FullParams:
    """src/whisper_params.rs:36-803 (`FullParams`): defaults from `whisper_full_default_params`, then setters."""

    def __init__(self, lib: C.CDLL, strategy: int = WHISPER_SAMPLING_GREEDY, **kw):
        self.c = lib.whisper_full_default_params(strategy)
        self._keep = {}
        # whisper-rs turns the C library's stdout printing off by default in its examples
        self.c.print_progress = False
        for k, v in kw.items():
            self.set(k, v)

    def set(self, name: str, value):
        if name == "best_of":
            self.c.greedy.best_of = value
        elif name == "beam_size":
            self.c.beam_search.beam_size = value
        elif name in ("language", "initial_prompt", "suppress_regex", "vad_model_path"):
            b = None if value is None else value.encode()
            self._keep[name] = b  # whisper-rs leaks the CString; we keep a reference
            setattr(self.c, name, b)
        elif name == "prompt_tokens":
            arr = (C.c_int32 * len(value))(*value)
            self._keep[name] = arr
            self.c.prompt_tokens = arr
            self.c.prompt_n_tokens = len(value)
        elif name == "grammar":
            # `value` = (rules, i_start_rule); rules[r] = the (type, value) elements of rule r, the closing END added here (None: a null
            # pointer in the array, for tests of the refusal).  whisper.h wants an
            # array of n_grammar_rules POINTERS, one END-terminated element array per rule; whisper-rs 0.14.3's own set_grammar hands over
            # one flat element array instead (src/whisper_params.rs:743-762), which no engine can read - this mirror follows the header.
            rules, i_start = value
            arrs = [None if r is None else
                    (whisper_grammar_element * (len(r) + 1))(*([whisper_grammar_element(t, v) for t, v in r] + [whisper_grammar_element(GRETYPE_END, 0)]))
                    for r in rules]
            ptrs = (C.c_void_p * max(1, len(arrs)))(*[None if a is None else C.addressof(a) for a in arrs])
            self._keep[name] = (arrs, ptrs)
            self.c.grammar_rules = C.cast(ptrs, C.c_void_p) if arrs else None
            self.c.n_grammar_rules = len(arrs)
            self.c.i_start_rule = i_start
        elif name.endswith("_callback"):
            ftype = dict(new_segment_callback=NEW_SEGMENT_CB, progress_callback=PROGRESS_CB,
                         encoder_begin_callback=ENCODER_BEGIN_CB, abort_callback=ABORT_CB,
                         logits_filter_callback=LOGITS_FILTER_CB)[name]
            cb = ftype(value)
            self._keep[name] = cb
            setattr(self.c, name, cb)
        else:
            setattr(self.c, name, value)
        return self


class WhisperContext:
    def __init__(self, lib: C.CDLL, ptr: int):
        self.lib, self.ptr = lib, ptr

    @classmethod
    def new_with_params(cls, path: str, params: Optional[WhisperContextParameters] = None,
                        lib: Optional[C.CDLL] = None) -> "WhisperContext":
        lib = lib or load_library()
        params = params or WhisperContextParameters(lib)
        ptr = lib.whisper_init_from_file_with_params_no_state(path.encode(), params.c)
        if not ptr:
            raise WhisperError("InitError")  # src/whisper_ctx.rs:38-42
        ctx = cls(lib, ptr)
        ctx._params = params
        return ctx

    @classmethod
    def new_from_buffer_with_params(cls, buf: bytes, params: Optional[WhisperContextParameters] = None,
                                    lib: Optional[C.CDLL] = None) -> "WhisperContext":
        lib = lib or load_library()
        params = params or WhisperContextParameters(lib)
        if isinstance(buf, np.ndarray):      # parsed in place (the library copies nothing beyond the call, whisper.cpp:3684-3719)
            arr = np.ascontiguousarray(buf, dtype=np.uint8)
            ptr = lib.whisper_init_from_buffer_with_params_no_state(C.c_void_p(arr.ctypes.data), arr.size, params.c)
        else:
            cbuf = C.create_string_buffer(buf, len(buf))
            ptr = lib.whisper_init_from_buffer_with_params_no_state(C.cast(cbuf, C.c_void_p), len(buf), params.c)
        if not ptr:
            raise WhisperError("InitError")
        ctx = cls(lib, ptr)
        ctx._params = params
        return ctx

    def create_state(self) -> "WhisperState":
        ptr = self.lib.whisper_init_state(self.ptr)
        if not ptr:
            raise WhisperError("InitError")
        return WhisperState(self, ptr)

    def __getattr__(self, name):
        # n_vocab(), model_n_text_layer(), token_eot(), ... -> whisper_<name>(ctx)
        if name.startswith("_"):
            raise AttributeError(name)
        fn = getattr(self.lib, "whisper_" + name)
        return lambda *a: fn(self.ptr, *a)

    def token_to_bytes(self, tok: int) -> bytes:
        return self.lib.whisper_token_to_str(self.ptr, tok)

    def tokenize(self, text: str, max_tokens: int = 1024) -> list[int]:
        arr = (C.c_int32 * max_tokens)()
        n = self.lib.whisper_tokenize(self.ptr, text.encode(), arr, max_tokens)
        if n < 0:
            raise WhisperError("InvalidText", n)
        return list(arr[:n])

    def load_stats(self) -> dict:
        """Extension (whisper_amd_load_stats): how the model was loaded."""
        out = (C.c_int64 * 6)()
        self.lib.whisper_amd_load_stats(self.ptr, out)
        return dict(zip(("path", "bytes_read", "kernels", "read_us", "wait_us", "load_us"), [int(v) for v in out]))

    def arena(self) -> np.ndarray:
        """Extension (whisper_amd_arena_read): the weight arena's bytes as the loader left them."""
        size = self.lib.whisper_amd_arena_read(self.ptr, 0, None, 0)
        if size < 0:
            raise WhisperError("ArenaRead")
        buf = np.empty(size, dtype=np.uint8)
        if self.lib.whisper_amd_arena_read(self.ptr, 0, C.c_void_p(buf.ctypes.data), size) != size:
            raise WhisperError("ArenaRead")
        return buf

    def free(self):
        if self.ptr:
            self.lib.whisper_free(self.ptr)
            self.ptr = None


def full_batch(ctx: "WhisperContext", states: Sequence["WhisperState"], params: "FullParams", pcms: Sequence) -> int:
    """Extension: transcribe several independent chunks concurrently on one device (whisper_amd_full_batch).
    `pcms[i]` is a numpy f32 array or a (device_ptr, n) tuple."""
    n = len(states)
    keep, ptrs, lens = [], (C.c_void_p * n)(), (C.c_int * n)()
    for i, p in enumerate(pcms):
        if isinstance(p, tuple):
            ptrs[i], lens[i] = p[0], p[1]
        else:
            a = np.ascontiguousarray(p, dtype=np.float32); keep.append(a)
            ptrs[i], lens[i] = a.ctypes.data, len(a)
    sp = (C.c_void_p * n)(*[s.ptr for s in states])
    r = ctx.lib.whisper_amd_full_batch(ctx.ptr, sp, n, params.c, ptrs, lens)
    if r != 0:
        raise WhisperError("GenericError(%d)" % r, r)
    return r


def rows_debug_rows(ctx: "WhisperContext", states: Sequence["WhisperState"], tokens: Sequence[int], n_past: Sequence[int]):
    """Extension (whisper_amd_rows_debug_rows): the several-rows one-launch step with a state, a token and a context length per row.
    Returns (return code, logits [B][n_vocab], row status words [B])."""
    n = len(states)
    logits = np.zeros((n, ctx.n_vocab()), dtype=np.float32)
    status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    sp = (C.c_void_p * n)(*[s.ptr for s in states])
    rc = ctx.lib.whisper_amd_rows_debug_rows(ctx.ptr, sp, n, (C.c_int * n)(*tokens), (C.c_int * n)(*n_past), logits.ctypes.data_as(C.POINTER(C.c_float)),
                                             status.ctypes.data_as(C.POINTER(C.c_uint)))
    return rc, logits, status


class WhisperState:
    def __init__(self, ctx: WhisperContext, ptr: int):
        self.ctx, self.lib, self.ptr = ctx, ctx.lib, ptr

    # -- low level stage API (src/whisper_state.rs:50-260) ---------------------------------------
    def pcm_to_mel(self, pcm: np.ndarray, n_threads: int = 1):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        r = self.lib.whisper_pcm_to_mel_with_state(self.ctx.ptr, self.ptr, pcm.ctypes.data_as(C.POINTER(C.c_float)),
                                                   len(pcm), n_threads)
        if r != 0:
            raise WhisperError("UnableToCalculateSpectrogram", r)

    def set_mel(self, mel: np.ndarray):
        """mel: [n_mel][n_len] f32 (layout of whisper.cpp:3904-3923)."""
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        n_mel, n_len = mel.shape
        r = self.lib.whisper_set_mel_with_state(self.ctx.ptr, self.ptr, mel.ctypes.data_as(C.POINTER(C.c_float)),
                                                n_len, n_mel)
        if r != 0:
            raise WhisperError("InvalidMelBands", r)

    def encode(self, offset: int = 0, n_threads: int = 1):
        r = self.lib.whisper_encode_with_state(self.ctx.ptr, self.ptr, offset, n_threads)
        if r != 0:
            raise WhisperError("UnableToCalculateEvaluation", r)

    def decode(self, tokens: Sequence[int], n_past: int, n_threads: int = 1):
        arr = (C.c_int32 * len(tokens))(*tokens)
        r = self.lib.whisper_decode_with_state(self.ctx.ptr, self.ptr, arr, len(tokens), n_past, n_threads)
        if r != 0:
            raise WhisperError("UnableToCalculateEvaluation", r)

    def get_logits_last(self, n_tokens: int) -> np.ndarray:
        """Row n_tokens-1 of the logits of the last decode() (the only valid row, whisper.cpp:2965-2971)."""
        nv = self.ctx.n_vocab()
        p = self.lib.whisper_get_logits_from_state(self.ptr)
        return np.ctypeslib.as_array(p, shape=(n_tokens * nv,))[(n_tokens - 1) * nv:].copy()

    def lang_detect(self, offset_ms: int = 0, n_threads: int = 1):
        probs = (C.c_float * (self.lib.whisper_lang_max_id() + 1))()
        r = self.lib.whisper_lang_auto_detect_with_state(self.ctx.ptr, self.ptr, offset_ms, n_threads, probs)
        if r < 0:
            raise WhisperError("GenericError", r)
        return r, np.array(probs[:], dtype=np.float32)

    def qgemm_stats(self) -> tuple:
        """Extension: (quantised products of more than 8 rows served by the int8 matrix-core kernel, served by k_qgemm_exact) since the state was created."""
        out = (C.c_long * 2)()
        self.lib.whisper_amd_qgemm_stats(self.ptr, out)
        return int(out[0]), int(out[1])

    def few_rows_stats(self) -> tuple:
        """Extension: (quantised products of 2..8 rows issued or captured that a few-rows kernel took, that the general kernel took) since the state was created."""
        out = (C.c_long * 2)()
        self.lib.whisper_amd_few_rows_stats(self.ptr, out)
        return int(out[0]), int(out[1])

    def rows_stats(self) -> tuple:
        """Extension: (decoder passes of several token rows served by the one-launch form, passes sent back to the launch sequence)."""
        out = (C.c_long * 2)()
        self.lib.whisper_amd_rows_stats(self.ptr, out)
        return int(out[0]), int(out[1])

    def decode_batch(self, tokens: Sequence[int], pos: Sequence[int], seq_id: Sequence[int], logits: Sequence[int]) -> np.ndarray:
        """Extension (whisper_amd_decode_batch): one decoder pass over a batch as whisper_full builds it; no cell is removed first.  Returns the logits
        rows of the flagged tokens, [number of flagged rows][n_vocab], in batch order."""
        n = len(tokens)
        assert len(pos) == n and len(seq_id) == n and len(logits) == n
        r = self.lib.whisper_amd_decode_batch(self.ctx.ptr, self.ptr, (C.c_int32 * n)(*tokens), (C.c_int32 * n)(*pos), (C.c_int32 * n)(*seq_id),
                                              (C.c_int8 * n)(*[1 if f else 0 for f in logits]), n)
        if r != 0:
            raise WhisperError("UnableToCalculateEvaluation", r)
        nv = self.ctx.n_vocab()
        rows = np.ctypeslib.as_array(self.lib.whisper_get_logits_from_state(self.ptr), shape=(n, nv))
        return rows[[i for i in range(n) if logits[i]]].copy()

    def kv_op(self, op: int, a: int = 0, b: int = 0, p0: int = -1, p1: int = -1) -> int:
        """Extension (whisper_amd_kv_op): 0 clear, 1 seq_rm(a, p0, p1), 2 seq_cp(a -> b, p0, p1), 3 a new cache of `a` cells, 4 / 5 / 6 the cache's
        n / head / size."""
        r = self.lib.whisper_amd_kv_op(self.ptr, op, a, b, p0, p1)
        if r < 0:
            raise WhisperError("KvOp(%d)" % op, r)
        return r

    def dtw_path(self, qk: np.ndarray, n_audio_tokens: int, sot_len: int, medfilt_width: int = 7, where: int = 0, cap: int = None, fill: int = -1):
        """Extension (whisper_amd_dtw_path): the DTW alignment alone over a host cube qk [n_heads][n_tokens][n_ctx] F32.  where = 0: the host
        function, 1: the device kernels.  Returns (the path length or a DTW_* code, token indices, time indices); the two arrays have `cap`
        entries (default N + M), pre-filled with `fill`, of which the first min(length, cap) are the path."""
        qk = np.ascontiguousarray(qk, dtype=np.float32)
        n_heads, n_tokens, n_ctx = qk.shape
        if cap is None:
            cap = max(1, n_tokens + n_audio_tokens)
        tok, tim = np.full(cap, fill, dtype=np.int32), np.full(cap, fill, dtype=np.int32)
        r = self.lib.whisper_amd_dtw_path(self.ptr, qk.ctypes.data_as(C.POINTER(C.c_float)), n_heads, n_tokens, n_ctx, n_audio_tokens, sot_len, medfilt_width,
                                          where, tok.ctypes.data_as(C.POINTER(C.c_int32)), tim.ctypes.data_as(C.POINTER(C.c_int32)), cap)
        return r, tok, tim

    def dtw_stats(self) -> tuple:
        """Extension: DTW calls on this state (served by the device path, served by the host path, device-path attempts that fell back)."""
        out = (C.c_long * 3)()
        self.lib.whisper_amd_dtw_stats(self.ptr, out)
        return int(out[0]), int(out[1]), int(out[2])

    def dtw_timings(self) -> tuple:
        """Extension: (wall time in us of full()'s DTW post-processing on this state - decoder pass done to t_dtw placed -, number of such calls)."""
        out = (C.c_int64 * 2)()
        self.lib.whisper_amd_dtw_timings(self.ptr, out)
        return int(out[0]), int(out[1])

    # -- forced alignment (whisper_amd_align*): times and log-probabilities of a known transcript --------------------------------
    def align(self, params: "FullParams", pcm, ids: Sequence[int]) -> list[dict]:
        """Extension (whisper_amd_align): one window of `pcm` (numpy f32 array on the host, or (device pointer, n)) against the text tokens `ids`.
        Returns len(ids) + 1 dicts {id, plog, p, best_id, best_plog, rank, t_dtw}; the last one is the closing eot's.  Scores are the model's
        own (raw logits, no sampler rules); t_dtw is -1 without alignment heads.  Raises WhisperError with the C code on refusal."""
        if isinstance(pcm, tuple):
            ptr, n = pcm
        else:
            self._pcm_keep = pcm = np.ascontiguousarray(pcm, dtype=np.float32)
            ptr, n = (pcm.ctypes.data if len(pcm) else None), len(pcm)
        n_tok = len(ids)
        out = (whisper_amd_align_token * (n_tok + 1))()
        r = self.lib.whisper_amd_align(self.ctx.ptr, self.ptr, params.c, C.c_void_p(ptr), n, (C.c_int32 * max(n_tok, 1))(*ids), n_tok, out)
        if r != 0:
            raise WhisperError("AlignError(%d)" % r, r)
        return [dict(id=o.id, plog=o.plog, p=o.p, best_id=o.best_id, best_plog=o.best_plog, rank=o.rank, t_dtw=o.t_dtw) for o in out]

    def align_text(self, params: "FullParams", pcm, text: str) -> list[dict]:
        """align() on the tokens whisper_tokenize gives for `text`"""
        return self.align(params, pcm, self.ctx.tokenize(text))

    def align_score(self, logits: np.ndarray, target: Sequence[int], where: int = 1) -> np.ndarray:
        """Extension (whisper_amd_align_score): the scores alone over host logits [n_rows][n_vocab].  where = 0: the host function, 1: the kernel on
        this state's stream.  Returns a structured array with fields plog, p, best_id, best_plog, rank, best_p."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        n_rows, n_vocab = logits.shape
        tgt = np.ascontiguousarray(target, dtype=np.int32)
        assert len(tgt) == n_rows
        out = (whisper_amd_align_score * n_rows)()
        r = self.lib.whisper_amd_align_score(self.ptr, logits.ctypes.data_as(C.POINTER(C.c_float)), n_rows, n_vocab, tgt.ctypes.data_as(C.POINTER(C.c_int32)),
                                             where, out)
        if r != 0:
            raise WhisperError("AlignError(%d)" % r, r)
        return np.frombuffer(out, dtype=ALIGN_SCORE_DTYPE).copy()

    def align_stats(self) -> tuple:
        """Extension: (align() calls that succeeded, logits rows scored on the device, bytes of logits that stayed on the device) since the state was created."""
        out = (C.c_long * 3)()
        self.lib.whisper_amd_align_stats(self.ptr, out)
        return int(out[0]), int(out[1]), int(out[2])

    def align_timings(self) -> tuple:
        """Extension: (device time in us of the last score kernel launch between two HIP events, wall time in us of the last align() call)."""
        out = (C.c_int64 * 2)()
        self.lib.whisper_amd_align_timings(self.ptr, out)
        return int(out[0]), int(out[1])

    # -- audio front end (whisper_amd_audio_*): int16 / F32, mono / stereo, 8 .. 192 kHz -> 16 kHz mono F32 on the device -------
    def _audio_args(self, data, channels, fmt):
        """`data`: a numpy array of interleaved samples on the host - int16 or float32, or what PCM_DTYPE names for a `fmt` given (S24: packed
        bytes) -, or (device pointer, n_frames) with `fmt` given"""
        if isinstance(data, tuple):
            return data[0], int(data[1]), fmt
        fmt = pcm_format_of(data, fmt)
        data = pcm_array(data, fmt)
        self._audio_keep = data
        return (data.ctypes.data if len(data) else None), pcm_frames(data, channels, fmt), fmt

    def audio_to_pcm(self, data, channels: int, sample_rate: int, fmt: Optional[int] = None) -> tuple:
        """Extension (whisper_amd_audio_to_pcm): returns (device pointer, n_samples) of the 16 kHz mono F32 audio, valid until the next call
        on this state; pass the pair to full() or pcm_to_mel_device()."""
        ptr, n_frames, fmt = self._audio_args(data, channels, fmt)
        n = C.c_int64(-1)
        r = self.lib.whisper_amd_audio_to_pcm(self.ptr, C.c_void_p(ptr), n_frames, channels, sample_rate, fmt, C.byref(n))
        if not r:
            raise WhisperError("AudioRefused", -1)
        return r, int(n.value)

    def full_audio(self, params: "FullParams", data, channels: int, sample_rate: int, fmt: Optional[int] = None) -> int:
        """Extension (whisper_amd_full_audio): audio_to_pcm + full() without a host copy of the PCM."""
        ptr, n_frames, fmt = self._audio_args(data, channels, fmt)
        r = self.lib.whisper_amd_full_audio(self.ctx.ptr, self.ptr, params.c, C.c_void_p(ptr), n_frames, channels, sample_rate, fmt)
        if r != 0:
            raise WhisperError("GenericError(%d)" % r, r)
        return r

    def audio_copy(self) -> np.ndarray:
        """Extension (whisper_amd_audio_copy): the last audio_to_pcm / full_audio result as a host array."""
        n = self.lib.whisper_amd_audio_copy(self.ptr, None, 0)
        if n < 0:
            raise WhisperError("NoAudio", int(n))
        out = np.zeros(max(n, 1), np.float32)
        if self.lib.whisper_amd_audio_copy(self.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n) != n:
            raise WhisperError("NoAudio", -1)
        return out[:n]

    # -- two-channel recordings (whisper_amd_audio_split, whisper_amd_channel_*) ------------------
    def audio_split(self, data, sample_rate: int, fmt: Optional[int] = None) -> tuple:
        """Extension (whisper_amd_audio_split): `data` interleaved stereo as _audio_args takes it.  Returns (device pointer, n_samples, stride):
        channel c lies at pointer + 4 * c * stride bytes, valid until the next split on this state."""
        ptr, n_frames, fmt = self._audio_args(data, 2, fmt)
        n, stride = C.c_int64(-1), C.c_int64(-1)
        r = self.lib.whisper_amd_audio_split(self.ptr, C.c_void_p(ptr), n_frames, sample_rate, fmt, C.byref(n), C.byref(stride))
        if not r:
            raise WhisperError("AudioRefused", -1)
        return r, int(n.value), int(stride.value)

    def audio_split_copy(self, channel: int) -> np.ndarray:
        """Extension (whisper_amd_audio_split_copy): plane `channel` of the last audio_split as a host array."""
        n = self.lib.whisper_amd_audio_split_copy(self.ptr, channel, None, 0)
        if n < 0:
            raise WhisperError("NoAudio", int(n))
        out = np.zeros(max(n, 1), np.float32)
        if self.lib.whisper_amd_audio_split_copy(self.ptr, channel, out.ctypes.data_as(C.POINTER(C.c_float)), n) != n:
            raise WhisperError("NoAudio", -1)
        return out[:n]

    def channel_energy(self, spans, where: int = -1) -> np.ndarray:
        """Extension (whisper_amd_channel_energy): `spans` [(first sample, end sample)] -> float64 [n][2]; where 0 host, 1 kernel, else either."""
        a = np.ascontiguousarray([s[0] for s in spans], dtype=np.int64)
        b = np.ascontiguousarray([s[1] for s in spans], dtype=np.int64)
        e = np.full((max(len(spans), 1), 2), np.nan, np.float64)
        I64P = C.POINTER(C.c_int64)
        if self.lib.whisper_amd_channel_energy(self.ptr, a.ctypes.data_as(I64P), b.ctypes.data_as(I64P), len(spans), where,
                                               e.ctypes.data_as(C.POINTER(C.c_double))) != 0:
            raise WhisperError("GenericError", -1)
        return e[:len(spans)]

    def channel_speakers(self, times_cs, ratio: float = 0.0) -> tuple:
        """Extension (whisper_amd_channel_speakers): `times_cs` [(t0, t1)] in centiseconds -> (labels int8 [n]: 0, 1, -1 = undecided; energies [n][2])."""
        a = np.ascontiguousarray([t[0] for t in times_cs], dtype=np.int64)
        b = np.ascontiguousarray([t[1] for t in times_cs], dtype=np.int64)
        e = np.full((max(len(times_cs), 1), 2), np.nan, np.float64)
        lab = np.full(max(len(times_cs), 1), -2, np.int8)
        I64P = C.POINTER(C.c_int64)
        if self.lib.whisper_amd_channel_speakers(self.ptr, a.ctypes.data_as(I64P), b.ctypes.data_as(I64P), len(times_cs), ratio,
                                                 e.ctypes.data_as(C.POINTER(C.c_double)), lab.ctypes.data_as(C.POINTER(C.c_int8))) != 0:
            raise WhisperError("GenericError", -1)
        return lab[:len(times_cs)], e[:len(times_cs)]

    def audio_stats(self) -> tuple:
        """Extension: audio front end calls on this state (served by the kernels, served by the host restatement, kernel attempts that fell back)."""
        out = (C.c_long * 3)()
        self.lib.whisper_amd_audio_stats(self.ptr, out)
        return int(out[0]), int(out[1]), int(out[2])

    def pcm_to_mel_device(self, ptr: int, n: int, n_threads: int = 1):
        """pcm_to_mel on PCM that lies in device memory (e.g. audio_to_pcm's result)"""
        r = self.lib.whisper_pcm_to_mel_with_state(self.ctx.ptr, self.ptr, C.cast(C.c_void_p(ptr), C.POINTER(C.c_float)), n, n_threads)
        if r != 0:
            raise WhisperError("UnableToCalculateSpectrogram", r)

    def n_len(self) -> int:
        return self.lib.whisper_n_len_from_state(self.ptr)

    # -- full pipeline (src/whisper_state.rs:289-321) ---------------------------------------------
    def full(self, params: FullParams, pcm) -> int:
        """`pcm`: numpy f32 array on the host, or an int device pointer + length tuple (ptr, n)."""
        if isinstance(pcm, tuple):
            ptr, n = pcm
        else:
            pcm = np.ascontiguousarray(pcm, dtype=np.float32)
            if len(pcm) == 0:
                raise WhisperError("NoSamples")  # src/whisper_state.rs:294-298
            self._pcm_keep = pcm
            ptr, n = pcm.ctypes.data, len(pcm)
        r = self.lib.whisper_full_with_state(self.ctx.ptr, self.ptr, params.c, C.c_void_p(ptr), n)
        if r != 0:
            raise WhisperError("GenericError(%d)" % r, r)  # src/whisper_state.rs:310-320
        return r

    def full_n_segments(self) -> int:
        return self.lib.whisper_full_n_segments_from_state(self.ptr)

    def full_lang_id(self) -> int:
        return self.lib.whisper_full_lang_id_from_state(self.ptr)

    def full_get_segment_t0(self, i: int) -> int:
        return self.lib.whisper_full_get_segment_t0_from_state(self.ptr, i)

    def full_get_segment_t1(self, i: int) -> int:
        return self.lib.whisper_full_get_segment_t1_from_state(self.ptr, i)

    def full_get_segment_bytes(self, i: int) -> bytes:
        return self.lib.whisper_full_get_segment_text_from_state(self.ptr, i)

    def full_get_segment_text(self, i: int) -> str:
        return self.full_get_segment_bytes(i).decode(errors="replace")

    def full_get_segment_no_speech_prob(self, i: int) -> float:
        return self.lib.whisper_full_get_segment_no_speech_prob_from_state(self.ptr, i)

    def full_n_tokens(self, i: int) -> int:
        return self.lib.whisper_full_n_tokens_from_state(self.ptr, i)

    def full_get_token_id(self, i: int, j: int) -> int:
        return self.lib.whisper_full_get_token_id_from_state(self.ptr, i, j)

    def full_get_token_data(self, i: int, j: int) -> whisper_token_data:
        return self.lib.whisper_full_get_token_data_from_state(self.ptr, i, j)

    def full_get_token_prob(self, i: int, j: int) -> float:
        return self.lib.whisper_full_get_token_p_from_state(self.ptr, i, j)

    def full_get_token_bytes(self, i: int, j: int) -> bytes:
        return self.lib.whisper_full_get_token_text_from_state(self.ctx.ptr, self.ptr, i, j)

    def segments(self) -> list[dict]:
        """Convenience: everything the examples print (examples/basic_use.rs:330-341) + token ids."""
        out = []
        for i in range(self.full_n_segments()):
            nt = self.full_n_tokens(i)
            toks = [self.full_get_token_data(i, j) for j in range(nt)]
            out.append(dict(t0=self.full_get_segment_t0(i), t1=self.full_get_segment_t1(i),
                            text=self.full_get_segment_bytes(i),
                            ids=[t.id for t in toks], tids=[t.tid for t in toks],
                            p=[t.p for t in toks], plog=[t.plog for t in toks],
                            pt=[t.pt for t in toks], ptsum=[t.ptsum for t in toks],
                            t_dtw=[t.t_dtw for t in toks],
                            tok_t0=[t.t0 for t in toks], tok_t1=[t.t1 for t in toks], vlen=[t.vlen for t in toks],
                            no_speech_prob=self.full_get_segment_no_speech_prob(i)))
        return out

    def free(self):
        if self.ptr:
            self.lib.whisper_free_state(self.ptr)
            self.ptr = None


# ---------------------------------------------------------------------------------------------------
# voice activity detection (whisper.h: whisper_vad_*) and whisper_full on the context's own state
# ---------------------------------------------------------------------------------------------------
def vad_params(lib: C.CDLL, threshold=None, min_speech_duration_ms=None, min_silence_duration_ms=None, max_speech_duration_s=None,
               speech_pad_ms=None, samples_overlap=None) -> whisper_vad_params:
    """`whisper_vad_default_params()` with the given fields replaced."""
    p = lib.whisper_vad_default_params()
    for k, v in dict(threshold=threshold, min_speech_duration_ms=min_speech_duration_ms, min_silence_duration_ms=min_silence_duration_ms,
                     max_speech_duration_s=max_speech_duration_s, speech_pad_ms=speech_pad_ms, samples_overlap=samples_overlap).items():
        if v is not None:
            setattr(p, k, v)
    return p


def _f32(pcm) -> np.ndarray:
    return np.ascontiguousarray(pcm, dtype=np.float32)


class WhisperVadContext:
    """whisper_vad_context: `detect_speech` leaves one probability per 512 samples, `segments_*` turn them into (t0, t1) centiseconds."""

    def __init__(self, lib: C.CDLL, ptr: int):
        self.lib, self.ptr = lib, ptr

    @staticmethod
    def _params(lib, n_threads, gpu_device):
        p = lib.whisper_vad_default_context_params()
        if n_threads is not None:
            p.n_threads = n_threads
        p.gpu_device = gpu_device
        return p

    @classmethod
    def new(cls, path: str, lib: Optional[C.CDLL] = None, n_threads: Optional[int] = None, gpu_device: int = 0) -> "WhisperVadContext":
        lib = lib or load_library()
        ptr = lib.whisper_vad_init_from_file_with_params(path.encode(), cls._params(lib, n_threads, gpu_device))
        if not ptr:
            raise WhisperError("InitError")
        return cls(lib, ptr)

    @classmethod
    def new_from_loader(cls, data: bytes, lib: Optional[C.CDLL] = None, n_threads: Optional[int] = None, gpu_device: int = 0) -> "WhisperVadContext":
        """Through `whisper_vad_init_with_params` with a whisper_model_loader that serves `data`."""
        lib = lib or load_library()
        pos = [0]

        def rd(_ctx, out, n):
            k = min(n, len(data) - pos[0])
            if k > 0:
                C.memmove(out, data[pos[0]:pos[0] + k], k)
            hit_end = k < n
            pos[0] += k
            if hit_end:
                pos[0] = len(data) + 1            # like a stream: eof is set by a read that runs past the end
            return k

        loader = whisper_model_loader(None, LOADER_READ(rd), LOADER_EOF(lambda _c: pos[0] > len(data)), LOADER_CLOSE(lambda _c: None))
        ptr = lib.whisper_vad_init_with_params(C.byref(loader), cls._params(lib, n_threads, gpu_device))
        if not ptr:
            raise WhisperError("InitError")
        return cls(lib, ptr)

    def detect_speech(self, pcm) -> np.ndarray:
        pcm = _f32(pcm)
        if not self.lib.whisper_vad_detect_speech(self.ptr, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm)):
            raise WhisperError("GenericError")
        return self.probs()

    def probs(self) -> np.ndarray:
        n = self.lib.whisper_vad_n_probs(self.ptr)
        if n == 0:
            return np.zeros(0, dtype=np.float32)
        return np.ctypeslib.as_array(self.lib.whisper_vad_probs(self.ptr), shape=(n,)).copy()

    def _take(self, seg) -> list[tuple]:
        if not seg:
            raise WhisperError("GenericError")
        out = [(self.lib.whisper_vad_segments_get_segment_t0(seg, i), self.lib.whisper_vad_segments_get_segment_t1(seg, i))
               for i in range(self.lib.whisper_vad_segments_n_segments(seg))]
        self.lib.whisper_vad_free_segments(seg)
        return out

    def segments_from_probs(self, params: whisper_vad_params) -> list[tuple]:
        return self._take(self.lib.whisper_vad_segments_from_probs(self.ptr, params))

    def segments_from_samples(self, params: whisper_vad_params, pcm) -> list[tuple]:
        pcm = _f32(pcm)
        return self._take(self.lib.whisper_vad_segments_from_samples(self.ptr, params, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm)))

    def front(self, pcm) -> np.ndarray:
        """Extension (whisper_amd_vad_front): the device front end's [n_chunks][512] LSTM gate inputs."""
        pcm = _f32(pcm)
        n = self.lib.whisper_amd_vad_front(self.ptr, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm), None, 0)
        if n < 0:
            raise WhisperError("GenericError", int(n))
        out = np.empty(n, dtype=np.float32)
        if self.lib.whisper_amd_vad_front(self.ptr, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm), out.ctypes.data_as(C.POINTER(C.c_float)), n) != n:
            raise WhisperError("GenericError")
        return out.reshape(-1, 512)

    def free(self):
        if self.ptr:
            self.lib.whisper_vad_free(self.ptr)
            self.ptr = None


class WhisperFullContext:
    """A context WITH its own state (`whisper_init_from_file_with_params`): `whisper_full`, `whisper_full_parallel` and the
    context-level getters - the entry points that honour `vad = true`."""

    def __init__(self, lib: C.CDLL, ptr: int):
        self.lib, self.ptr = lib, ptr

    @classmethod
    def new_with_params(cls, path: str, params: Optional[WhisperContextParameters] = None, lib: Optional[C.CDLL] = None) -> "WhisperFullContext":
        lib = lib or load_library()
        params = params or WhisperContextParameters(lib)
        ptr = lib.whisper_init_from_file_with_params(path.encode(), params.c)
        if not ptr:
            raise WhisperError("InitError")
        ctx = cls(lib, ptr)
        ctx._params = params
        return ctx

    def full(self, params: FullParams, pcm) -> int:
        pcm = _f32(pcm)
        return self.lib.whisper_full(self.ptr, params.c, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm))

    def full_parallel(self, params: FullParams, pcm, n_processors: int) -> int:
        pcm = _f32(pcm)
        return self.lib.whisper_full_parallel(self.ptr, params.c, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm), n_processors)

    def segments(self) -> list[dict]:
        out = []
        for i in range(self.lib.whisper_full_n_segments(self.ptr)):
            toks = [self.lib.whisper_full_get_token_data(self.ptr, i, j) for j in range(self.lib.whisper_full_n_tokens(self.ptr, i))]
            out.append(dict(t0=self.lib.whisper_full_get_segment_t0(self.ptr, i), t1=self.lib.whisper_full_get_segment_t1(self.ptr, i),
                            text=self.lib.whisper_full_get_segment_text(self.ptr, i), ids=[t.id for t in toks],
                            tok_t0=[t.t0 for t in toks], tok_t1=[t.t1 for t in toks]))
        return out

    # -- long recordings (whisper_amd_full_long, whisper_amd_long_*) -------------------------------
    def state_ptr(self) -> int:
        """Extension (whisper_amd_context_state): the context's own state, for the calls that take one."""
        return self.lib.whisper_amd_context_state(self.ptr)

    def full_long(self, params: FullParams, pcm, max_chunk_ms: int = 0, n_parallel: int = 0) -> int:
        """Extension (whisper_amd_full_long).  `pcm`: numpy f32 array on the host, or (device pointer, n)."""
        if isinstance(pcm, tuple):
            ptr, n = pcm
        else:
            self._pcm_keep = pcm = _f32(pcm)
            ptr, n = pcm.ctypes.data, len(pcm)
        return self.lib.whisper_amd_full_long(self.ptr, params.c, C.c_void_p(ptr), n, max_chunk_ms, n_parallel)

    def full_long_audio(self, params: FullParams, data, channels: int, sample_rate: int, fmt: Optional[int] = None, max_chunk_ms: int = 0,
                        n_parallel: int = 0) -> int:
        """Extension (whisper_amd_full_long_audio): interleaved samples of any format (int16 or float32 where `fmt` is not given) at any supported rate."""
        fmt = pcm_format_of(data, fmt)
        self._audio_keep = data = pcm_array(data, fmt)
        return self.lib.whisper_amd_full_long_audio(self.ptr, params.c, C.c_void_p(data.ctypes.data), pcm_frames(data, channels, fmt), channels,
                                                    sample_rate, fmt, max_chunk_ms, n_parallel)

    def long_chunks(self) -> list[dict]:
        """Extension (whisper_amd_long_chunk_info): the last call's chunks."""
        out, v = [], (C.c_int64 * 6)()
        for i in range(self.lib.whisper_amd_long_n_chunks(self.ptr)):
            if self.lib.whisper_amd_long_chunk_info(self.ptr, i, v) != 0:
                raise WhisperError("GenericError", -1)
            out.append(dict(first=int(v[0]), count=int(v[1]), packed=int(v[2]), t0=int(v[3]), t1=int(v[4]), n_result=int(v[5])))
        return out

    def long_chunk_copy(self, i: int) -> np.ndarray:
        """Extension (whisper_amd_long_chunk_copy): the packed PCM of chunk i."""
        n = self.lib.whisper_amd_long_chunk_copy(self.ptr, i, None, 0)
        if n < 0:
            raise WhisperError("NoChunk", int(n))
        out = np.zeros(max(n, 1), np.float32)
        if self.lib.whisper_amd_long_chunk_copy(self.ptr, i, out.ctypes.data_as(C.POINTER(C.c_float)), n) != n:
            raise WhisperError("NoChunk", -1)
        return out[:n]

    def long_stats(self) -> dict:
        """Extension (whisper_amd_long_stats) of the last whisper_amd_full_long call."""
        v = (C.c_int64 * 8)()
        self.lib.whisper_amd_long_stats(self.ptr, v)
        return dict(zip(("path", "fallbacks", "chunks", "waves", "vad_us", "pack_us", "transcribe_us", "h2d_bytes"), (int(x) for x in v)))

    def long_pack(self, pcm, segs, overlap: float, runs, where: int) -> int:
        """Extension (whisper_amd_long_pack) on the context's state: `segs` [(start cs, end cs)], `runs` [(first, count)]; `pcm` as full_long."""
        if isinstance(pcm, tuple):
            ptr, n = pcm
        else:
            self._pcm_keep = pcm = _f32(pcm)
            ptr, n = pcm.ctypes.data, len(pcm)
        s = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1)
        first = np.ascontiguousarray([r[0] for r in runs], dtype=np.int32)
        count = np.ascontiguousarray([r[1] for r in runs], dtype=np.int32)
        return self.lib.whisper_amd_long_pack(self.state_ptr(), C.c_void_p(ptr), n, s.ctypes.data_as(C.POINTER(C.c_int64)), len(s) // 2, overlap,
                                              first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_int32)), len(runs), where)

    # -- two-channel recordings (whisper_amd_full_long_channels) ----------------------------------
    def full_long_channels(self, params: FullParams, data, sample_rate: int, fmt: Optional[int] = None, max_chunk_ms: int = 0, n_parallel: int = 0,
                           crosstalk_ratio: float = 0.0) -> int:
        """Extension (whisper_amd_full_long_channels).  `data`: interleaved stereo int16 / float32 on the host, or (device pointer, n_frames) with `fmt`."""
        if isinstance(data, tuple):
            ptr, n_frames = data
        else:
            fmt = pcm_format_of(data, fmt)
            self._audio_keep = data = pcm_array(data, fmt)
            ptr, n_frames = (data.ctypes.data if len(data) else None), pcm_frames(data, 2, fmt)
        cp = whisper_amd_channels_params()
        self.lib.whisper_amd_channels_default_params(C.byref(cp))
        cp.max_chunk_ms, cp.n_parallel, cp.crosstalk_ratio = max_chunk_ms, n_parallel, crosstalk_ratio
        return self.lib.whisper_amd_full_long_channels(self.ptr, params.c, C.byref(cp), C.c_void_p(ptr), n_frames, sample_rate, fmt)

    def segment_channels(self) -> list[int]:
        """Extension (whisper_amd_long_segment_channel): the channel of every result segment; -1 where the last long call had no channels."""
        return [self.lib.whisper_amd_long_segment_channel(self.ptr, i) for i in range(self.lib.whisper_full_n_segments(self.ptr))]

    def chunk_channels(self) -> list[int]:
        """Extension (whisper_amd_long_chunk_channel): the channel of every chunk of the last call, in wave order."""
        return [self.lib.whisper_amd_long_chunk_channel(self.ptr, i) for i in range(self.lib.whisper_amd_long_n_chunks(self.ptr))]

    def channels_stats(self) -> dict:
        """Extension (whisper_amd_channels_stats) of the last whisper_amd_full_long_channels call."""
        v = (C.c_int64 * 11)()
        self.lib.whisper_amd_channels_stats(self.ptr, v)
        return dict(zip(("split_path", "split_fallbacks", "energy_launches", "pack_launches", "segments_0", "segments_1", "dropped", "chunks", "waves",
                         "h2d_bytes", "energy_fallbacks"), (int(x) for x in v)))

    def batch_stats(self) -> tuple:
        """Extension (whisper_amd_batch_stats): lock-step passes of the last batch / parallel / long call and the rows they served."""
        a, b = C.c_long(0), C.c_long(0)
        self.lib.whisper_amd_batch_stats(self.ptr, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def free(self):
        if self.ptr:
            self.lib.whisper_free(self.ptr)
            self.ptr = None


def long_plan(lib: C.CDLL, segs, n_samples: int, overlap: float, max_chunk_samples: int) -> list[tuple]:
    """Extension (whisper_amd_long_plan, no device): [(first, count, packed samples)] for `segs` [(start cs, end cs)]."""
    s = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1)
    n = lib.whisper_amd_long_plan(s.ctypes.data_as(C.POINTER(C.c_int64)), len(s) // 2, n_samples, overlap, max_chunk_samples, None, None, None, 0)
    if n < 0:
        raise WhisperError("GenericError", int(n))
    first, count, packed = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64)
    lib.whisper_amd_long_plan(s.ctypes.data_as(C.POINTER(C.c_int64)), len(s) // 2, n_samples, overlap, max_chunk_samples,
                              first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_int32)),
                              packed.ctypes.data_as(C.POINTER(C.c_int64)), n)
    return [(int(first[i]), int(count[i]), int(packed[i])) for i in range(n)]


# ---------------------------------------------------------------------------------------------------
# live streaming sessions (whisper_amd_stream_*): sliding windows on a device ring
# ---------------------------------------------------------------------------------------------------
STREAM_BAD_ARGS, STREAM_FULL, STREAM_ENDED, STREAM_MIXED, STREAM_FAILED = -31, -32, -33, -34, -35    # WHISPER_AMD_STREAM_*
STREAM_INFO = ("windows", "start", "length", "take", "committed", "prompt_tokens", "dropped", "pending", "feeds_device", "feeds_host")


def stream_params(lib: C.CDLL, **kw) -> whisper_amd_stream_params:
    """`whisper_amd_stream_default_params()` with the given fields replaced."""
    p = whisper_amd_stream_params()
    lib.whisper_amd_stream_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class WhisperStream:
    """A live session (whisper_amd_stream_open): feed packets, step the windows that are due, read the results from `state`."""

    def __init__(self, ctx: WhisperContext, **kw):
        self.ctx, self.lib = ctx, ctx.lib
        self.params = stream_params(self.lib, **kw)
        self.ptr = self.lib.whisper_amd_stream_open(ctx.ptr, C.byref(self.params))
        if not self.ptr:
            raise WhisperError("StreamOpenRefused")
        self.state = WhisperState(ctx, self.lib.whisper_amd_stream_state(self.ptr))       # owned by the session: never free()d through this object

    def feed(self, data) -> int:
        """`data`: a numpy array of the session's format (interleaved where it has two channels), or a (device pointer, n_frames) tuple.
        Returns the windows now due or a negative STREAM_* code."""
        if isinstance(data, tuple):
            return self.lib.whisper_amd_stream_feed(self.ptr, C.c_void_p(data[0]), data[1])
        a = pcm_array(data, self.params.format)
        return self.lib.whisper_amd_stream_feed(self.ptr, C.c_void_p(a.ctypes.data), pcm_frames(a, self.params.channels, self.params.format))

    def flush(self) -> int:
        return self.lib.whisper_amd_stream_flush(self.ptr)

    def pending(self) -> int:
        return self.lib.whisper_amd_stream_pending(self.ptr)

    def step(self, params: FullParams) -> int:
        return self.lib.whisper_amd_stream_step(self.ptr, C.byref(params.c))

    def info(self) -> dict:
        out = (C.c_int64 * 10)()
        if self.lib.whisper_amd_stream_info(self.ptr, out) != 0:
            raise WhisperError("StreamInfo")
        return dict(zip(STREAM_INFO, [int(v) for v in out]))

    def window(self) -> np.ndarray:
        """The last window's PCM."""
        n = self.lib.whisper_amd_stream_window_copy(self.ptr, None, 0)
        if n < 0:
            raise WhisperError("StreamWindowCopy", int(n))
        out = np.zeros(max(n, 1), np.float32)
        if self.lib.whisper_amd_stream_window_copy(self.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n) != n:
            raise WhisperError("StreamWindowCopy")
        return out[:n]

    def prompt(self) -> list:
        """The prompt the last window ran with."""
        n = self.lib.whisper_amd_stream_prompt_copy(self.ptr, None, 0)
        out = (C.c_int32 * max(n, 1))()
        self.lib.whisper_amd_stream_prompt_copy(self.ptr, out, n)
        return list(out[:n])

    def segments(self) -> list:
        return self.state.segments()

    def reset(self):
        self.lib.whisper_amd_stream_reset(self.ptr)

    def close(self):
        if self.ptr:
            self.lib.whisper_amd_stream_close(self.ptr)
            self.ptr = None
            self.state.ptr = None


UTTERANCE_INFO = ("utterances", "start", "length", "start_cs", "end_cs", "split", "front_launches", "windows")


def stream_vad_params(lib: C.CDLL, vad=None, **kw) -> whisper_amd_stream_vad_params:
    """`whisper_amd_stream_vad_default_params()` with the given fields replaced; `vad`: a dict of whisper_vad_params fields."""
    p = whisper_amd_stream_vad_params()
    lib.whisper_amd_stream_vad_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    for k, v in (vad or {}).items():
        if not hasattr(p.vad, k):
            raise AttributeError(k)
        setattr(p.vad, k, v)
    return p


class WhisperVadStream(WhisperStream):
    """A live session that cuts at pauses (whisper_amd_stream_open_vad): feed packets, step the utterances that are due.  `vctx` is a
    WhisperVadContext the caller keeps alive; sessions share it."""

    def __init__(self, ctx: WhisperContext, vctx: "WhisperVadContext", vad=None, **kw):
        self.ctx, self.lib, self.vctx = ctx, ctx.lib, vctx
        self.params = stream_vad_params(self.lib, vad, **kw)
        self.ptr = self.lib.whisper_amd_stream_open_vad(ctx.ptr, vctx.ptr if vctx is not None else None, C.byref(self.params))
        if not self.ptr:
            raise WhisperError("StreamOpenRefused")
        self.state = WhisperState(ctx, self.lib.whisper_amd_stream_state(self.ptr))

    def utterance_info(self) -> dict:
        out = (C.c_int64 * 8)()
        if self.lib.whisper_amd_stream_utterance_info(self.ptr, out) != 0:
            raise WhisperError("StreamUtteranceInfo")
        return dict(zip(UTTERANCE_INFO, [int(v) for v in out]))

    def probs(self) -> np.ndarray:
        n = self.lib.whisper_amd_stream_vad_probs_copy(self.ptr, None, 0)
        if n < 0:
            raise WhisperError("StreamVadProbsCopy", int(n))
        out = np.zeros(max(n, 1), np.float32)
        self.lib.whisper_amd_stream_vad_probs_copy(self.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n)
        return out[:n]


def stream_vad_poll_many(streams: Sequence["WhisperVadStream"]) -> int:
    """Extension (whisper_amd_stream_vad_poll_many): the front end on the new windows of all sessions; the utterances due in total."""
    n = len(streams)
    sp = (C.c_void_p * max(n, 1))(*[s.ptr for s in streams])
    return streams[0].lib.whisper_amd_stream_vad_poll_many(sp, n)


def stream_step_many(streams: Sequence["WhisperStream"], params: FullParams) -> int:
    """Extension (whisper_amd_stream_step_many): one due window of every session that has one; the windows that ran or a negative code."""
    n = len(streams)
    sp = (C.c_void_p * max(n, 1))(*[s.ptr for s in streams])
    return streams[0].lib.whisper_amd_stream_step_many(sp, n, C.byref(params.c))


def batch_stats(ctx) -> tuple:
    """Extension (whisper_amd_batch_stats): lock-step passes of the context's last batch call and the rows they served."""
    a, b = C.c_long(0), C.c_long(0)
    ctx.lib.whisper_amd_batch_stats(ctx.ptr, C.byref(a), C.byref(b))
    return int(a.value), int(b.value)

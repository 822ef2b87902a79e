/*
 * whisper_amd.h - C ABI of the MI355X-native Whisper backend (libwhisper.so).
 *
 * This is the DROP-IN BOUNDARY: every entry point below has the same symbol name,
 * argument list, struct layout and return-code convention as the one whisper-rs binds through
 * bindgen over the reference's `sys/whisper.cpp/include/whisper.h` (cited per group as `ref:`),
 * so `whisper-rs-sys` can link this library instead of whisper.cpp + ggml without touching the
 * Rust sources.  Plain pointers and sizes only; no C++ / torch types.
 *
 * Layout facts verified by tests/test_abi.py against sizes measured on the reference header
 * (x86-64 SysV): whisper_context_params 48 B, whisper_full_params 296 B (`vad` at offset 260),
 * whisper_token_data 56 B.  Both params structs are passed BY VALUE, whisper_token_data and
 * whisper_full_params are also RETURNED by value (hidden sret pointer).
 *
 * Every function may be called with a null ctx/state only where the reference tolerates it.
 * No C++ exception crosses this boundary.
 */
#ifndef WHISPER_AMD_H
#define WHISPER_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#  define WHISPER_API __attribute__((visibility("default")))
#else
#  define WHISPER_API
#endif

/* ref: include/whisper.h:33-36 */
#define WHISPER_SAMPLE_RATE 16000
#define WHISPER_N_FFT       400
#define WHISPER_HOP_LENGTH  160
#define WHISPER_CHUNK_SIZE  30

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The three ggml items that leak into whisper.h and that whisper-rs binds
 * ref: ggml/include/ggml.h:550-557 (log levels), :614 (abort cb), :2105-2109 (log cb, ggml_log_set)
 *      ggml/include/ggml-cpu.h:80-85 (ggml_cpu_has_*), src/standalone.rs:150-170
 * ---------------------------------------------------------------------------------------------- */
enum ggml_log_level {
    GGML_LOG_LEVEL_NONE  = 0,
    GGML_LOG_LEVEL_DEBUG = 1,
    GGML_LOG_LEVEL_INFO  = 2,
    GGML_LOG_LEVEL_WARN  = 3,
    GGML_LOG_LEVEL_ERROR = 4,
    GGML_LOG_LEVEL_CONT  = 5,
};
typedef void (*ggml_log_callback)(enum ggml_log_level level, const char * text, void * user_data);
typedef bool (*ggml_abort_callback)(void * data);

WHISPER_API void ggml_log_set(ggml_log_callback log_callback, void * user_data);
WHISPER_API int  ggml_cpu_has_avx (void);
WHISPER_API int  ggml_cpu_has_avx2(void);
WHISPER_API int  ggml_cpu_has_fma (void);
WHISPER_API int  ggml_cpu_has_f16c(void);
/* ref: ggml/include/ggml-backend.h (ggml_backend_load_all): the reference's own examples call it before whisper_init_* (examples/bench/
 * bench.cpp:159, examples/cli); here there is one built-in backend and nothing to load - a no-op kept so that they link unmodified. */
WHISPER_API void ggml_backend_load_all(void);

/* ------------------------------------------------------------------------------------------------
 * Opaque handles and scalar typedefs            ref: include/whisper.h:80-86
 * ---------------------------------------------------------------------------------------------- */
struct whisper_context;      /* read-only model: weights resident in HBM, vocab, filters          */
struct whisper_state;        /* per-stream mutable state: mel, activations, KV caches, results    */
struct whisper_full_params;
struct whisper_vad_context;  /* Silero VAD: front end on the device, LSTM recurrence on the host ("VAD") */
struct whisper_vad_segments;

typedef int32_t whisper_pos;
typedef int32_t whisper_token;
typedef int32_t whisper_seq_id;

/* ref: include/whisper.h:88-104 - numeric order is ABI */
enum whisper_alignment_heads_preset {
    WHISPER_AHEADS_NONE,
    WHISPER_AHEADS_N_TOP_MOST,
    WHISPER_AHEADS_CUSTOM,
    WHISPER_AHEADS_TINY_EN,
    WHISPER_AHEADS_TINY,
    WHISPER_AHEADS_BASE_EN,
    WHISPER_AHEADS_BASE,
    WHISPER_AHEADS_SMALL_EN,
    WHISPER_AHEADS_SMALL,
    WHISPER_AHEADS_MEDIUM_EN,
    WHISPER_AHEADS_MEDIUM,
    WHISPER_AHEADS_LARGE_V1,
    WHISPER_AHEADS_LARGE_V2,
    WHISPER_AHEADS_LARGE_V3,
    WHISPER_AHEADS_LARGE_V3_TURBO,
};

/* ref: include/whisper.h:106-114 */
typedef struct whisper_ahead  { int n_text_layer; int n_head; } whisper_ahead;
typedef struct whisper_aheads { size_t n_heads; const whisper_ahead * heads; } whisper_aheads;

/* ref: include/whisper.h:116-129 (48 bytes).  `use_gpu=false` is rejected by this backend: there
 * is no CPU path in the product (init returns NULL with an error log). `gpu_device` = HIP device. */
struct whisper_context_params {
    bool  use_gpu;
    bool  flash_attn;            /* false (default): reference summation order, bit-identical to whisper.cpp CPU; true: F16-MFMA encoder / prompt
                                    products (tolerance-level parity) and, as in the reference, DTW off (whisper.cpp:3724-3727) */
    int   gpu_device;
    bool  dtw_token_timestamps;
    enum whisper_alignment_heads_preset dtw_aheads_preset;
    int   dtw_n_top;
    struct whisper_aheads dtw_aheads;
    size_t dtw_mem_size;
};

/* ref: include/whisper.h:131-151 (56 bytes) */
typedef struct whisper_token_data {
    whisper_token id;
    whisper_token tid;
    float   p;
    float   plog;
    float   pt;
    float   ptsum;
    int64_t t0;
    int64_t t1;
    int64_t t_dtw;
    float   vlen;
} whisper_token_data;

/* ref: include/whisper.h:153-159 */
typedef struct whisper_model_loader {
    void * context;
    size_t (*read)(void * ctx, void * output, size_t read_size);
    bool   (*eof)(void * ctx);
    void   (*close)(void * ctx);
} whisper_model_loader;

/* ref: include/whisper.h:162-190 (grammar-constrained sampling: whisper_full_params::grammar_rules is an array of
 * n_grammar_rules pointers, one END-terminated element array per rule; a malformed grammar makes whisper_full return -20) */
enum whisper_gretype {
    WHISPER_GRETYPE_END            = 0,
    WHISPER_GRETYPE_ALT            = 1,
    WHISPER_GRETYPE_RULE_REF       = 2,
    WHISPER_GRETYPE_CHAR           = 3,
    WHISPER_GRETYPE_CHAR_NOT       = 4,
    WHISPER_GRETYPE_CHAR_RNG_UPPER = 5,
    WHISPER_GRETYPE_CHAR_ALT       = 6,
};
typedef struct whisper_grammar_element { enum whisper_gretype type; uint32_t value; } whisper_grammar_element;

/* ref: include/whisper.h:192-199 */
typedef struct whisper_vad_params {
    float threshold;
    int   min_speech_duration_ms;
    int   min_silence_duration_ms;
    float max_speech_duration_s;
    int   speech_pad_ms;
    float samples_overlap;
} whisper_vad_params;

/* ref: include/whisper.h:453-456 */
enum whisper_sampling_strategy { WHISPER_SAMPLING_GREEDY, WHISPER_SAMPLING_BEAM_SEARCH };

/* ref: include/whisper.h:458-480 - callbacks run on the thread that called whisper_full* */
typedef void (*whisper_new_segment_callback)(struct whisper_context * ctx, struct whisper_state * state, int n_new, void * user_data);
typedef void (*whisper_progress_callback)(struct whisper_context * ctx, struct whisper_state * state, int progress, void * user_data);
typedef bool (*whisper_encoder_begin_callback)(struct whisper_context * ctx, struct whisper_state * state, void * user_data);
typedef void (*whisper_logits_filter_callback)(struct whisper_context * ctx, struct whisper_state * state,
                                               const whisper_token_data * tokens, int n_tokens, float * logits, void * user_data);

/* ref: include/whisper.h:485-588 (296 bytes; field order is ABI) */
struct whisper_full_params {
    enum whisper_sampling_strategy strategy;

    int n_threads;               /* advisory on this backend */
    int n_max_text_ctx;
    int offset_ms;
    int duration_ms;

    bool translate;
    bool no_context;
    bool no_timestamps;
    bool single_segment;
    bool print_special;
    bool print_progress;
    bool print_realtime;
    bool print_timestamps;

    bool  token_timestamps;      /* heuristic per-token t0 / t1 / vlen (whisper.cpp:8326-8616), with max_len / split_on_word wrapping */
    float thold_pt;
    float thold_ptsum;
    int   max_len;
    bool  split_on_word;
    int   max_tokens;

    bool debug_mode;
    int  audio_ctx;

    bool tdrz_enable;

    const char * suppress_regex;

    const char * initial_prompt;
    const whisper_token * prompt_tokens;
    int prompt_n_tokens;

    const char * language;
    bool detect_language;

    bool suppress_blank;
    bool suppress_nst;

    float temperature;
    float max_initial_ts;
    float length_penalty;

    float temperature_inc;
    float entropy_thold;
    float logprob_thold;
    float no_speech_thold;

    struct { int best_of; } greedy;
    struct { int beam_size; float patience; } beam_search;

    whisper_new_segment_callback new_segment_callback;
    void * new_segment_callback_user_data;
    whisper_progress_callback progress_callback;
    void * progress_callback_user_data;
    whisper_encoder_begin_callback encoder_begin_callback;
    void * encoder_begin_callback_user_data;
    ggml_abort_callback abort_callback;
    void * abort_callback_user_data;
    whisper_logits_filter_callback logits_filter_callback;
    void * logits_filter_callback_user_data;

    const whisper_grammar_element ** grammar_rules;
    size_t n_grammar_rules;
    size_t i_start_rule;
    float  grammar_penalty;

    bool         vad;
    const char * vad_model_path;
    whisper_vad_params vad_params;
};

/* ref: include/whisper.h:436-442 */
struct whisper_timings { float sample_ms, encode_ms, decode_ms, batchd_ms, prompt_ms; };

/* ref: include/whisper.h:679-683 */
struct whisper_vad_context_params { int n_threads; bool use_gpu; int gpu_device; };

/* ------------------------------------------------------------------------------------------------
 * Model load / state / free
 * ref: include/whisper.h:204-239, 266-269; engine whisper.cpp:3640-3889.  NULL on failure.
 * whisper-rs calls only the *_no_state constructors + whisper_init_state
 * (src/whisper_ctx.rs:33,60; src/whisper_ctx_wrapper.rs:446).
 * ---------------------------------------------------------------------------------------------- */
WHISPER_API struct whisper_context * whisper_init_from_file_with_params  (const char * path_model, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_from_buffer_with_params(void * buffer, size_t buffer_size, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_with_params            (struct whisper_model_loader * loader, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_from_file_with_params_no_state  (const char * path_model, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_from_buffer_with_params_no_state(void * buffer, size_t buffer_size, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_with_params_no_state            (struct whisper_model_loader * loader, struct whisper_context_params params);
WHISPER_API struct whisper_context * whisper_init_from_file           (const char * path_model);
WHISPER_API struct whisper_context * whisper_init_from_buffer         (void * buffer, size_t buffer_size);
WHISPER_API struct whisper_context * whisper_init                     (struct whisper_model_loader * loader);
WHISPER_API struct whisper_context * whisper_init_from_file_no_state  (const char * path_model);
WHISPER_API struct whisper_context * whisper_init_from_buffer_no_state(void * buffer, size_t buffer_size);
WHISPER_API struct whisper_context * whisper_init_no_state            (struct whisper_model_loader * loader);

WHISPER_API struct whisper_state * whisper_init_state(struct whisper_context * ctx);

WHISPER_API void whisper_free               (struct whisper_context * ctx);
WHISPER_API void whisper_free_state         (struct whisper_state * state);
WHISPER_API void whisper_free_params        (struct whisper_full_params * params);
WHISPER_API void whisper_free_context_params(struct whisper_context_params * params);

/* ref: include/whisper.h:252-263 - OpenVINO is another vendor's runtime: always returns 1 ("not enabled") */
WHISPER_API int whisper_ctx_init_openvino_encoder_with_state(struct whisper_context * ctx, struct whisper_state * state,
                                                             const char * model_path, const char * device, const char * cache_dir);
WHISPER_API int whisper_ctx_init_openvino_encoder(struct whisper_context * ctx, const char * model_path,
                                                  const char * device, const char * cache_dir);

/* ------------------------------------------------------------------------------------------------
 * Stage API: PCM -> log-mel -> encoder (+cross K/V) -> decoder logits
 * ref: include/whisper.h:274-338, 413-414; engine whisper.cpp:3891-3971.
 * `samples` may be a host pointer or a HIP device pointer (detected with hipPointerGetAttributes).
 * Returns: pcm_to_mel/encode 0 | -1; set_mel 0 | -1 (n_mel mismatch); decode 0 | 1.
 * whisper_get_logits*: row n_tokens-1 of the last decode call is valid (whisper.cpp:2965-2971).
 * ---------------------------------------------------------------------------------------------- */
WHISPER_API int whisper_pcm_to_mel           (struct whisper_context * ctx, const float * samples, int n_samples, int n_threads);
WHISPER_API int whisper_pcm_to_mel_with_state(struct whisper_context * ctx, struct whisper_state * state, const float * samples, int n_samples, int n_threads);
WHISPER_API int whisper_set_mel              (struct whisper_context * ctx, const float * data, int n_len, int n_mel);
WHISPER_API int whisper_set_mel_with_state   (struct whisper_context * ctx, struct whisper_state * state, const float * data, int n_len, int n_mel);
WHISPER_API int whisper_encode               (struct whisper_context * ctx, int offset, int n_threads);
WHISPER_API int whisper_encode_with_state    (struct whisper_context * ctx, struct whisper_state * state, int offset, int n_threads);
WHISPER_API int whisper_decode               (struct whisper_context * ctx, const whisper_token * tokens, int n_tokens, int n_past, int n_threads);
WHISPER_API int whisper_decode_with_state    (struct whisper_context * ctx, struct whisper_state * state, const whisper_token * tokens, int n_tokens, int n_past, int n_threads);
WHISPER_API float * whisper_get_logits           (struct whisper_context * ctx);
WHISPER_API float * whisper_get_logits_from_state(struct whisper_state * state);

/* ------------------------------------------------------------------------------------------------
 * Tokenizer / languages                        ref: include/whisper.h:345-387; whisper.cpp:3973-4110
 * tokenize: count, or -(needed) when n_max_tokens is too small.
 * lang_auto_detect: id >= 0, or -1 (offset<0), -2 (offset past end), -6 (encode), -7 (decode).
 * ---------------------------------------------------------------------------------------------- */
WHISPER_API int whisper_tokenize   (struct whisper_context * ctx, const char * text, whisper_token * tokens, int n_max_tokens);
WHISPER_API int whisper_token_count(struct whisper_context * ctx, const char * text);
WHISPER_API int          whisper_lang_max_id  (void);
WHISPER_API int          whisper_lang_id      (const char * lang);
WHISPER_API const char * whisper_lang_str     (int id);
WHISPER_API const char * whisper_lang_str_full(int id);
WHISPER_API int whisper_lang_auto_detect           (struct whisper_context * ctx, int offset_ms, int n_threads, float * lang_probs);
WHISPER_API int whisper_lang_auto_detect_with_state(struct whisper_context * ctx, struct whisper_state * state, int offset_ms, int n_threads, float * lang_probs);

/* ------------------------------------------------------------------------------------------------
 * Model / vocabulary introspection              ref: include/whisper.h:389-433; whisper.cpp:4120-4259
 * ---------------------------------------------------------------------------------------------- */
WHISPER_API int whisper_n_len           (struct whisper_context * ctx);
WHISPER_API int whisper_n_len_from_state(struct whisper_state * state);   /* = n_len_org (whisper.cpp:4185-4187) */
WHISPER_API int whisper_n_vocab         (struct whisper_context * ctx);
WHISPER_API int whisper_n_text_ctx      (struct whisper_context * ctx);
WHISPER_API int whisper_n_audio_ctx     (struct whisper_context * ctx);
WHISPER_API int whisper_is_multilingual (struct whisper_context * ctx);

WHISPER_API int whisper_model_n_vocab      (struct whisper_context * ctx);
WHISPER_API int whisper_model_n_audio_ctx  (struct whisper_context * ctx);
WHISPER_API int whisper_model_n_audio_state(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_audio_head (struct whisper_context * ctx);
WHISPER_API int whisper_model_n_audio_layer(struct whisper_context * ctx);
WHISPER_API int whisper_model_n_text_ctx   (struct whisper_context * ctx);
WHISPER_API int whisper_model_n_text_state (struct whisper_context * ctx);
WHISPER_API int whisper_model_n_text_head  (struct whisper_context * ctx);
WHISPER_API int whisper_model_n_text_layer (struct whisper_context * ctx);
WHISPER_API int whisper_model_n_mels       (struct whisper_context * ctx);
WHISPER_API int whisper_model_ftype        (struct whisper_context * ctx);   /* loadable: 1 F16, 7 Q8_0, 8 Q5_0, 9 Q5_1, 3 Q4_1, 10 Q2_K, 11 Q3_K, 13 Q5_K, 14 Q6_K */
WHISPER_API int whisper_model_type         (struct whisper_context * ctx);
WHISPER_API const char * whisper_model_type_readable(struct whisper_context * ctx);

WHISPER_API const char * whisper_token_to_str(struct whisper_context * ctx, whisper_token token);
WHISPER_API whisper_token whisper_token_eot (struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_sot (struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_solm(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_prev(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_nosp(struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_not (struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_beg (struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_lang(struct whisper_context * ctx, int lang_id);
WHISPER_API whisper_token whisper_token_translate (struct whisper_context * ctx);
WHISPER_API whisper_token whisper_token_transcribe(struct whisper_context * ctx);

/* ------------------------------------------------------------------------------------------------
 * Timings / system info / logging       ref: include/whisper.h:443-448, 729; whisper.cpp:4261-4355
 * ---------------------------------------------------------------------------------------------- */
WHISPER_API struct whisper_timings * whisper_get_timings(struct whisper_context * ctx);
WHISPER_API void whisper_print_timings(struct whisper_context * ctx);
WHISPER_API void whisper_reset_timings(struct whisper_context * ctx);
WHISPER_API const char * whisper_print_system_info(void);
WHISPER_API void whisper_log_set(ggml_log_callback log_callback, void * user_data);

/* ------------------------------------------------------------------------------------------------
 * Full pipeline                                ref: include/whisper.h:591-623; whisper.cpp:5898-6019,
 *                                                   6795-7864
 * whisper_full_with_state: 0 ok; -2 mel; -3 language detect; -4 too many decoders; -5 audio_ctx;
 * -6 encode; -7 KV realloc; -8 / -9 decode   (same codes as whisper.cpp:6810-7433).
 * ---------------------------------------------------------------------------------------------- */
WHISPER_API struct whisper_context_params * whisper_context_default_params_by_ref(void);
WHISPER_API struct whisper_context_params   whisper_context_default_params       (void);
WHISPER_API struct whisper_full_params * whisper_full_default_params_by_ref(enum whisper_sampling_strategy strategy);
WHISPER_API struct whisper_full_params   whisper_full_default_params       (enum whisper_sampling_strategy strategy);

WHISPER_API int whisper_full           (struct whisper_context * ctx, struct whisper_full_params params, const float * samples, int n_samples);
WHISPER_API int whisper_full_with_state(struct whisper_context * ctx, struct whisper_state * state, struct whisper_full_params params, const float * samples, int n_samples);
WHISPER_API int whisper_full_parallel  (struct whisper_context * ctx, struct whisper_full_params params, const float * samples, int n_samples, int n_processors);

/* ------------------------------------------------------------------------------------------------
 * Result getters (valid until the next whisper_full* on the same state; readable from inside
 * new_segment_callback)                         ref: include/whisper.h:627-669, 732-733; whisper.cpp:7866-8033
 * ---------------------------------------------------------------------------------------------- */
WHISPER_API int     whisper_full_n_segments           (struct whisper_context * ctx);
WHISPER_API int     whisper_full_n_segments_from_state(struct whisper_state * state);
WHISPER_API int     whisper_full_lang_id              (struct whisper_context * ctx);
WHISPER_API int     whisper_full_lang_id_from_state   (struct whisper_state * state);
WHISPER_API int64_t whisper_full_get_segment_t0           (struct whisper_context * ctx, int i_segment);
WHISPER_API int64_t whisper_full_get_segment_t0_from_state(struct whisper_state * state, int i_segment);
WHISPER_API int64_t whisper_full_get_segment_t1           (struct whisper_context * ctx, int i_segment);
WHISPER_API int64_t whisper_full_get_segment_t1_from_state(struct whisper_state * state, int i_segment);
WHISPER_API bool    whisper_full_get_segment_speaker_turn_next           (struct whisper_context * ctx, int i_segment);
WHISPER_API bool    whisper_full_get_segment_speaker_turn_next_from_state(struct whisper_state * state, int i_segment);
WHISPER_API const char * whisper_full_get_segment_text           (struct whisper_context * ctx, int i_segment);
WHISPER_API const char * whisper_full_get_segment_text_from_state(struct whisper_state * state, int i_segment);
WHISPER_API int     whisper_full_n_tokens           (struct whisper_context * ctx, int i_segment);
WHISPER_API int     whisper_full_n_tokens_from_state(struct whisper_state * state, int i_segment);
WHISPER_API const char * whisper_full_get_token_text           (struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API const char * whisper_full_get_token_text_from_state(struct whisper_context * ctx, struct whisper_state * state, int i_segment, int i_token);
WHISPER_API whisper_token whisper_full_get_token_id           (struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API whisper_token whisper_full_get_token_id_from_state(struct whisper_state * state, int i_segment, int i_token);
WHISPER_API whisper_token_data whisper_full_get_token_data           (struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API whisper_token_data whisper_full_get_token_data_from_state(struct whisper_state * state, int i_segment, int i_token);
WHISPER_API float   whisper_full_get_token_p           (struct whisper_context * ctx, int i_segment, int i_token);
WHISPER_API float   whisper_full_get_token_p_from_state(struct whisper_state * state, int i_segment, int i_token);
WHISPER_API float   whisper_full_get_segment_no_speech_prob           (struct whisper_context * ctx, int i_segment);
WHISPER_API float   whisper_full_get_segment_no_speech_prob_from_state(struct whisper_state * state, int i_segment);

/* ------------------------------------------------------------------------------------------------
 * VAD (ref: include/whisper.h:677-725): probabilities, segments and whisper_full's `vad = true` are
 * bit-identical to the reference's CPU VAD.  One model shape is supported (the Silero 16 kHz model the
 * reference's graph hard-codes); anything else is refused at load time with a message naming it.
 * whisper_vad_context_params.use_gpu is not looked at (its default is false and there is no CPU path):
 * the context always runs on `gpu_device`; a context that whisper_full creates from `vad_model_path`
 * runs on the whisper context's device.  `n_threads` is accepted and unused.
 * The bench helpers below remain link-completeness stubs.
 * ---------------------------------------------------------------------------------------------- */
WHISPER_API struct whisper_vad_params         whisper_vad_default_params(void);
WHISPER_API struct whisper_vad_context_params whisper_vad_default_context_params(void);
WHISPER_API struct whisper_vad_context * whisper_vad_init_from_file_with_params(const char * path_model, struct whisper_vad_context_params params);
WHISPER_API struct whisper_vad_context * whisper_vad_init_with_params          (struct whisper_model_loader * loader, struct whisper_vad_context_params params);
WHISPER_API bool    whisper_vad_detect_speech(struct whisper_vad_context * vctx, const float * samples, int n_samples);
WHISPER_API int     whisper_vad_n_probs(struct whisper_vad_context * vctx);
WHISPER_API float * whisper_vad_probs  (struct whisper_vad_context * vctx);
WHISPER_API struct whisper_vad_segments * whisper_vad_segments_from_probs  (struct whisper_vad_context * vctx, struct whisper_vad_params params);
WHISPER_API struct whisper_vad_segments * whisper_vad_segments_from_samples(struct whisper_vad_context * vctx, struct whisper_vad_params params, const float * samples, int n_samples);
WHISPER_API int   whisper_vad_segments_n_segments(struct whisper_vad_segments * segments);
WHISPER_API float whisper_vad_segments_get_segment_t0(struct whisper_vad_segments * segments, int i_segment);
WHISPER_API float whisper_vad_segments_get_segment_t1(struct whisper_vad_segments * segments, int i_segment);
WHISPER_API void  whisper_vad_free_segments(struct whisper_vad_segments * segments);
WHISPER_API void  whisper_vad_free         (struct whisper_vad_context  * ctx);

WHISPER_API int          whisper_bench_memcpy          (int n_threads);
WHISPER_API const char * whisper_bench_memcpy_str      (int n_threads);
WHISPER_API int          whisper_bench_ggml_mul_mat    (int n_threads);
WHISPER_API const char * whisper_bench_ggml_mul_mat_str(int n_threads);

/* ================================================================================================
 * Extensions of this backend (not in the reference header; prefix whisper_amd_).
 * They exist for tests, the bench and multi-GPU chunk sharding; whisper-rs never needs them.
 * ============================================================================================== */

/* sizeof/offsetof self-description so a binding can verify its struct layout at run time:
 * out[0]=sizeof(context_params) out[1]=sizeof(full_params) out[2]=sizeof(token_data)
 * out[3]=offsetof(full_params, vad) out[4]=offsetof(full_params, greedy) out[5]=offsetof(full_params, language) */
WHISPER_API void whisper_amd_abi_sizes(size_t out[6]);

/* Device-resident intermediates for parity tests.  Each copies up to `cap` elements into `dst`
 * (host) and returns the full element count (call with cap=0 to size).  -1 when not available.
 *   mel:      [n_mel][n_len] f32 as produced by whisper_pcm_to_mel*  (whisper.cpp:3186-3276)
 *   embd_enc: [n_audio_ctx][n_state] f32 encoder output              (whisper.cpp:2056-2287)
 *   embd_conv:[n_audio_ctx][n_state] f32 conv-stem output (+GELU), BEFORE the positional add */
WHISPER_API int64_t whisper_amd_get_mel      (struct whisper_state * state, float * dst, int64_t cap, int * n_len, int * n_mel);
WHISPER_API int64_t whisper_amd_get_embd_enc (struct whisper_state * state, float * dst, int64_t cap);
WHISPER_API int64_t whisper_amd_get_embd_conv(struct whisper_state * state, float * dst, int64_t cap);

/* VAD front end alone (k_vad_front): the [n_chunks][512] F32 LSTM gate inputs W_ih x + b_ih of every 512-sample window of
 * `samples` (the last one zero-filled), gate order i, f, g, o.  Copies up to `cap` elements, returns the full count, -1 on failure.
 * whisper_amd_vad_tile: windows per workgroup of that kernel (tests put chunk counts on either side of it).
 * whisper_amd_vad_timings: out = { whisper_vad_detect_speech wall time, of it waiting for the device, of it host recurrence } in us. */
WHISPER_API int64_t whisper_amd_vad_front  (struct whisper_vad_context * vctx, const float * samples, int n_samples, float * dst, int64_t cap);
WHISPER_API int     whisper_amd_vad_tile   (void);
WHISPER_API void    whisper_amd_vad_timings(struct whisper_vad_context * vctx, int64_t out_us[3]);

/* Per-state stage timers in microseconds + call counts (the reference keeps them per state but
 * only prints ctx->state's, whisper.cpp:868-881,4274-4296):
 * out = { t_sample, t_encode, t_decode, t_batchd, t_prompt, t_mel, n_sample, n_encode, n_decode,
 *         n_batchd, n_prompt, n_fail_p + n_fail_h } */
WHISPER_API void whisper_amd_get_timings_us(struct whisper_state * state, int64_t out[12]);
WHISPER_API void whisper_amd_reset_timings (struct whisper_state * state);

/* The F16 GELU table the device kernels use (65536 entries; vec.h:571-585 semantics). */
WHISPER_API void whisper_amd_gelu_table_f16(uint16_t * dst);

/* HIP stream (hipStream_t as void*) every kernel of this state is launched on - for external
 * event timing (bench.py) and stream-ordered hand-off of device PCM buffers. */
WHISPER_API void * whisper_amd_state_stream(struct whisper_state * state);

/* Decode-loop bookkeeping of decoder `j` after whisper_full* (for tests: compares the loop's internal decisions with
 * the reference even when no segment was emitted): out = { failed, completed, has_ts, seek_delta, result_len,
 * avg_logprobs, entropy, no_speech_prob }; ids receives up to max_ids token ids; returns the token count. */
WHISPER_API int whisper_amd_decoder_info(struct whisper_state * state, int j, double out[8], int32_t * ids, int max_ids);

/* Measurement helper (bench.py): replays the single-token decoder pass `n_iters` times back to back on the
 * state's stream between two HIP events and returns the average DEVICE time of one decode step in ms.
 * Needs a prior whisper_encode*; touches KV cell `n_past` of the state.  0 on success. */
WHISPER_API int whisper_amd_decode_step_probe(struct whisper_context * ctx, struct whisper_state * state, int n_past, int n_iters, float * ms_per_step);

/* 1 when the state runs the single-token decoder pass as ONE persistent launch (wa_mega.hip), 0 when it replays the
 * captured launch sequence (WHISPER_AMD_NO_MEGA=1, unsupported shape, after a hand-off time-out, or a model whose weight format has no
 * one-launch kernel: Q5_1 / Q4_1 and Q2_K / Q3_K / Q5_K / Q6_K files run the launch sequence in every decode mode, and whisper_amd_rows_enabled is 0 too). */
WHISPER_API int whisper_amd_mega_enabled(struct whisper_state * state);
/* Role of workgroup `wg` of the n_wg workgroups of the one-launch step for a model with n_head text heads (no device needed): role 0 =
 * weight streaming (index = its rank), 1 = self-attention of head `index`, 2 = cross-attention (index = 4 head + quarter). */
WHISPER_API void whisper_amd_mega_role_of(int n_wg, int n_head, int wg, int * role, int * index);

/* Host-overlapped greedy decoding (the device decodes its own prediction of the next token while the host applies the
 * reference's sampling rules to the previous logits): out = { predictions confirmed, predictions wrong (step redone) }
 * since the last whisper_amd_reset_timings. */
WHISPER_API void whisper_amd_overlap_stats(struct whisper_state * state, int out[2]);

/* Debugging aid (tools/mega_check.py): runs the one-launch step for (token, position n_past) on KV cell n_past and copies
 * out the hand-off granules [n_text_layer][8][2 * n_text_state] (tag << 32 | value bits) and the logits [n_vocab].
 * Returns the step's status word (0 = ok), < 0 when the one-launch step is not available. */
WHISPER_API int whisper_amd_mega_debug(struct whisper_context * ctx, struct whisper_state * state, int token, int n_past,
                                       unsigned long long * granules_out, float * logits_out);
/* The same step through the launch sequence, stage by stage: values only, in the granule layout above (32-bit words). */
WHISPER_API int whisper_amd_seq_debug(struct whisper_context * ctx, struct whisper_state * state, int token, int n_past, unsigned * values_out,
                                      float * logits_out);

/* The decode step for 2..8 token rows as ONE launch (wa_rows.hip: beam / best_of steps, small batches, lock-step chunks):
 * out = { passes served by it, passes sent to the launch sequence after a status word } since the state was created. */
WHISPER_API void whisper_amd_rows_stats(struct whisper_state * state, long out[2]);
WHISPER_API int  whisper_amd_rows_enabled(struct whisper_state * state);
/* Quantised models (Q5_0 / Q8_0 / Q4_1 / Q5_1 and the K formats Q2_K / Q3_K / Q5_K / Q6_K): the products with more than 8 activation rows - the
 * encoder, the cross K/V product, prompt passes, DTW's extra pass - that this state launched since it was created: out = { served by the int8
 * matrix-core kernel (k_qgemm_mfma; K formats: k_kgemm_mfma), served by k_qgemm_exact (K formats: k_kgemm_exact) }.  WHISPER_AMD_NO_QMFMA=1 in
 * the environment sends all of them to the second. */
WHISPER_API void whisper_amd_qgemm_stats(struct whisper_state * state, long out[2]);
/* Quantised models: the products of 2..8 activation rows - beam-search and best_of steps, small whisper_decode batches - that this state issued (or
 * captured into a graph: passes are captured once and replayed, so these count captures, not replays) since it was created: out = { taken by a
 * few-rows kernel (k_qgemv_rows; K formats: k_kgemv_rows), taken by the general kernel (k_qgemm_exact; K formats: k_kgemm_exact) }.
 * WHISPER_AMD_NO_FEW_ROWS=1 in the environment sends all of them to the second. */
WHISPER_API void whisper_amd_few_rows_stats(struct whisper_state * state, long out[2]);
/* Debugging aid (tools/rows_check.py): B identical rows (token, position n_past) of this state through the several-rows step; copies out the
 * hand-off granules [n_text_layer][8][B][2 * n_text_state] and the logits [B][n_vocab].  Returns the status word (0 = ok), < 0: not available. */
WHISPER_API int whisper_amd_rows_debug(struct whisper_context * ctx, struct whisper_state * state, int B, int token, int n_past,
                                       unsigned long long * granules_out, float * logits_out);
/* Measurement helper (bench.py): average DEVICE time of one B-row step, row i on states[i]'s cells and encoder K / V (null = states[0]). */
WHISPER_API int whisper_amd_rows_step_probe(struct whisper_context * ctx, struct whisper_state ** states, int B, int n_past, int n_iters, float * ms_per_step);
/* Test entries (tests/test_rows_kernel_gpu.py): they hand the decoder the batches whisper_full builds and do the cell operations it does between them.
 * None of them is on a decode path.
 * whisper_amd_decode_batch: one decoder pass over n_tokens rows, each with its token, position, sequence id and logits flag, exactly as whisper_full
 *   issues it; unlike whisper_decode_with_state it removes no cell first.  0 on success; row i's logits then stand at
 *   whisper_get_logits_from_state(state) + i * n_vocab for every flagged i.
 * whisper_amd_kv_op: the bookkeeping of the self-attention cells.  op 0: forget every cell; 1: remove sequence a from the cells at positions [p0, p1)
 *   (a < 0: every sequence; p0 / p1 < 0: open end); 2: add sequence b to the cells of sequence a at positions [p0, p1); 3: a new, empty cache of `a`
 *   cells, as whisper_full makes one for several decoders (at most 5120 cells; the state then counts as prepared for as many decoders as whisper_full's
 *   rule, 512 cells x (decoders + 2), fits into `a`); 4, 5, 6: return the cells in use (n), the cell the next batch is tried at (head), the cache's
 *   size.  -1: bad arguments or a failed allocation.
 * whisper_amd_rows_fits: 1 where the several-rows one-launch step takes B rows of this model on this device, else 0.
 * whisper_amd_rows_debug_rows: whisper_amd_rows_debug with a state, a token and a context length per row - row i attends over cells [0, n_past[i]] of
 *   states[i] and that state's encoder K / V, and writes cell n_past[i] with the values a decode would write; the cell bookkeeping is left alone.  The
 *   states are distinct and agree in cache size and audio context (-2 otherwise).  logits_out [B][n_vocab]; row_status_out [B]: 0, or 9000 for a row
 *   that the launch sequence would redo.  Returns as whisper_amd_rows_debug. */
WHISPER_API int whisper_amd_decode_batch(struct whisper_context * ctx, struct whisper_state * state, const whisper_token * tokens, const int32_t * pos,
                                         const int32_t * seq_id, const int8_t * logits, int n_tokens);
WHISPER_API int whisper_amd_kv_op(struct whisper_state * state, int op, int a, int b, int p0, int p1);
WHISPER_API int whisper_amd_rows_fits(struct whisper_context * ctx, int B);
WHISPER_API int whisper_amd_rows_debug_rows(struct whisper_context * ctx, struct whisper_state ** states, int B, const int * tokens, const int * n_past,
                                            float * logits_out, unsigned * row_status_out);

/* Chunk-parallel transcription on ONE device (the reference's model: one state + thread per chunk, whisper.cpp:7771-7806):
 * runs `n_chunks` independent whisper_full_with_state jobs, each on its own state / HIP stream / host thread; mel, encoder and
 * prompts overlap on the device, and the single-token decode steps of the chunks are served in LOCK STEP - one decoder pass reads
 * every weight row once for all chunks' tokens (up to 8 rows per pass; F16 models, and Q5_0 / Q8_0 models where the several-rows one-launch
 * step of wa_rows.hip takes the shape - the members of any other group decode their tokens alone).
 * Results are those of each chunk alone.
 * samples[i] may be host or device pointers.  Returns 0 or the first non-zero per-chunk code. */
WHISPER_API int whisper_amd_full_batch(struct whisper_context * ctx, struct whisper_state ** states, int n_chunks,
                                       struct whisper_full_params params, const float * const * samples, const int * n_samples);
/* how the last whisper_amd_full_batch or whisper_full_parallel call on this context decoded: lock-step passes and the token rows they served */
WHISPER_API void whisper_amd_batch_stats(struct whisper_context * ctx, long * steps, long * rows);
/* ... and how many of those passes were ONE launch (wa_rows.hip) rather than the launch sequence */
WHISPER_API long whisper_amd_batch_one_launch(struct whisper_context * ctx);
/* ... and how many of them DELIVERED their rows to the members, as one launch or through the launch sequence (`steps` counts every pass the
 * group formed; the passes not counted here ended with each member decoding its token alone) */
WHISPER_API long whisper_amd_batch_served(struct whisper_context * ctx);

/* DTW token timestamps, the alignment alone (wa_dtw.cpp): normalise over tokens, median over audio with reflect padding, mean over heads,
 * DTW table and backtrace over a caller's own cross-attention probabilities - what whisper_full does after its extra decoder pass when
 * dtw_token_timestamps is set.  qk is a host cube [n_heads][n_tokens][n_ctx] F32 of which the first n_audio_tokens frames are used; rows
 * [sot_len, n_tokens - 1) enter the table (N = n_tokens - sot_len - 1 rows, M = n_audio_tokens columns).
 * where = 0: the host function.  where = 1: the device kernels (wa_dtw.hip); the cube is uploaded into the state's capture buffer and runs
 * through the launchers of the product path, on the state's stream.  Both give the same path, pair for pair.
 * Returns the path length (at most N + M) and copies up to `cap` pairs (token index, time index; one time index = 20 ms), or
 *   WHISPER_AMD_DTW_REFUSED    the arguments are refused by both paths: an even or non-positive medfilt_width, M <= medfilt_width, M > n_ctx,
 *                              N <= 0, no heads, null pointers, another `where`;
 *   WHISPER_AMD_DTW_NOT_TAKEN  where = 1 and the device path does not take them: it serves medfilt_width 7 and n_tokens up to the state's
 *                              decoder rows (the text context rounded up to 64);
 *   WHISPER_AMD_DTW_HIP_ERROR  a HIP call failed.
 * Nothing is written on a negative return.
 * whisper_amd_dtw_stats: out = { DTW calls served by the device path, calls served by the host path, device-path attempts that fell back to
 * the host path } since the state was created, whisper_full's calls and whisper_amd_dtw_path's alike.  WHISPER_AMD_DTW_HOST=1 in the environment
 * when a state is created makes whisper_full take the host path on that state.
 * whisper_amd_dtw_timings: out = { wall time in us of whisper_full's DTW post-processing on this state, from the end of the decoder pass to
 * t_dtw placed, number of such calls } (tools/dtw_probe.py). */
#define WHISPER_AMD_DTW_REFUSED   (-1)
#define WHISPER_AMD_DTW_NOT_TAKEN (-2)
#define WHISPER_AMD_DTW_HIP_ERROR (-3)
WHISPER_API int  whisper_amd_dtw_path(struct whisper_state * state, const float * qk, int n_heads, int n_tokens, int n_ctx, int n_audio_tokens,
                                      int sot_len, int medfilt_width, int where, int32_t * path_tok, int32_t * path_time, int cap);
WHISPER_API void whisper_amd_dtw_stats(struct whisper_state * state, long out[3]);
WHISPER_API void whisper_amd_dtw_timings(struct whisper_state * state, int64_t out[2]);

/* Model load (wa_loader.cpp).  By default the tensor bytes go to the device in pinned chunks while the next chunk is being read, and
 * HIP kernels (wa_load.hip) write the kernel layouts straight into the weight arena; WHISPER_AMD_LOAD_HOST=1 in the environment WHEN A CONTEXT IS
 * CREATED takes the host path instead (a host image of the arena, unpacked on the host, one upload).  Both leave the same arena, byte for byte.
 * whisper_amd_arena_read: copies up to `cap` bytes of the weight arena from byte `offset` into `dst` (host) and returns the arena's size in bytes
 *   (call with cap = 0 to size the buffer); -1 without a loaded model or when the copy fails.
 * whisper_amd_load_stats: out = { path taken (0 host, 1 device), tensor bytes read from the loader, unpack kernels launched, microseconds in
 *   loader->read for tensor bytes, microseconds waiting for the device, microseconds for the whole load }. */
WHISPER_API int64_t whisper_amd_arena_read(struct whisper_context * ctx, int64_t offset, void * dst, int64_t cap);
WHISPER_API void    whisper_amd_load_stats(struct whisper_context * ctx, int64_t out[6]);

/* Audio front end (wa_audio.cpp): a recording as it comes out of a WAV file (whisper_amd_wav_parse reads the header) - 8-, 16-, 24- or
 * 32-bit PCM, F32, F64 or G.711 mu-law / A-law samples, one or two interleaved channels, 8 .. 192 kHz - converted, down-mixed and resampled to the 16 kHz mono F32 that whisper_full* takes, by HIP kernels on the
 * state's stream.  whisper-rs callers do the first two steps on the host (src/utilities.rs) and its examples refuse every rate but 16 kHz.
 * At 16 kHz the result is bit-identical to those utilities: I16 mono (float) s / 32768.0f, F32 stereo (l + r) / 2.0f, I16 stereo
 * ((float) l + (float) r) / 2.0f / 32768.0f.  Other rates R go through a polyphase Kaiser-windowed sinc (g = gcd(R, 16000), L = 16000 / g,
 * M = R / g; accepted: 8000 <= R <= 192000 with L <= 640, which covers 8, 11.025, 12, 16, 22.05, 24, 32, 44.1, 48, 88.2, 96, 176.4 and
 * 192 kHz): ceil(n_frames 16000 / R) samples, each one F32 fmaf chain over its K taps (csrc/wa_audio.h states the arithmetic; the kernels
 * and the host restatement there agree bit for bit).
 * Refused, with an error log, -1 (whisper_amd_audio_to_pcm: NULL) and nothing written: null data with n_frames > 0, n_frames < 0, channels
 * other than 1 or 2, an unknown format, a rate outside the rule above.
 * whisper_amd_audio_n_samples: the output length for n_frames at sample_rate.
 * whisper_amd_audio_to_pcm: `data` is a host or a device pointer (detected as whisper_pcm_to_mel does).  Returns a DEVICE pointer to
 *   *n_samples F32 samples in a buffer the state owns (grown when needed, freed with the state), filled on the state's stream and valid until
 *   the next call on this state; hand it to whisper_full_with_state / whisper_pcm_to_mel_with_state of the same state without any
 *   synchronisation.  Host input may be released on return.  n_frames == 0 gives 0 samples and a non-null pointer.  The filter table of a
 *   rate is built once per context and kept.  A HIP failure on the way is logged and the call is served by the host restatement;
 *   WHISPER_AMD_AUDIO_HOST=1 in the environment when a state is created sends every call on that state there.
 * whisper_amd_full_audio: whisper_amd_audio_to_pcm, then whisper_full_with_state on its result; returns that call's code.
 * whisper_amd_audio_copy: copies up to `cap` samples of the state's last result into `dst` (host) and returns their full count; -1: none yet.
 * whisper_amd_audio_taps: the filter table of a rate, taps[L][K] phase-major (output n, t = n M: phase t mod L, first input frame
 *   t / L - K/2 + 1); copies up to `cap` values, returns L K (0 at 16 kHz: no filter); no device needed.
 * whisper_amd_audio_tile: outputs per workgroup of the resampling kernel (tests put lengths on either side of it).
 * whisper_amd_audio_stats: out = { calls served by the kernels, calls served by the host restatement, kernel attempts that fell back to
 *   it } since the state was created (calls with no output sample count nowhere).
 *
 * Sample formats.  Every entry that takes a `format` (here, whisper_amd_full_long_audio, whisper_amd_audio_split,
 * whisper_amd_full_long_channels, and whisper_amd_stream_open / _open_vad through their params) takes every code below; 2, anything above 8
 * and every negative code are refused.  A sample becomes a value v in F32 and is divided by the format's scale S, every operation rounded
 * on its own: U8 v = (float) ((int) u - 128), S = 128; S24 (3 bytes little-endian, packed) v = (float) s, S = 8388608; S32 v = (float) s
 * rounded to nearest even, S = 2147483648; F64 v = (float) x rounded to nearest even, no scale, NaN and Inf passing through as F32's do;
 * ULAW / ALAW v = (float) e with e the G.711 expansion to int16 (csrc/wa_audio.h: wa_audio_ulaw, wa_audio_alaw), S = 32768.  Mono v / S,
 * stereo ((vl + vr) / 2.0f) / S.  So G.711 input gives, bit for bit, what I16 input holding the expanded samples gives, and U8 / S24 / S32 /
 * F64 input what F32 input holding the per-sample v / S gives.
 * Alignment: a HOST pointer may have any alignment in every format (the samples of a WAV image lie where its header ends).  A DEVICE pointer
 * may be any byte address for U8, ULAW, ALAW and S24, and must be naturally aligned (2, 4, 4, 8 bytes) for I16, S32, F32 and F64.
 *
 * whisper_amd_wav_parse: walks the header of a RIFF/WAVE image in host memory (`size` bytes) and fills `out`: data_offset - the byte offset of
 *   the first sample -, n_frames, channels, sample_rate, format (a code below) and bits, ready to hand `(char *) image + data_offset` and the
 *   rest to any entry above.  PCM of 8 / 16 / 24 / 32 bits (tag 1), IEEE float of 32 / 64 bits (tag 3), A-law (6) and mu-law (7), plain or
 *   in the extensible form (tag 0xFFFE with the standard sub-format GUID, valid bits equal to container bits); nBlockAlign must be
 *   channels * bits / 8.  The data length is the smaller of the declared one and what the image holds; a declared 0 or 0xFFFFFFFF means "to
 *   the end"; n_frames rounds down.  Channels and rate are reported as found.  Returns 0, or -1 null or short arguments, -2 not RIFF ... WAVE
 *   (RF64 and RIFX included), -3 a malformed chunk list or no "fmt " chunk before "data", -4 an unsupported encoding or an nBlockAlign that
 *   does not fit it, -5 no "data" chunk; on failure *out is untouched.  No device needed. */
#define WHISPER_AMD_PCM_I16  0
#define WHISPER_AMD_PCM_F32  1
#define WHISPER_AMD_PCM_U8   3   /* unsigned 8-bit PCM */
#define WHISPER_AMD_PCM_S24  4   /* signed 24-bit PCM, 3 bytes little-endian, packed */
#define WHISPER_AMD_PCM_S32  5   /* signed 32-bit PCM */
#define WHISPER_AMD_PCM_F64  6   /* IEEE double */
#define WHISPER_AMD_PCM_ULAW 7   /* G.711 mu-law */
#define WHISPER_AMD_PCM_ALAW 8   /* G.711 A-law */
struct whisper_amd_wav_info { int64_t data_offset, n_frames; int32_t channels, sample_rate, format, bits; };
WHISPER_API int           whisper_amd_wav_parse(const void * image, int64_t size, struct whisper_amd_wav_info * out);
WHISPER_API int64_t       whisper_amd_audio_n_samples(int64_t n_frames, int sample_rate);
WHISPER_API const float * whisper_amd_audio_to_pcm(struct whisper_state * state, const void * data, int64_t n_frames, int channels,
                                                   int sample_rate, int format, int64_t * n_samples);
WHISPER_API int           whisper_amd_full_audio(struct whisper_context * ctx, struct whisper_state * state, struct whisper_full_params params,
                                                 const void * data, int64_t n_frames, int channels, int sample_rate, int format);
WHISPER_API int64_t       whisper_amd_audio_copy(struct whisper_state * state, float * dst, int64_t cap);
WHISPER_API int64_t       whisper_amd_audio_taps(int sample_rate, float * dst, int64_t cap, int * L, int * M, int * K);
WHISPER_API int           whisper_amd_audio_tile(void);
WHISPER_API void          whisper_amd_audio_stats(struct whisper_state * state, long out[3]);

/* Long recordings (wa_long.cpp): a recording of any length cut at the silences the VAD found, the speech packed into chunks of
 * at most max_chunk_ms, the chunks transcribed in lock-step waves, the times mapped back.  A chunk is whisper_full_with_state on that chunk's
 * speech-only audio and nothing else, so every chunk's result is the one that call gives for it alone.
 * whisper_vad_detect_speech (and every call built on it: whisper_vad_segments_from_samples, whisper_full* with vad = true) takes a host or a
 *   device pointer, detected as whisper_pcm_to_mel does; device audio is read in place, on the VAD context's OWN stream, which is ordered
 *   against no other: work that still writes the audio on another stream - whisper_amd_audio_to_pcm's on its state's stream, a caller's own
 *   kernel - is the caller's to finish first (hipStreamSynchronize on that stream).  whisper_amd_full_long does that for ctx->state's stream.
 * whisper_amd_full_long, on the context's own state (ctx->state):
 *   - `samples` is a host or a device pointer.  Host PCM is uploaded once into a buffer the state owns; device PCM is read where it lies (work
 *     on it that the caller queued on another stream than the state's is the caller's to finish first).
 *   - max_chunk_ms <= 0 means 30000; n_parallel <= 0 means 8; n_parallel is clamped to 8 (the lock-step group's width).
 *   - params.vad_model_path and params.vad_params are used; params.vad itself is not looked at.  The VAD context is the one
 *     whisper_full(vad = true) keeps on the state.
 *   - Chunks: greedy, in order, whole VAD segments.  A chunk takes the next segment while its packed length stays <= max_chunk_ms; a single
 *     segment longer than that is a chunk of its own and whisper_full's 30 s window loop covers it.  Packed length, audio and time table of a
 *     chunk are what whisper_full(vad = true) makes of that run of segments taken as the whole list, with the caller's n_samples: the
 *     chunk's last segment gets no overlap extension and no trailing silence, the n_samples - 1 / n_samples clamps apply, 0.1 s of silence
 *     stands between segments, the table's original times are the caller's.  A chunk shorter than 100 ms gives no segments, as whisper_full
 *     on it would; nothing is padded.
 *   - One launch of k_long_pack writes every chunk into one allocation of the state, each chunk on a 256-byte boundary, byte for byte what
 *     the host function gives.  WHISPER_AMD_LONG_HOST=1 in the environment, read at each call, takes the host function instead; so does a
 *     call whose HIP path fails (logged, counted).  VAD and pack are complete before the first wave starts.
 *   - The chunks run in waves of up to n_parallel, as whisper_amd_full_batch runs its chunks: one state, host thread and stream per member,
 *     single-token steps in lock step.  Member params follow whisper_full_parallel's members: new_segment and progress callbacks nulled,
 *     print_* off.  encoder_begin_callback, abort_callback and logits_filter_callback stay set and are called CONCURRENTLY from up to
 *     n_parallel threads, as whisper_full_parallel's members call them: what they touch must be safe for that.  The states beside ctx->state
 *     are made for the call and released at its end.  Chunks are independent: no prompt is carried from one chunk to the next, whatever
 *     no_context says and whatever the context transcribed before (no_context = false still carries the context from one 30 s window to the
 *     next INSIDE a chunk longer than 30 s); initial_prompt applies to each.  whisper_amd_batch_stats then sums the call's waves.
 *   - Results are appended to ctx->state in chunk order with t0 / t1 ALREADY mapped into the caller's audio through the chunk's table; a
 *     segment lasts at least 10 cs (t1 >= t0 + 10, the getters' rule), then t0 = max(t0, previous segment's t1).  The state's own VAD table
 *     is cleared, so the getters return the stored times.  Token t0 / t1 / t_dtw that are >= 0 are mapped the same way.
 *     new_segment_callback fires on ctx->state once per appended segment; whisper_full_lang_id is the first chunk's.
 *   - Returns 0 with no segments when the VAD finds no speech (earlier results are cleared, as whisper_full does); -1 with a log line for a
 *     missing or refused VAD model, non-zero offset_ms / duration_ms (not supported here) and null arguments; otherwise the first non-zero
 *     chunk code, with the results and the chunk list cleared.  No exception crosses the boundary.
 * whisper_amd_full_long_audio: whisper_amd_audio_to_pcm on ctx->state, then whisper_amd_full_long on its device result.
 * whisper_amd_long_n_chunks / _chunk_info: the last call's chunks; out = { first segment, segment count, packed samples, original start cs,
 *   original end cs, result segments }; -1 for an index out of range.
 * whisper_amd_long_chunk_copy: the packed PCM of chunk i, kept until the next call: copies up to `cap` samples, returns their full count.
 * whisper_amd_long_stats: out = { pack path taken (0 host, 1 kernel), device packs that fell back since the state was created, chunks, waves,
 *   us VAD, us plan + pack, us transcription (member states made and released, waves, mapping), bytes of the CALLER'S recording copied host -> device (0 for device
 *   input; the pack's piece table and, on the host pack path, the packed chunks it uploads are not counted) } of the last whisper_amd_full_long
 *   call; whisper_amd_long_pack sets the first, the third and the last for its own call.
 * whisper_amd_long_plan: the planner alone, no device needed: segs_cs = n_segs pairs (start, end) in centiseconds; writes up to `cap` chunks,
 *   returns their full count, -1 for refused arguments.
 * whisper_amd_long_pack: the pack alone on a caller's segment list and runs (first[c], count[c]); where = 0 the host function, 1 the kernel
 *   (no fallback); 0 on success.  The chunks are then read with whisper_amd_long_chunk_copy on the state's context when `state` is its own state.
 * whisper_amd_long_tile: output samples per workgroup of k_long_pack (tests put piece boundaries on either side of it).
 * whisper_amd_context_state: ctx->state, for the calls above that take a state. */
WHISPER_API int     whisper_amd_full_long(struct whisper_context * ctx, struct whisper_full_params params, const float * samples, int n_samples,
                                          int max_chunk_ms, int n_parallel);
WHISPER_API int     whisper_amd_full_long_audio(struct whisper_context * ctx, struct whisper_full_params params, const void * data, int64_t n_frames,
                                                int channels, int sample_rate, int format, int max_chunk_ms, int n_parallel);
WHISPER_API int     whisper_amd_long_n_chunks(struct whisper_context * ctx);
WHISPER_API int     whisper_amd_long_chunk_info(struct whisper_context * ctx, int i, int64_t out[6]);
WHISPER_API int64_t whisper_amd_long_chunk_copy(struct whisper_context * ctx, int i, float * dst, int64_t cap);
WHISPER_API void    whisper_amd_long_stats(struct whisper_context * ctx, int64_t out[8]);
WHISPER_API int     whisper_amd_long_plan(const int64_t * segs_cs, int n_segs, int n_samples, float samples_overlap, int max_chunk_samples,
                                          int32_t * first, int32_t * count, int64_t * packed, int cap);
WHISPER_API int     whisper_amd_long_pack(struct whisper_state * state, const float * samples, int n_samples, const int64_t * segs_cs, int n_segs,
                                          float samples_overlap, const int32_t * first, const int32_t * count, int n_chunks, int where);
WHISPER_API int     whisper_amd_long_tile(void);
WHISPER_API struct whisper_state * whisper_amd_context_state(struct whisper_context * ctx);

/* Two-channel recordings (wa_channels.cpp): a stereo call recording carries one speaker per channel.  The audio front end
 * above can only average the two; the calls here keep them apart: both channels as two planes of 16 kHz F32 from ONE launch, the energy of
 * spans of either plane, the reference cli's --diarize rule, and whisper_amd_full_long for both channels in one call, whose chunks share
 * the lock-step waves.  csrc/wa_channels.h states every piece of arithmetic once; the kernels and the host functions there agree bit for bit.
 * whisper_amd_audio_split: `data` is a host or a device pointer (detected as whisper_pcm_to_mel does) to n_frames interleaved STEREO frames,
 *   int16 or F32, at any rate whisper_amd_audio_to_pcm accepts.  Returns a DEVICE pointer to a planar buffer the state owns: channel c lies
 *   at ptr + c * *stride, *n_samples F32 samples each, *stride = *n_samples rounded up to 64 floats (the floats between a plane's end and
 *   the stride are undefined).  Plane c is, bit for bit, what whisper_amd_audio_to_pcm gives for channel c presented as a mono recording of
 *   the same rate and format, with the context's filter table for that rate.  The buffer is an allocation of its own - not
 *   whisper_amd_audio_to_pcm's - filled on the state's stream, kept until the next split on this state and freed with the state.  Host input
 *   may be released on return.  n_frames == 0 gives 0 samples and a non-null pointer.  Refused as whisper_amd_audio_to_pcm refuses (NULL, an
 *   error log line, nothing written), also for a null n_samples or stride.  A HIP failure on the way is logged, counted and served by the host
 *   restatement; WHISPER_AMD_CHANNELS_HOST=1 in the environment, read at each call, sends split and energy to the host functions.
 * whisper_amd_audio_split_copy: copies up to `cap` samples of plane `channel` of the state's last split into `dst` (host) and returns their
 *   full count; -1: no split yet, or a channel other than 0 / 1.
 * whisper_amd_channel_energy: energy[2 i + c] = the sum of |x_c[j]| over j in [is0[i], is1[i]) of the state's last split, in F64, spans
 *   clamped to [0, n_samples], 0.0 for an empty span; ONE launch serves all spans of both channels, without atomics, in the fixed order of
 *   csrc/wa_channels.h (lane l of whisper_amd_channels_energy_lanes() takes the samples whose index is l modulo that count, ascending, then a
 *   stated tree), which does not depend on launch geometry.  where: 0 the host function, 1 the kernel (no fallback), any other value the
 *   kernel with the host function behind it (and WHISPER_AMD_CHANNELS_HOST honoured).  0 on success, -1 refused or failed.
 * whisper_amd_channel_speakers: the reference cli's --diarize rule (examples/cli/cli.cpp) on caller-given times in centiseconds: sample
 *   = clamp((int) (t * 16000 / 100), 0, n_samples - 1) (kept in 64 bits: beyond the 37 h at which the cli's int cast stops being defined it is
 *   n_samples - 1), energies over [sample(t0), sample(t1)), then in F64 e0 > ratio * e1 -> 0, else
 *   e1 > ratio * e0 -> 1, else -1 (undecided: the cli prints "?"); ratio <= 0 means the cli's 1.1.  `energy` ([n][2]) may be null.  With
 *   whisper_amd_full_long_audio (the down-mix) followed by whisper_amd_audio_split and this call on the segment times a caller gets what
 *   cli --diarize prints.  The cli sums sequentially; the fixed order here differs from that by at most n 2^-53 relative, so the labels
 *   agree wherever the energies are not within that of the threshold.
 * whisper_amd_full_long_channels, on the context's own state: whisper_amd_full_long for both channels of one recording in one call.
 *   - One whisper_amd_audio_split: the recording crosses PCIe once (host input) or never (device input).
 *   - The VAD runs per plane, where it lies, on the state's VAD context, channel 0 then channel 1.
 *   - crosstalk_ratio = g > 0: ONE energy launch covers every VAD segment of both channels over its own span [cs_to_samples(start),
 *     min(cs_to_samples(end), n_samples)); a segment of channel c is dropped when E_c < g * E_other (the other speaker bleeding through).
 *     g = 0 launches nothing and drops nothing; g < 0 is refused.
 *   - The chunk planner runs per channel over that channel's kept segments (max_chunk_ms <= 0 means 30000); ONE launch of k_long_pack packs
 *     the chunks of both channels (WHISPER_AMD_LONG_HOST=1 keeps meaning the host pack).
 *   - All chunks form one list ordered by (original start, channel) and run in waves of n_parallel (<= 0 means 8, clamped to 8) exactly as
 *     whisper_amd_full_long's: C0 + C1 chunks take ceil((C0 + C1) / n_parallel) waves.  Member params, callbacks and prompt rules are those
 *     of whisper_amd_full_long.
 *   - Results: per channel, times mapped and clamped as whisper_amd_full_long does - at least 10 cs, t0 = max(t0, t1 of the previous segment
 *     OF THE SAME CHANNEL): overlapping speech on the two channels stays overlapping - then both channels' segments are merged into
 *     ctx->state's list by (t0, channel); a channel's segments always keep their own order (csrc/wa_channels.h: wa_ch_merge).  new_segment_callback fires once per merged segment, in merged order;
 *     whisper_full_lang_id is the first chunk's in wave order; the state's VAD table is cleared.  whisper_amd_long_n_chunks / _chunk_info /
 *     _chunk_copy describe the chunks in wave order (segment indices count within the chunk's channel, after the gate).
 *   - With crosstalk_ratio = 0 the segments of channel c in the merged list are exactly what whisper_amd_full_long gives on
 *     whisper_amd_audio_to_pcm of channel c extracted on the host: texts, token ids, p / plog bit patterns, t0 / t1 and token times.
 *   - Returns 0 with no segments when neither channel has speech, 0 with one channel's segments when only one has; -1 with a log line for
 *     null arguments, what the split refuses, n_frames == 0, more than INT_MAX samples, non-zero offset_ms / duration_ms, a negative
 *     crosstalk_ratio (all of these before anything of the state is touched) and for a missing or refused VAD model; otherwise the first
 *     non-zero chunk code; results and chunk list are then cleared.  No exception crosses the boundary.
 * whisper_amd_long_segment_channel / whisper_amd_long_chunk_channel: the channel (0 / 1) of result segment / chunk i of the last call;
 *   -1: out of range, or the last long call had no channels.
 * whisper_amd_channels_stats: out = { split path taken (0 host, 1 kernel), split attempts on the device that fell back since the state was
 *   created, energy launches, pack launches, VAD segments found on channel 0, on channel 1, segments dropped by the gate, chunks, waves,
 *   bytes of the CALLER'S recording copied host -> device (0 for device input), energy launches whose result did not arrive and that the host
 *   function served instead since the state was created (a launch that took place counts as a launch too) } of the last
 *   whisper_amd_full_long_channels call;
 *   whisper_amd_long_stats then holds its times: us in the two VAD passes, us gate + plan + pack, us transcription.
 * whisper_amd_channels_tile: outputs per channel and workgroup of the split kernel (tests put lengths on either side of it). */
struct whisper_amd_channels_params {
    int32_t max_chunk_ms;        /* 30000 */
    int32_t n_parallel;          /* 8 */
    double  crosstalk_ratio;     /* 0.0: the gate is off */
};
WHISPER_API const float * whisper_amd_audio_split(struct whisper_state * state, const void * data, int64_t n_frames, int sample_rate, int format,
                                                  int64_t * n_samples, int64_t * stride);
WHISPER_API int64_t       whisper_amd_audio_split_copy(struct whisper_state * state, int channel, float * dst, int64_t cap);
WHISPER_API int           whisper_amd_channel_energy(struct whisper_state * state, const int64_t * is0, const int64_t * is1, int n_spans, int where,
                                                     double * energy);
WHISPER_API int           whisper_amd_channel_speakers(struct whisper_state * state, const int64_t * t0_cs, const int64_t * t1_cs, int n, double ratio,
                                                       double * energy, int8_t * speaker);
WHISPER_API void          whisper_amd_channels_default_params(struct whisper_amd_channels_params * p);
WHISPER_API int           whisper_amd_full_long_channels(struct whisper_context * ctx, struct whisper_full_params params,
                                                         const struct whisper_amd_channels_params * cp, const void * data, int64_t n_frames,
                                                         int sample_rate, int format);
WHISPER_API int           whisper_amd_long_segment_channel(struct whisper_context * ctx, int i_segment);
WHISPER_API int           whisper_amd_long_chunk_channel(struct whisper_context * ctx, int i_chunk);
WHISPER_API void          whisper_amd_channels_stats(struct whisper_context * ctx, int64_t out[11]);
WHISPER_API int           whisper_amd_channels_tile(void);
WHISPER_API int           whisper_amd_channels_energy_lanes(void);

/* Forced alignment (wa_align.cpp): the audio and the text are both known; when was each token said, and how well does the
 * model agree with it?  One teacher-forced decoder pass over [sot, lang, not, tokens..., eot] - the pass whisper_full's DTW runs over its own
 * result - whose logits rows stay on the device: k_align_score (wa_align.hip) turns each row into one record there.
 * The scores are taken on the RAW logits of the model.  No suppression list, no blank or non-speech rule and no timestamp rule applies: this
 * is the model's distribution over the vocabulary, not the choice of whisper_full's sampler (whose plog / p follow its own rules and its own
 * F32 summation order).  For a row with logits x and target t (csrc/wa_align.h states it once more, with the host function):
 *   mx = max x, best_id = the lowest index that attains it; lse = mx + log(sum_i exp((double) x_i - (double) mx)), sum and exp in F64;
 *   plog = (float) (x_t - lse), p = (float) exp(x_t - lse); best_plog / best_p the same for best_id;
 *   rank = #{ i : x_i > x_t or (x_i == x_t and i < t) } - 0 where the target is the model's own choice;
 *   a -inf logit adds 0 to the sum; a -inf target gives plog = -inf, p = 0.
 *   (Evaluated as (x_t - mx) - log1p(sum over i != best_id): the same value, precise also where the model is sure and plog approaches -0.)
 * Layouts are ABI: whisper_amd_align_score 24 bytes (plog 0, p 4, best_id 8, best_plog 12, rank 16, best_p 20), whisper_amd_align_token
 * 32 bytes (id 0, plog 4, p 8, best_id 12, best_plog 16, rank 20, t_dtw 24).
 * whisper_amd_align: one window.  Log-mel of `samples` (a host or a device pointer, detected as whisper_pcm_to_mel does), the encoder at
 *   params.offset_ms / 10, the sequence [sot, lang, not, tokens..., eot] - lang on multilingual models only: params.language, detected when
 *   that is null, "" or "auto" -, one decoder pass, the scores with target = the next token, and - on a context created with
 *   dtw_token_timestamps and a preset - the DTW alignment over the window's frames (to the end of the audio or of params.duration_ms, at
 *   most 30 s).  out[i], i < n_tokens, belongs to tokens[i]; out[n_tokens] is the row of the closing eot (id = eot, t_dtw = -1).  t_dtw is
 *   placed as whisper_full places it: the first time index of the token's run on the path x 2 + offset, in centiseconds; -1 for every token
 *   on a context without alignment heads, and for the tokens that the path does not reach.
 *   Returns 0, or - with an error log line, nothing written and the state as usable as before -
 *     WHISPER_AMD_ALIGN_BAD_TOKEN   a token < 0 or >= eot (text tokens only: no timestamps, no specials)
 *     WHISPER_AMD_ALIGN_NO_TOKENS   n_tokens <= 0, or a null pointer among the arguments
 *     WHISPER_AMD_ALIGN_TOO_LONG    the sequence has more rows than the state's decoder holds (the text context; walk windows with offset_ms)
 *     WHISPER_AMD_ALIGN_FLASH_ATTN  the context was created with flash_attn: only the exact path is scored
 *     WHISPER_AMD_ALIGN_TOO_SHORT   less than 100 ms of audio after the offset
 *   or whisper_full's codes for the stages they share: -2 mel, -3 language detection, -6 encode, -8 decode (and the scores' launch or copy).
 *   The state's results (segments, tokens) are not touched; its self-attention cells are cleared, so that whisper_full afterwards behaves as
 *   on a fresh state.  The pass's logits never reach the host and it does not write whisper_get_logits_from_state (language detection, where
 *   the call has to do it, is whisper_lang_auto_detect_with_state at offset 0 as in whisper_full: one single-token pass that does).
 * whisper_amd_align_score: the scores alone, for a caller's own logits - host [n_rows][n_vocab] F32, target[n_rows] in [0, n_vocab).
 *   where = 0: the host function.  where = 1: uploaded into the state's buffer and scored by the launcher of the product path, on the state's
 *   stream.  The two agree in best_id and rank; plog / p may differ in the last bit of an F64 exp.  0, WHISPER_AMD_ALIGN_NO_TOKENS for refused
 *   arguments (nothing written), -8 for a HIP failure.
 * whisper_amd_align_stats: out = { whisper_amd_align calls that returned 0, logits rows scored by the kernel, bytes of logits that stayed on
 *   the device (rows x n_vocab x 4, whisper_amd_align's rows only) } since the state was created.
 * whisper_amd_align_timings: out = { device time in us of the last k_align_score launch on this state, between two HIP events; wall time in
 *   us of the last whisper_amd_align call } (tools/align_probe.py). */
#define WHISPER_AMD_ALIGN_BAD_TOKEN  (-21)
#define WHISPER_AMD_ALIGN_NO_TOKENS  (-22)
#define WHISPER_AMD_ALIGN_TOO_LONG   (-23)
#define WHISPER_AMD_ALIGN_FLASH_ATTN (-24)
#define WHISPER_AMD_ALIGN_TOO_SHORT  (-25)
struct whisper_amd_align_score { float plog; float p; int32_t best_id; float best_plog; int32_t rank; float best_p; };
struct whisper_amd_align_token { whisper_token id; float plog; float p; whisper_token best_id; float best_plog; int32_t rank; int64_t t_dtw; };
WHISPER_API int  whisper_amd_align(struct whisper_context * ctx, struct whisper_state * state, struct whisper_full_params params,
                                   const float * samples, int n_samples, const whisper_token * tokens, int n_tokens,
                                   struct whisper_amd_align_token * out);
WHISPER_API int  whisper_amd_align_score(struct whisper_state * state, const float * logits, int n_rows, int n_vocab, const int32_t * target,
                                         int where, struct whisper_amd_align_score * out);
WHISPER_API void whisper_amd_align_stats(struct whisper_state * state, long out[3]);
WHISPER_API void whisper_amd_align_timings(struct whisper_state * state, int64_t out[2]);

/* Live streaming sessions (wa_stream.cpp): audio transcribed while it arrives, in the sliding windows of the reference's
 * examples/stream/stream.cpp (its step mode).  A session owns a state, a 16 kHz ring in device memory and the resampler's carry; the caller
 * pushes packets of any size in the session's rate, channel count and format (what whisper_amd_audio_to_pcm takes) and runs the windows that
 * became due.  Every struct travels by pointer.  One thread at a time per session.  No exception crosses the boundary.
 * Sizes: keep_ms = min(keep_ms, step_ms), length_ms = max(length_ms, step_ms); n_step, n_len, n_keep = (int) ((1e-3 ms) * 16000) samples;
 *   n_new_line = max(1, length_ms / step_ms - 1).
 * Window k consumes exactly n_step new samples: take = min(old, max(0, n_keep + n_len - n_step)); the window is the last `take` samples of the
 *   previous window followed by the new ones; old becomes the window's length.  After the window's whisper_full the iteration count goes up by
 *   one; when it is a multiple of n_new_line the line is COMMITTED: old becomes the window's last n_keep samples and, with carry_prompt, the
 *   prompt of the following windows becomes every token id of every segment of this window's result (until the next commit it stays what it
 *   was).  Without drops window k is the range [e - len, e) of the session's 16 kHz sample axis, e = (k + 1) n_step, len <= n_keep + n_len.
 *   stream.cpp's VAD mode (step_ms <= 0) is whisper_amd_stream_open_vad below: utterances cut at pauses by the Silero VAD, not by vad_simple.
 * The 16 kHz axis of a session is whisper_amd_audio_to_pcm's of the whole input, bit for bit, however the input is cut into packets: sample n
 *   becomes final - is written to the ring - with the packet that brings the last frame its filter reads (floor(n M / L) + K/2), and
 *   whisper_amd_stream_flush releases the rest, the frames behind the end of input read as zero.
 * whisper_amd_stream_open: refused (NULL, an error log line, nothing made) for null arguments, a rate, channel count or format that
 *   whisper_amd_audio_to_pcm refuses, step_ms <= 0, and keep_ms + length_ms > 30000 after the clamps.  A flash_attn context is served.  The
 *   ring holds n_keep + n_len + backlog samples, backlog = backlog_ms x 16 (at least 2 n_step + 1).  WHISPER_AMD_STREAM_HOST=1 in the
 *   environment when the session opens keeps ring and carry on the host and serves every feed and gather by the host restatement
 *   (csrc/wa_stream.h); a session whose HIP path fails moves there for good (logged; whisper_amd_stream_info counts the feeds each way).
 * whisper_amd_stream_feed: `data` is a host or a device pointer (detected as whisper_pcm_to_mel does) to n_frames frames.  One kernel launch on
 *   the state's stream; host input may be released on return, device input stays stream-ordered.  Returns the number of windows now due, or
 *   WHISPER_AMD_STREAM_FULL with NOTHING changed when the packet's samples do not fit the backlog beside those still unconsumed (drop_late = 1:
 *   the unconsumed samples are discarded and counted first, as a late step would; FULL only for a packet larger than the backlog itself),
 *   WHISPER_AMD_STREAM_ENDED after a flush, WHISPER_AMD_STREAM_BAD_ARGS for null or negative arguments.
 * whisper_amd_stream_flush: the end of input.  Releases the filter's tail; what is left behind the last whole step becomes one last, shorter
 *   window.  Returns the windows due.  Feeds are refused until whisper_amd_stream_reset.
 * whisper_amd_stream_pending: the windows due.
 * whisper_amd_stream_step: runs ONE due window: one gather launch into the state's PCM buffer, then whisper_full_with_state on it with *params
 *   as the caller gave them, but for prompt_tokens / prompt_n_tokens, which are the session's when carry_prompt is set.  stream.cpp's own
 *   settings are the recommended ones: single_segment = true, no_timestamps = true, an audio_ctx that fits the window.  The result is, bit for
 *   bit, what whisper_full_with_state gives on that state for those samples and that prompt; read it with whisper_full_*_from_state on
 *   whisper_amd_stream_state.  Returns 1, 0 when no window is due, whisper_full's negative code when it fails (the window's audio counts as
 *   consumed), or a WHISPER_AMD_STREAM_* code.  drop_late = 1 is stream.cpp's rule: when more than 2 n_step new samples are pending at a step,
 *   all of them are discarded and counted and NO window runs (0); the next window is then the old tail followed by fresh audio.
 * whisper_amd_stream_step_many: one due window of every session of `ss` that has one.  All sessions belong to one context
 *   (WHISPER_AMD_STREAM_MIXED otherwise, and for n > 64).  Groups of up to 8: ONE gather launch for the group, then its members run as
 *   whisper_amd_full_batch runs its chunks - a host thread, state and stream per member, single-token steps in lock step - each with its own
 *   params copy.  Callbacks follow whisper_amd_full_long's rule: new_segment and progress callbacks nulled, print_* off; encoder_begin, abort
 *   and logits_filter callbacks stay set and are called concurrently.  Every session's result is the one whisper_amd_stream_step gives it
 *   alone.  Returns the number of windows that ran, or the first failure's code.  whisper_amd_batch_stats then describes the call's groups.
 * whisper_amd_stream_info: out = { windows run, the last window's start on the absolute 16 kHz axis, its length, its take, whether it committed
 *   (0 / 1), the prompt tokens it ran with, samples dropped, windows due, feeds served by the kernels, feeds served by the host restatement }.
 * whisper_amd_stream_window_copy / _prompt_copy: the last window's PCM / the prompt it ran with: copies up to `cap`, returns the full count.
 * whisper_amd_stream_reset: forget everything fed; the next window equals a fresh session's first.
 * whisper_amd_stream_tile: outputs per workgroup of the two kernels (tests put packet and window sizes on either side of it). */
#define WHISPER_AMD_STREAM_BAD_ARGS (-31)
#define WHISPER_AMD_STREAM_FULL     (-32)
#define WHISPER_AMD_STREAM_ENDED    (-33)
#define WHISPER_AMD_STREAM_MIXED    (-34)
#define WHISPER_AMD_STREAM_FAILED   (-35)
struct whisper_amd_stream;
struct whisper_amd_stream_params {
    int32_t step_ms;        /* 3000  */
    int32_t length_ms;      /* 10000 */
    int32_t keep_ms;        /* 200   */
    int32_t sample_rate;    /* 16000 */
    int32_t channels;       /* 1     */
    int32_t format;         /* WHISPER_AMD_PCM_F32 */
    int32_t backlog_ms;     /* 30000: unconsumed audio the ring holds beside one window */
    int32_t carry_prompt;   /* 1: stream.cpp without --no-context */
    int32_t drop_late;      /* 0 */
};
WHISPER_API void    whisper_amd_stream_default_params(struct whisper_amd_stream_params * p);
WHISPER_API struct whisper_amd_stream * whisper_amd_stream_open(struct whisper_context * ctx, const struct whisper_amd_stream_params * p);
WHISPER_API void    whisper_amd_stream_close(struct whisper_amd_stream * s);
WHISPER_API int     whisper_amd_stream_feed(struct whisper_amd_stream * s, const void * data, int64_t n_frames);
WHISPER_API int     whisper_amd_stream_flush(struct whisper_amd_stream * s);
WHISPER_API int     whisper_amd_stream_pending(struct whisper_amd_stream * s);
WHISPER_API int     whisper_amd_stream_step(struct whisper_amd_stream * s, const struct whisper_full_params * params);
WHISPER_API int     whisper_amd_stream_step_many(struct whisper_amd_stream ** ss, int n, const struct whisper_full_params * params);
WHISPER_API struct whisper_state * whisper_amd_stream_state(struct whisper_amd_stream * s);
WHISPER_API int     whisper_amd_stream_info(struct whisper_amd_stream * s, int64_t out[10]);
WHISPER_API int64_t whisper_amd_stream_window_copy(struct whisper_amd_stream * s, float * dst, int64_t cap);
WHISPER_API int     whisper_amd_stream_prompt_copy(struct whisper_amd_stream * s, whisper_token * dst, int cap);
WHISPER_API void    whisper_amd_stream_reset(struct whisper_amd_stream * s);
WHISPER_API int     whisper_amd_stream_tile(void);

/* Live sessions that cut at pauses (wa_stream.cpp, csrc/wa_stream_vad.h): nothing runs while the line is silent, and each
 * utterance is transcribed once, when the speaker pauses.  The yardstick is stated offline.  Let x[0..T) be the session's 16 kHz axis (above), P
 * the probabilities whisper_vad_detect_speech gives on x, S the segments whisper_vad_segments_from_probs gives for params->vad.  Utterance j is
 * the contiguous range [cs_to_samples(S[j].start), min(cs_to_samples(S[j].end), T)) - none of vad = true's overlap or inserted silence.  A VAD
 * session delivers exactly these utterances, in order, however the input was cut into packets, each one as soon as later audio can no longer
 * change it, the rest at the flush; its probabilities so far are the first windows of P, bit for bit (the session carries the LSTM state from
 * one 512-sample window to the next; the last partial window exists only at the flush, zero-filled).
 * When an utterance is due: its last speech ended at sample e (a multiple of 512) and the window that ends at or beyond e + 3200 has been
 *   processed with no speech candidate open - the reference merges neighbours less than 3200 samples apart, so a candidate that opened inside
 *   that gap is waited for until the rules have kept or discarded it.  Delay bound, in samples fed beyond e, when nothing reaches the threshold
 *   behind e: max(ceil512(min_silence_samples) + 512, 3584) plus what the resampler holds back (K/2 input frames) and, with vad_on_feed = 0, the
 *   time to the next poll.  A candidate behind e is decided at most max_speech_duration_s later.
 * The length cap: an utterance holds at most max_utterance_ms (<= 30000: the state's PCM buffer; vad.max_speech_duration_s may not exceed it).
 *   The reference's merge pass can re-join what max_speech split; a merge whose result would exceed the cap is NOT made: the earlier part is
 *   delivered as it stands, flagged `split`, and the rest follows as the next utterance.  This is the one departure from S; for inputs whose S
 *   has no segment over the cap the utterances ARE S.  (csrc/wa_stream_vad.h states the rule; tools/stream_vad_ref.py restates it.)
 * Prompt: carry_prompt = 0 (stream.cpp's VAD mode never fills prompt_tokens): every utterance runs with the caller's prompt.  1: utterance j + 1
 *   runs with every token id of utterance j's result.
 * whisper_amd_stream_open_vad: `vctx` is the caller's whisper_vad_context on the context's device; sessions share it read-only (it must outlive
 *   them; whisper_vad_detect_speech on it stays the caller's to use), each owns its LSTM state and probabilities.  The ring holds max_utterance +
 *   backlog samples, backlog = backlog_ms x 16, raised to 16000 x max_speech_duration_s + 8192: an open speech and a candidate behind it always
 *   fit.  Refused (NULL, an error log line, nothing made) for null arguments, what whisper_amd_audio_to_pcm refuses, speech_pad_ms outside
 *   [0, 100], max_utterance_ms outside (0, 30000], max_speech_duration_s above the cap (or below one window and its pads: the reference then
 *   drops the bound), negative durations, a vctx of another device.  whisper_amd_stream_open keeps refusing step_ms <= 0.
 * The calls above on a VAD session: _feed is the same single k_stream_push launch; with vad_on_feed = 1 it also runs the front end on the
 *   session's new whole windows (one k_stream_vad_front launch straight from the ring), the recurrence and the segmenter on the calling thread,
 *   and returns the utterances due.  FULL, with nothing changed, when the packet would overwrite an utterance that is due or still open, or a
 *   window not yet processed.  _flush processes the last partial window and closes an open speech.  _pending: the utterances due.  _step /
 *   _step_many run ONE due utterance per session - one k_stream_window gather (per group of 8), then whisper_full_with_state, alone or in the
 *   lock-step group, exactly as for windows; segment times are relative to the utterance.  _info: windows run counts utterances, take is 0,
 *   committed 1.  _window_copy / _prompt_copy: the last utterance's PCM and prompt.  _reset: a fresh session's state, LSTM included.
 * whisper_amd_stream_vad_poll_many: for servers that set vad_on_feed = 0: the new whole windows of all `ss` (VAD sessions of one context and
 *   one vctx; at most 64; MIXED otherwise) through ONE k_stream_vad_front launch per group of up to 8 sessions, then recurrences and segmenters
 *   on the calling thread.  Returns the utterances due in total.  Nothing is done for windows already processed.
 * whisper_amd_stream_utterance_info: out = { utterances run, the last one's start on the absolute 16 kHz axis, its length, its start_cs, its
 *   end_cs, whether it was split at the cap (0 / 1), front-end launches so far, windows processed so far }.
 * whisper_amd_stream_vad_probs_copy: the probabilities so far: copies up to `cap`, returns the full count.
 * WHISPER_AMD_STREAM_HOST=1 (or a HIP failure): the session stages its new windows linearly and uses the whole-recording front-end launch; the
 *   bits are the same. */
struct whisper_amd_stream_vad_params {
    int32_t sample_rate;        /* 16000 */
    int32_t channels;           /* 1     */
    int32_t format;             /* WHISPER_AMD_PCM_F32 */
    int32_t backlog_ms;         /* 40000 */
    int32_t carry_prompt;       /* 0     */
    int32_t max_utterance_ms;   /* 30000 */
    int32_t vad_on_feed;        /* 1     */
    struct whisper_vad_params vad;      /* whisper_vad_default_params() with max_speech_duration_s = 30 */
};
WHISPER_API void    whisper_amd_stream_vad_default_params(struct whisper_amd_stream_vad_params * p);
WHISPER_API struct whisper_amd_stream * whisper_amd_stream_open_vad(struct whisper_context * ctx, struct whisper_vad_context * vctx,
                                                                     const struct whisper_amd_stream_vad_params * p);
WHISPER_API int     whisper_amd_stream_vad_poll_many(struct whisper_amd_stream ** ss, int n);
WHISPER_API int     whisper_amd_stream_utterance_info(struct whisper_amd_stream * s, int64_t out[8]);
WHISPER_API int64_t whisper_amd_stream_vad_probs_copy(struct whisper_amd_stream * s, float * dst, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* WHISPER_AMD_H */

// wa_align.cpp - forced alignment: whisper_amd_align / whisper_amd_align_score / whisper_amd_align_stats of include/whisper_amd.h.
//
// The caller knows the text.  One teacher-forced decoder pass over [sot, lang, not, tokens..., eot] - wa_dtw_pass of wa_dtw.cpp, the pass
// whisper_full's DTW runs over its own result - with every text row flagged: wa_decode (st.align_pass) points the reference-order vocabulary
// product at a buffer of the state that holds all of them, and k_align_score (wa_align.hip) turns each row into a 24-byte record where it
// lies.  What comes back is n_rows x 24 bytes; the rows themselves (n_rows x n_vocab x 4 bytes, 46 MB for 223 tokens) never cross to the host
// and st.logits is not written.  The scores are taken on the raw logits (wa_align.h).
#include "wa_internal.h"
#include "wa_align.h"
#include "wa_dtw_host.h"

#include <cstring>

static size_t align_pad256(size_t n) { return (n + 255) / 256 * 256; }

void wa_align_free(whisper_state & st) {
    if (st.d_align_logits) { (void) hipFree(st.d_align_logits); st.d_align_logits = nullptr; st.align_logits_cap = 0; }
    if (st.d_align_io) { (void) hipFree(st.d_align_io); st.d_align_io = nullptr; st.d_align_io_cap = 0; }
    if (st.h_align_io) { (void) hipHostFree(st.h_align_io); st.h_align_io = nullptr; st.h_align_io_cap = 0; }
    for (int i = 0; i < 2; ++i) if (st.ev_align[i]) { (void) hipEventDestroy(st.ev_align[i]); st.ev_align[i] = nullptr; }
}

// [rows padded to 64][n_vocab] F32, grow-only (replaced only while the state's stream is idle: every caller has waited for its last pass)
static bool align_reserve_logits(whisper_state & st, int n_rows, int n_vocab) {
    return wa_dev_reserve(st.d_align_logits, st.align_logits_cap, (size_t) wa_pad(n_rows, 64) * n_vocab);
}

// k_align_score over n_rows rows of d_logits on the state's stream: targets up, records down, one stream synchronise
static bool align_score_device(whisper_state & st, const float * d_logits, long long ld, int n_rows, int n_vocab, const int32_t * target,
                               struct whisper_amd_align_score * out) {
    const size_t o_rec = align_pad256((size_t) n_rows * sizeof(int32_t)), need = o_rec + (size_t) n_rows * sizeof(struct whisper_amd_align_score);
    if (!wa_dev_reserve(st.d_align_io, st.d_align_io_cap, need)) return false;
    if (need > st.h_align_io_cap) {
        if (st.h_align_io) { (void) hipHostFree(st.h_align_io); st.h_align_io = nullptr; st.h_align_io_cap = 0; }
        if (!WA_HIP_OK(hipHostMalloc((void **) &st.h_align_io, need))) { st.h_align_io = nullptr; return false; }
        st.h_align_io_cap = need;
    }
    for (int i = 0; i < 2; ++i) if (!st.ev_align[i] && !WA_HIP_OK(hipEventCreate(&st.ev_align[i]))) { st.ev_align[i] = nullptr; return false; }
    hipStream_t s = st.stream;
    memcpy(st.h_align_io, target, (size_t) n_rows * sizeof(int32_t));
    auto * d_rec = (struct whisper_amd_align_score *) (st.d_align_io + o_rec);
    if (!WA_HIP_OK(hipMemcpyAsync(st.d_align_io, st.h_align_io, (size_t) n_rows * sizeof(int32_t), hipMemcpyHostToDevice, s))) return false;
    (void) hipEventRecord(st.ev_align[0], s);
    const bool launched = wa_align_score_launch(s, d_logits, ld, n_rows, n_vocab, (const int32_t *) st.d_align_io, d_rec);
    (void) hipEventRecord(st.ev_align[1], s);
    const bool copied = launched && WA_HIP_OK(hipMemcpyAsync(st.h_align_io + o_rec, d_rec, (size_t) n_rows * sizeof(struct whisper_amd_align_score), hipMemcpyDeviceToHost, s));
    if (!WA_HIP_OK(hipStreamSynchronize(s)) || !copied) return false;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, st.ev_align[0], st.ev_align[1]) == hipSuccess) st.t_align_kernel_us = (int64_t) (ms * 1000.0f + 0.5f);
    memcpy(out, st.h_align_io + o_rec, (size_t) n_rows * sizeof(struct whisper_amd_align_score));
    st.n_align_rows += n_rows;
    return true;
}

extern "C" int whisper_amd_align(struct whisper_context * ctx, struct whisper_state * st, struct whisper_full_params params, const float * samples,
                                 int n_samples, const whisper_token * tokens, int n_tokens, struct whisper_amd_align_token * out) {
    const int64_t t0 = wa_time_us();
    if (!ctx || !st || !samples || !tokens || !out || n_tokens <= 0 || n_samples <= 0) {
        WA_ERROR("%s: no tokens (n_tokens = %d), no audio or a null argument\n", __func__, n_tokens);
        return WHISPER_AMD_ALIGN_NO_TOKENS;
    }
    const auto & hp = ctx->model.hp;
    const auto & vocab = ctx->vocab;
    if (!ctx->exact) { WA_ERROR("%s: the context was created with flash_attn; only the exact path is scored\n", __func__); return WHISPER_AMD_ALIGN_FLASH_ATTN; }
    for (int i = 0; i < n_tokens; ++i)
        if (tokens[i] < 0 || tokens[i] >= vocab.token_eot) {
            WA_ERROR("%s: token %d at %d is not a text token (eot = %d)\n", __func__, tokens[i], i, vocab.token_eot);
            return WHISPER_AMD_ALIGN_BAD_TOKEN;
        }
    const int sot_len = vocab.is_multilingual() ? 2 : 1;
    const int n_seq = sot_len + 1 + n_tokens + 1, n_rows = n_tokens + 1;
    if (n_seq > std::min(st->dec_mpad, hp.n_text_ctx)) {
        WA_ERROR("%s: %d tokens make a sequence of %d, the decoder holds %d\n", __func__, n_tokens, n_seq, std::min(st->dec_mpad, hp.n_text_ctx));
        return WHISPER_AMD_ALIGN_TOO_LONG;
    }
    const int seek = params.offset_ms / 10;
    const int n_len_org = 1 + (n_samples + 200 - 400) / 160;                 // (wa_mel_compute)
    const int seek_end = params.duration_ms == 0 ? n_len_org : std::min(n_len_org, seek + params.duration_ms / 10);
    if (seek < 0 || seek_end < seek + 10) {
        WA_ERROR("%s: %d ms of audio after the offset, at least 100 ms are needed\n", __func__, (seek_end - seek) * 10);
        return WHISPER_AMD_ALIGN_TOO_SHORT;
    }
    if (params.audio_ctx > hp.n_audio_ctx) { WA_ERROR("%s: audio_ctx is larger than the maximum allowed (%d > %d)\n", __func__, params.audio_ctx, hp.n_audio_ctx); return -5; }
    if (ctx->model.n_loaded == 0) { WA_ERROR("%s: the model has no weights\n", __func__); return -8; }
    if (!WA_HIP_OK(hipSetDevice(ctx->device))) return -8;

    if (!wa_mel_compute(*ctx, *st, samples, n_samples)) { WA_ERROR("%s: failed to compute log mel spectrogram\n", __func__); return -2; }
    std::vector<whisper_token> seq = { vocab.token_sot };
    if (vocab.is_multilingual()) {
        int lang_id;
        if (params.language == nullptr || strlen(params.language) == 0 || strcmp(params.language, "auto") == 0) {       // as whisper_full detects it
            lang_id = whisper_lang_auto_detect_with_state(ctx, st, 0, params.n_threads, nullptr);
            if (lang_id < 0) { WA_ERROR("%s: failed to auto-detect language\n", __func__); wa_kv_clear(st->kv_self); return -3; }
        } else {
            lang_id = whisper_lang_id(params.language);
            if (lang_id < 0) { WA_ERROR("%s: unknown language '%s'\n", __func__, params.language); return -3; }
        }
        st->lang_id = lang_id;
        seq.push_back(vocab.token_sot + 1 + lang_id);
    }
    seq.push_back(vocab.token_not);
    seq.insert(seq.end(), tokens, tokens + n_tokens);
    seq.push_back(vocab.token_eot);

    st->exp_n_audio_ctx = params.audio_ctx;
    if (!wa_encode(*ctx, *st, seek, params.abort_callback, params.abort_callback_user_data)) { WA_ERROR("%s: failed to encode\n", __func__); return -6; }
    if (!align_reserve_logits(*st, n_rows, hp.n_vocab)) return -8;

    // the pass: rows sot_len .. n_seq - 2 flagged, row i scored against token i + 1; the alignment heads captured where the context has some
    const int n_frames = std::min(WHISPER_CHUNK_SIZE * 100, seek_end - seek);
    wa_dtw_path_t path;
    int64_t t_pass_end = 0;
    st->align_pass = true;
    const int have = wa_dtw_pass(ctx, st, seq, sot_len, n_frames, 7, true, path, t_pass_end);
    st->align_pass = false;
    wa_kv_clear(st->kv_self);                            // whisper_full afterwards finds the cells of a fresh state
    if (have < 0) { WA_ERROR("%s: failed to decode\n", __func__); return -8; }

    std::vector<struct whisper_amd_align_score> rec(n_rows);
    if (!align_score_device(*st, st->d_align_logits, hp.n_vocab, n_rows, hp.n_vocab, seq.data() + sot_len + 1, rec.data())) {
        WA_ERROR("%s: failed to score the logits rows\n", __func__);
        return -8;
    }
    for (int i = 0; i < n_rows; ++i) {
        struct whisper_amd_align_token o;
        o.id = seq[sot_len + 1 + i]; o.plog = rec[i].plog; o.p = rec[i].p; o.best_id = rec[i].best_id; o.best_plog = rec[i].best_plog; o.rank = rec[i].rank;
        o.t_dtw = -1;
        out[i] = o;
    }
    if (have == 1) {
        // whisper_full's placement (wa_dtw_timestamps; whisper.cpp:8894-8920): path row 0 is `not`, row v the v-th text token; the first time
        // index of each row
        int32_t last_v = 0;
        int at = 0;
        for (const auto & pr : path) {
            if (pr.first == last_v) continue;
            last_v = pr.first;
            if (at >= n_tokens) break;
            out[at++].t_dtw = (int64_t) pr.second * 2 + seek;
        }
    }
    st->n_align_calls += 1;
    st->align_bytes_kept += (long long) n_rows * hp.n_vocab * (long long) sizeof(float);
    st->t_align_call_us = wa_time_us() - t0;
    return 0;
}

extern "C" int whisper_amd_align_score(struct whisper_state * st, const float * logits, int n_rows, int n_vocab, const int32_t * target, int where,
                                       struct whisper_amd_align_score * out) {
    bool ok = st && logits && target && out && n_rows > 0 && n_vocab > 0 && (where == 0 || where == 1);
    for (int r = 0; ok && r < n_rows; ++r) ok = target[r] >= 0 && target[r] < n_vocab;
    if (!ok) { WA_ERROR("%s: refused arguments\n", __func__); return WHISPER_AMD_ALIGN_NO_TOKENS; }
    if (where == 0) { wa_align_score_host(logits, n_vocab, n_rows, n_vocab, target, out); return 0; }
    if (!st->ctx || !WA_HIP_OK(hipSetDevice(st->ctx->device))) return -8;
    // the rows take the alignment pass's place; launcher, buffers and stream are the product path's
    if (!align_reserve_logits(*st, n_rows, n_vocab)) return -8;
    if (!WA_HIP_OK(hipMemcpyAsync(st->d_align_logits, logits, (size_t) n_rows * n_vocab * sizeof(float), hipMemcpyHostToDevice, st->stream))) return -8;
    std::vector<struct whisper_amd_align_score> rec(n_rows);
    if (!align_score_device(*st, st->d_align_logits, n_vocab, n_rows, n_vocab, target, rec.data())) return -8;
    memcpy(out, rec.data(), (size_t) n_rows * sizeof(struct whisper_amd_align_score));
    return 0;
}

extern "C" void whisper_amd_align_stats(struct whisper_state * st, long out[3]) {
    out[0] = st->n_align_calls; out[1] = st->n_align_rows; out[2] = (long) st->align_bytes_kept;
}
extern "C" void whisper_amd_align_timings(struct whisper_state * st, int64_t out[2]) { out[0] = st->t_align_kernel_us; out[1] = st->t_align_call_us; }

// wa_dtw.cpp - DTW token-level timestamps (BASELINE config 4).
//
// ref: whisper_exp_compute_token_level_timestamps_dtw whisper.cpp:8772-8933, dtw_and_backtrace 8647-8731,
// median_filter 8737-8770, alignment-head selection 1190-1303, QK capture in the decoder graph 2737-2752 / 2838-2845.
//
// One extra decoder pass over [sot, lang, not, text..., eot] whose cross-attention kernels also write their F32 soft-max probabilities
// (k_attn_exact's qk_out) into the state's capture buffer [layer slot][token][head][n_audio_ctx].  The rest - normalise over tokens, 7-wide
// median over audio, mean over heads, DTW table - runs on the device too (wa_dtw.hip), on the state's stream, reading the alignment heads in
// place through a table of (slot, head) offsets; the trace (one byte per cell) comes back to a pinned buffer and the backtrace runs here.
// A device call that fits the state's grow-only buffers allocates nothing, issues nothing on the null stream and waits for the stream once.
// The same arithmetic on the host (wa_dtw_host.cpp, the reference's order: F64 sums of ggml_norm / ggml_mean) serves every other shape, any
// HIP error on the way, and WHISPER_AMD_DTW_HOST=1 (read when the state is created).
#include "wa_internal.h"
#include "wa_dtw_host.h"
#include "wa_kernels.h"

#include <cstring>

static size_t dtw_pad256(size_t n) { return (n + 255) / 256 * 256; }

// the capture buffer, grow-only (a larger one replaces it only while the state's stream is idle: every caller has waited for its last pass)
static bool dtw_reserve_capture(whisper_state & st, size_t n_floats) {
    if (n_floats <= st.aheads_qk_cap && st.d_aheads_qk) return true;
    if (st.d_aheads_qk) { (void) hipFree(st.d_aheads_qk); st.d_aheads_qk = nullptr; st.aheads_qk_cap = 0; }
    if (!WA_HIP_OK(hipMalloc((void **) &st.d_aheads_qk, n_floats * sizeof(float)))) { st.d_aheads_qk = nullptr; return false; }
    st.aheads_qk_cap = n_floats;
    return true;
}

static bool dtw_device_takes(const whisper_state & st, int n_tokens, int M, int sot_len, int medfilt_width) {
    const int N = n_tokens - sot_len - 1;
    return medfilt_width == 7 && M > 7 && N > 0 && N <= WA_DTW_MAX_N && n_tokens <= st.dec_mpad;
}

// The device path on x(k, t, j) = d_x[head_off[k] + t * tok_stride + j]: the path length, or WA_DTW_HIP_ERROR.  One stream synchronise.
static int dtw_device_path(whisper_state & st, const float * d_x, const long long * head_off, long long tok_stride, int n_heads, int n_tokens, int M,
                           int sot_len, wa_dtw_path_t & path) {
    const int N = n_tokens - sot_len - 1;
    const size_t nd = (size_t) N + M - 1;
    const size_t o_mean = dtw_pad256((size_t) n_heads * sizeof(long long)), o_scale = o_mean + dtw_pad256((size_t) n_heads * M * sizeof(float)),
                 o_cost = o_scale + dtw_pad256((size_t) n_heads * M * sizeof(float)), o_trace = o_cost + dtw_pad256(nd * N * sizeof(float)),
                 d_need = o_trace + dtw_pad256(nd * N), h_need = o_mean + dtw_pad256(nd * N);
    if (d_need > st.d_dtw_cap) {
        if (st.d_dtw) { (void) hipFree(st.d_dtw); st.d_dtw = nullptr; st.d_dtw_cap = 0; }
        if (!WA_HIP_OK(hipMalloc((void **) &st.d_dtw, d_need))) { st.d_dtw = nullptr; return WA_DTW_HIP_ERROR; }
        st.d_dtw_cap = d_need;
    }
    if (h_need > st.h_dtw_cap) {
        if (st.h_dtw) { (void) hipHostFree(st.h_dtw); st.h_dtw = nullptr; st.h_dtw_cap = 0; }
        if (!WA_HIP_OK(hipHostMalloc((void **) &st.h_dtw, h_need))) { st.h_dtw = nullptr; return WA_DTW_HIP_ERROR; }
        st.h_dtw_cap = h_need;
    }
    hipStream_t s = st.stream;
    memcpy(st.h_dtw, head_off, (size_t) n_heads * sizeof(long long));
    uint8_t * h_trace = st.h_dtw + o_mean, * d_trace = st.d_dtw + o_trace;
    if (!WA_HIP_OK(hipMemcpyAsync(st.d_dtw, st.h_dtw, (size_t) n_heads * sizeof(long long), hipMemcpyHostToDevice, s))) return WA_DTW_HIP_ERROR;
    wa_launch_dtw(s, d_x, (const long long *) st.d_dtw, tok_stride, n_heads, n_tokens, sot_len, M, (float *) (st.d_dtw + o_mean), (float *) (st.d_dtw + o_scale),
                  (float *) (st.d_dtw + o_cost), d_trace);
    const bool launched = WA_HIP_OK(hipGetLastError());
    const bool copied = launched && WA_HIP_OK(hipMemcpyAsync(h_trace, d_trace, nd * N, hipMemcpyDeviceToHost, s));
    if (!WA_HIP_OK(hipStreamSynchronize(s)) || !copied) return WA_DTW_HIP_ERROR;
    // cell (i, j) of the table at [(i - 1 + j - 1) * N + (i - 1)]
    wa_dtw_backtrace(h_trace, (long long) N + 1, (long long) N, N, M, path);
    return (int) path.size();
}

int wa_dtw_pass(whisper_context * ctx, whisper_state * st, const std::vector<whisper_token> & tokens, int sot_len_, int n_frames, int medfilt_width,
                bool score_rows, wa_dtw_path_t & path, int64_t & t_pass_end) {
    const auto & hp = ctx->model.hp;
    const int n_audio_ctx = st->exp_n_audio_ctx > 0 ? st->exp_n_audio_ctx : hp.n_audio_ctx;
    const int H = hp.n_text_head;
    const bool want_dtw = !(st->aheads_n <= 0 || n_frames > 2 * n_audio_ctx || medfilt_width % 2 == 0);
    if (!want_dtw && !score_rows) return -1;
    if (!WA_HIP_OK(hipSetDevice(ctx->device))) return -1;
    const size_t sot_len = (size_t) sot_len_;
    const int n_tokens = (int) tokens.size();
    if (n_tokens > st->dec_mpad) { WA_WARN("%s: too many tokens for DTW (%d)\n", __func__, n_tokens); return -1; }

    // capture buffer: [layer slot][token][head][n_audio_ctx] F32 for the layers that own alignment heads; sized for a multiple of 64 tokens
    // so that a longer window seldom replaces it
    std::vector<int> slot(hp.n_text_layer, -1);
    int n_slots = 0;
    if (want_dtw) for (int il = 0; il < hp.n_text_layer; ++il) if (!st->aheads[il].empty()) slot[il] = n_slots++;
    const size_t per_layer = (size_t) n_tokens * H * n_audio_ctx;
    if (want_dtw && !dtw_reserve_capture(*st, (size_t) std::min(st->dec_mpad, wa_pad(n_tokens, 64)) * H * n_audio_ctx * n_slots)) return -1;

    // the decoder pass (whisper.cpp:8823-8829)
    wa_kv_clear(st->kv_self);
    auto & b = st->batch;
    b.n_tokens = n_tokens;
    b.token.assign(tokens.begin(), tokens.end());
    b.pos.resize(n_tokens); b.seq_id.assign(n_tokens, 0); b.logits.assign(n_tokens, 0);
    for (int i = 0; i < n_tokens; ++i) b.pos[i] = i;
    if (score_rows) for (int i = sot_len_; i < n_tokens - 1; ++i) b.logits[i] = 1;      // row i predicts token i + 1
    else b.logits[n_tokens - 1] = 1;
    wa_kv_seq_rm(st->kv_self, 0, 0, -1);
    // wa_decode indexes the capture buffer by layer; give it a slot table through aheads_slot
    if (want_dtw) st->aheads_slot = slot;
    const bool ok = wa_decode(*ctx, *st, b, want_dtw, nullptr, nullptr);
    if (!ok) { WA_ERROR("%s: decoder pass failed\n", __func__); return -1; }
    t_pass_end = wa_time_us();
    if (!want_dtw) return 0;

    // the alignment heads in the capture buffer, head k at (slot, head): x(k, t, j) = d_aheads_qk[head_off[k] + t * H * n_audio_ctx + j]
    const int n_heads = st->aheads_n;
    const int n_audio_tokens = n_frames / 2;
    if (n_audio_tokens <= 0) return 0;
    std::vector<long long> head_off;
    for (int il = 0; il < hp.n_text_layer; ++il)
        for (int h : st->aheads[il]) head_off.push_back((long long) ((size_t) slot[il] * per_layer + (size_t) h * n_audio_ctx));
    const long long tok_stride = (long long) H * n_audio_ctx;
    if (medfilt_width >= n_audio_tokens) { WA_WARN("%s: too few audio frames for the median filter\n", __func__); return 0; }
    if (!wa_dtw_args_ok(n_heads, n_tokens, n_audio_ctx, n_audio_tokens, (int) sot_len, medfilt_width)) return 0;      // (N <= 0)

    bool served = false;
    if (!st->dtw_host && dtw_device_takes(*st, n_tokens, n_audio_tokens, (int) sot_len, medfilt_width)) {
        served = dtw_device_path(*st, st->d_aheads_qk, head_off.data(), tok_stride, n_heads, n_tokens, n_audio_tokens, (int) sot_len, path) >= 0;
        if (served) st->n_dtw_device++; else { st->n_dtw_fallback++; WA_WARN("%s: the device path failed, taking the host path\n", __func__); }
    }
    if (!served) {
        // copy back the alignment heads only, the frames in use: cube[k][t][j]
        const int M_ = n_audio_tokens;
        std::vector<float> cube((size_t) n_heads * n_tokens * M_);
        std::vector<long long> off_h(n_heads);
        for (int k = 0; k < n_heads; ++k) {
            off_h[k] = (long long) k * n_tokens * M_;
            if (!WA_HIP_OK(hipMemcpy2D(cube.data() + off_h[k], (size_t) M_ * sizeof(float), st->d_aheads_qk + head_off[k], (size_t) tok_stride * sizeof(float),
                                       (size_t) M_ * sizeof(float), n_tokens, hipMemcpyDeviceToHost))) return 0;
        }
        const wa_dtw_view v = { cube.data(), off_h.data(), n_heads, (long long) M_, n_tokens, M_ };
        if (wa_dtw_host_path(v, M_, (int) sot_len, medfilt_width, path) < 0) return 0;
        st->n_dtw_host++;
    }
    return 1;
}

void wa_dtw_timestamps(whisper_context * ctx, whisper_state * st, const whisper_full_params & params, int i_segment, size_t n_segments,
                       int seek, int n_frames, int medfilt_width) {
    const auto & hp = ctx->model.hp;
    const auto & vocab = ctx->vocab;
    const int n_audio_ctx = st->exp_n_audio_ctx > 0 ? st->exp_n_audio_ctx : hp.n_audio_ctx;
    if (st->aheads_n <= 0 || n_frames > 2 * n_audio_ctx || medfilt_width % 2 == 0) return;
    if (!WA_HIP_OK(hipSetDevice(ctx->device))) return;

    // sot + [lang] + not + text tokens of the new segments + eot   (whisper.cpp:8800-8817)
    std::vector<whisper_token> tokens = { vocab.token_sot };
    if (vocab.is_multilingual()) {
        const int lang_id = whisper_lang_id(params.language);
        st->lang_id = lang_id;
        tokens.push_back(vocab.token_sot + 1 + lang_id);
    }
    const size_t sot_len = tokens.size();
    tokens.push_back(vocab.token_not);
    for (size_t i = i_segment; i < i_segment + n_segments; ++i)
        for (const auto & t : st->result_all[i].tokens) if (t.id < vocab.token_eot) tokens.push_back(t.id);
    tokens.push_back(vocab.token_eot);

    wa_dtw_path_t path;                                   // (token index, time index)
    int64_t t_post = 0;
    if (wa_dtw_pass(ctx, st, tokens, (int) sot_len, n_frames, medfilt_width, false, path, t_post) != 1) return;

    // place the timestamps on the text tokens of the new segments (whisper.cpp:8894-8920)
    int32_t last_v = 0;
    size_t seg_i = i_segment;
    const size_t seg_end = i_segment + n_segments;
    size_t tok_i = 0;
    auto advance_to_text = [&]() -> bool {
        while (seg_i < seg_end) {
            auto & toks = st->result_all[seg_i].tokens;
            while (tok_i < toks.size() && !(toks[tok_i].id < vocab.token_eot)) ++tok_i;
            if (tok_i < toks.size()) return true;
            ++seg_i; tok_i = 0;
        }
        return false;
    };
    for (const auto & pr : path) {
        const int32_t v = pr.first;
        if (v != last_v) {
            const int64_t timestamp = (int64_t) pr.second * 2 + seek;      // one DTW index = 20 ms
            last_v = v;
            if (!advance_to_text()) break;
            st->result_all[seg_i].tokens[tok_i].t_dtw = timestamp;
            ++tok_i;
        }
    }
    st->t_dtw_post_us += wa_time_us() - t_post; st->n_dtw_post++;
}

// ---- the alignment alone (include/whisper_amd.h) ----
int whisper_amd_dtw_path(struct whisper_state * st, const float * qk, int n_heads, int n_tokens, int n_ctx, int n_audio_tokens, int sot_len,
                         int medfilt_width, int where, int32_t * path_tok, int32_t * path_time, int cap) {
    if (!st || !qk || (where != 0 && where != 1)) return WA_DTW_REFUSED;
    if (!wa_dtw_args_ok(n_heads, n_tokens, n_ctx, n_audio_tokens, sot_len, medfilt_width)) return WA_DTW_REFUSED;
    std::vector<long long> head_off(n_heads);
    for (int k = 0; k < n_heads; ++k) head_off[k] = (long long) k * n_tokens * n_ctx;
    wa_dtw_path_t path;
    int n;
    if (where == 0) {
        const wa_dtw_view v = { qk, head_off.data(), n_heads, (long long) n_ctx, n_tokens, n_ctx };
        n = wa_dtw_host_path(v, n_audio_tokens, sot_len, medfilt_width, path);
        if (n >= 0) st->n_dtw_host++;
    } else {
        if (!dtw_device_takes(*st, n_tokens, n_audio_tokens, sot_len, medfilt_width)) return WA_DTW_NOT_TAKEN;
        if (!st->ctx || !WA_HIP_OK(hipSetDevice(st->ctx->device))) return WA_DTW_HIP_ERROR;
        // the cube takes the capture buffer's place; the launchers are the product path's
        const size_t n_cube = (size_t) n_heads * n_tokens * n_ctx;
        if (!dtw_reserve_capture(*st, n_cube)) return WA_DTW_HIP_ERROR;
        if (!WA_HIP_OK(hipMemcpyAsync(st->d_aheads_qk, qk, n_cube * sizeof(float), hipMemcpyHostToDevice, st->stream))) return WA_DTW_HIP_ERROR;
        n = dtw_device_path(*st, st->d_aheads_qk, head_off.data(), (long long) n_ctx, n_heads, n_tokens, n_audio_tokens, sot_len, path);
        if (n >= 0) st->n_dtw_device++; else st->n_dtw_fallback++;
    }
    if (n < 0) return n;
    for (int i = 0; i < n && i < cap; ++i) {
        if (path_tok)  path_tok[i]  = path[i].first;
        if (path_time) path_time[i] = path[i].second;
    }
    return n;
}

void whisper_amd_dtw_stats(struct whisper_state * st, long out[3]) { out[0] = st->n_dtw_device; out[1] = st->n_dtw_host; out[2] = st->n_dtw_fallback; }
void whisper_amd_dtw_timings(struct whisper_state * st, int64_t out[2]) { out[0] = st->t_dtw_post_us; out[1] = st->n_dtw_post; }

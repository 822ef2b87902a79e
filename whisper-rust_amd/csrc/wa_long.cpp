// wa_long.cpp - long recordings: the whisper_amd_full_long / whisper_amd_long_* entry points of include/whisper_amd.h.
//
// A recording of any length is cut at the silences the VAD found (wa_long_plan.h: chunks of whole segments, at most max_chunk_ms of
// speech-only audio each), every chunk's speech-only audio is written by ONE launch of k_long_pack (wa_long.hip) into a buffer of the
// context's state, and the chunks run in waves of n_parallel through wa_wave_run (wa_wave.h), as whisper_amd_full_batch's do: a chunk is
// whisper_full_with_state on its audio, nothing else.  The PCM crosses PCIe once (host input) or never (device input): the VAD reads it in
// place (wa_vad.cpp), the pack kernel reads it in place, the members read the packed chunks in place.  VAD and pack have completed - a
// stream synchronise - before the first wave starts: a foreign kernel beside the one-launch passes costs hand-off time-outs.
// wa_vad_filter_audio, the host function, is the yardstick and the fallback: WHISPER_AMD_LONG_HOST=1, read at each call, takes it, and so
// does a call whose HIP path fails (logged and counted).
#include "wa_long_host.h"
#include "wa_wave.h"

#include <climits>
#include <cstring>

wa_long_state & wa_long_of(whisper_state & st) {
    if (!st.lng) st.lng = new wa_long_state;
    return *st.lng;
}

void wa_long_free(whisper_state & st) {
    if (!st.lng) return;
    if (st.ctx) (void) hipSetDevice(st.ctx->device);
    if (st.stream) (void) hipStreamSynchronize(st.stream);
    if (st.lng->d_pcm) (void) hipFree(st.lng->d_pcm);
    if (st.lng->d_chunks) (void) hipFree(st.lng->d_chunks);
    if (st.lng->d_pieces) (void) hipFree(st.lng->d_pieces);
    delete st.lng;
    st.lng = nullptr;
}

// host PCM into the state's buffer, once
static const float * long_upload(whisper_state & st, const float * h_samples, int n_samples) {
    wa_long_state & L = wa_long_of(st);
    if (!wa_dev_reserve(L.d_pcm, L.d_pcm_cap, (size_t) std::max(n_samples, WA_LONG_ALIGN))) return nullptr;
    if (!WA_HIP_OK(hipMemcpyAsync(L.d_pcm, h_samples, (size_t) n_samples * sizeof(float), hipMemcpyHostToDevice, st.stream)) ||
        !WA_HIP_OK(hipStreamSynchronize(st.stream))) return nullptr;
    L.stats[7] += (int64_t) n_samples * (int64_t) sizeof(float);
    return L.d_pcm;
}

bool wa_long_pack(whisper_state & st, const float * h_samples, const float * d_samples, const std::vector<wa_long_src> & srcs,
                  const std::vector<wa_long_pick> & order, float samples_overlap, int where) {
    wa_long_state & L = wa_long_of(st);
    L.chunks.clear();
    if (srcs.empty() || (h_samples && (srcs.size() != 1 || srcs[0].src_off != 0))) return false;
    std::vector<wa_long_piece> all, pieces;
    std::vector<int> src_of;
    int64_t off = 0;
    for (const wa_long_pick & pk : order) {
        if (pk.src < 0 || (size_t) pk.src >= srcs.size() || pk.chunk < 0 || (size_t) pk.chunk >= srcs[(size_t) pk.src].plan->size()) return false;
        const wa_long_src & S = srcs[(size_t) pk.src];
        const wa_long_chunk & c = (*S.plan)[(size_t) pk.chunk];
        wa_long_rec r;
        r.first = c.first; r.count = c.count; r.off = off; r.channel = S.channel;
        r.packed = wa_vad_layout_make(S.segs + c.first, c.count, samples_overlap, S.n_samples, &pieces, &r.table);
        r.t0 = S.segs[c.first].start; r.t1 = S.segs[c.first + c.count - 1].end;
        int64_t cur = off;
        for (const wa_long_piece & p : pieces) {        // contiguous from the chunk's start; the kernel trusts what is checked here
            if (p.dst + off != cur || p.len <= 0 || p.src < -1 || (p.src >= 0 && p.src + p.len > (int64_t) S.n_samples) || cur + p.len > off + r.packed) return false;
            all.push_back({ cur, p.src >= 0 ? p.src + S.src_off : -1, p.len });
            cur += p.len;
        }
        const int64_t next = (off + r.packed + WA_LONG_ALIGN - 1) / WA_LONG_ALIGN * WA_LONG_ALIGN;
        if (next > cur) all.push_back({ cur, -1, next - cur });     // what no piece covers is zero; so is the gap in front of the next chunk
        off = next;
        L.chunks.push_back(std::move(r));
        src_of.push_back(pk.src);
    }
    const int64_t n_out = off;
    if (all.size() > (size_t) INT_MAX) return false;
    if (!wa_dev_reserve(L.d_chunks, L.d_chunks_cap, (size_t) std::max<int64_t>(n_out, WA_LONG_ALIGN))) return false;
    L.stats[0] = where;
    if (n_out == 0) return true;
    if (where == 1) {
        const float * src = d_samples ? d_samples : long_upload(st, h_samples, srcs[0].n_samples);
        if (!src) return false;
        if (!(wa_dev_reserve(L.d_pieces, L.d_pieces_cap, all.size())
            && WA_HIP_OK(hipMemcpyAsync(L.d_pieces, all.data(), all.size() * sizeof(wa_long_piece), hipMemcpyHostToDevice, st.stream))
            && wa_long_pack_launch((void *) st.stream, src, L.d_pieces, (int) all.size(), n_out, L.d_chunks))) return false;
        L.n_pack_launches++;
        return WA_HIP_OK(hipStreamSynchronize(st.stream));
    }
    std::vector<std::vector<float>> down(srcs.size());
    std::vector<const float *> host(srcs.size(), h_samples);
    if (!h_samples) {
        if (!WA_HIP_OK(hipStreamSynchronize(st.stream))) return false;
        for (size_t k = 0; k < srcs.size(); ++k) {
            down[k].resize((size_t) srcs[k].n_samples);
            if (!WA_HIP_OK(hipMemcpy(down[k].data(), d_samples + srcs[k].src_off, down[k].size() * sizeof(float), hipMemcpyDeviceToHost))) return false;
            host[k] = down[k].data();
        }
    }
    std::vector<float> img((size_t) n_out, 0.0f), filtered;
    std::vector<wa_vad_map_point> table;
    for (size_t c = 0; c < L.chunks.size(); ++c) {
        const wa_long_rec & r = L.chunks[c];
        const wa_long_src & S = srcs[(size_t) src_of[c]];
        const std::vector<wa_vad_seg> sub(S.segs + r.first, S.segs + r.first + r.count);
        wa_vad_filter_audio(sub, samples_overlap, host[(size_t) src_of[c]], S.n_samples, filtered, table);
        if ((int) filtered.size() != r.packed) return false;
        if (r.packed > 0) memcpy(img.data() + r.off, filtered.data(), (size_t) r.packed * sizeof(float));
    }
    return WA_HIP_OK(hipMemcpyAsync(L.d_chunks, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, st.stream))
        && WA_HIP_OK(hipStreamSynchronize(st.stream));
}

bool wa_long_pack_any(whisper_state & st, const float * h_samples, const float * d_samples, const std::vector<wa_long_src> & srcs,
                      const std::vector<wa_long_pick> & order, float samples_overlap, const char * who) {
    wa_long_state & L = wa_long_of(st);
    const char * env = getenv("WHISPER_AMD_LONG_HOST");
    bool packed = false;
    if (!(env && atoi(env) != 0)) {
        packed = wa_long_pack(st, h_samples, d_samples, srcs, order, samples_overlap, 1);
        if (!packed) { L.stats[1]++; (void) hipGetLastError(); WA_WARN("%s: the device pack failed, taking the host path\n", who); }
    }
    if (!packed && !wa_long_pack(st, h_samples, d_samples, srcs, order, samples_overlap, 0)) {
        WA_ERROR("%s: the host pack failed\n", who);
        L.chunks.clear();
        return false;
    }
    return true;
}

// one segment list over one buffer, every chunk of its plan in order
static void single_source(const wa_vad_seg * segs, int n_samples, const std::vector<wa_long_chunk> & plan, std::vector<wa_long_src> & srcs,
                          std::vector<wa_long_pick> & order) {
    srcs = { { segs, n_samples, 0, -1, &plan } };
    order.clear();
    for (size_t c = 0; c < plan.size(); ++c) order.push_back({ 0, (int) c });
}

static std::vector<wa_vad_seg> long_segs(const int64_t * segs_cs, int n_segs) {
    std::vector<wa_vad_seg> segs((size_t) std::max(n_segs, 0));
    for (int i = 0; i < n_segs; ++i) { segs[i].start = segs_cs[2 * i]; segs[i].end = segs_cs[2 * i + 1]; }
    return segs;
}

// the waves (wa_wave.h): chunks [c0, c0 + members) of the list, chunk c0 + i on states[i], in lock step where a group forms
int wa_long_waves(whisper_context * ctx, const whisper_full_params & params, int n_parallel, std::vector<std::vector<wa_segment>> & results) {
    whisper_state * st = ctx->state;
    wa_long_state & L = wa_long_of(*st);
    const int64_t t = wa_time_us();
    const size_t n_chunks = L.chunks.size();
    std::vector<whisper_state *> states = { st };         // the context's state and, as whisper_full_parallel, states of this call
    auto release = [&]() { for (size_t i = 1; i < states.size(); ++i) whisper_free_state(states[i]); states.resize(1); };
    for (size_t i = 1; i < std::min(n_chunks, (size_t) n_parallel); ++i) {
        whisper_state * s = whisper_init_state(ctx);
        if (!s) { release(); L.chunks.clear(); return -1; }
        states.push_back(s);
    }
    whisper_full_params pc = params;
    wa_params_silent(pc);
    pc.vad = false; pc.offset_ms = 0; pc.duration_ms = 0;
    pc.print_timestamps = false; pc.print_special = false;      // print_special: no special tokens in a chunk's text (wa_full.cpp)

    std::vector<int> rcs;
    results.assign(n_chunks, std::vector<wa_segment>());
    wa_wave_totals totals;
    int lang_id = st->lang_id;
    for (size_t c0 = 0; c0 < n_chunks; c0 += states.size()) {
        const std::vector<whisper_state *> members(states.begin(), states.begin() + std::min(states.size(), n_chunks - c0));
        const std::vector<int> wave = wa_wave_run(ctx, members, [&](size_t i) {
            const wa_long_rec & r = L.chunks[c0 + i];
            // chunks are independent: nothing of the state's earlier text - an earlier call's on the context's state, the previous wave's chunk on
            // any member - prompts this one, whatever no_context says; inside the chunk whisper_full's windows carry their context as they always do
            members[i]->prompt_past.clear();
            if (r.packed > 0) return whisper_full_with_state(ctx, members[i], pc, L.d_chunks + r.off, r.packed);
            members[i]->result_all.clear();         // every segment clamped away: no audio, no result
            return 0;
        });
        rcs.insert(rcs.end(), wave.begin(), wave.end());
        totals.add(ctx);
        for (size_t i = 0; i < members.size(); ++i) { results[c0 + i] = std::move(members[i]->result_all); members[i]->result_all.clear(); }
        if (c0 == 0) lang_id = st->lang_id;
        L.stats[3]++;
    }
    totals.publish(ctx);
    for (size_t i = 1; i < states.size(); ++i) wa_state_add_counters(*st, *states[i]);
    release();
    st->lang_id = lang_id;
    st->vad_mapping_table.clear();                  // the times are stored mapped: the getters return them as they are
    st->has_vad_segments = false;
    L.stats[6] = wa_time_us() - t;                  // states and waves; a caller that maps the times afterwards sets it again, mapping included
    for (int rc : rcs) if (rc != 0) { L.chunks.clear(); return rc; }       // a failed call describes no chunks
    return 0;
}

void wa_long_map_segment(wa_segment & seg, const std::vector<wa_vad_map_point> & table) {
    const int64_t t0 = wa_vad_map_time(seg.t0, table);
    int64_t t1 = wa_vad_map_time(seg.t1, table);
    if (t1 - t0 < 10) t1 = t0 + 10;
    seg.t0 = t0;
    seg.t1 = t1;
    for (whisper_token_data & tok : seg.tokens) {
        if (tok.t0 >= 0) tok.t0 = wa_vad_map_time(tok.t0, table);
        if (tok.t1 >= 0) tok.t1 = wa_vad_map_time(tok.t1, table);
        if (tok.t_dtw >= 0) tok.t_dtw = wa_vad_map_time(tok.t_dtw, table);
    }
}

static int long_full(whisper_context * ctx, whisper_full_params params, const float * samples, int n_samples, int max_chunk_ms, int n_parallel) {
    whisper_state * st = ctx->state;
    wa_long_state & L = wa_long_of(*st);
    st->result_all.clear();
    L.chunks.clear();
    L.seg_channel.clear();
    for (int k : { 0, 2, 3, 4, 5, 6, 7 }) L.stats[k] = 0;
    if (max_chunk_ms <= 0) max_chunk_ms = 30000;
    if (n_parallel <= 0) n_parallel = 8;
    n_parallel = std::min(n_parallel, WA_MAX_DECODERS);
    const int max_chunk_samples = (int) std::min<int64_t>((int64_t) max_chunk_ms * (WHISPER_SAMPLE_RATE / 1000), INT_MAX);
    if (!WA_HIP_OK(hipSetDevice(ctx->device))) return -1;

    // the audio in HBM: the caller's own buffer, or one upload (work of the caller's on another stream is the caller's to order)
    const bool on_device = wa_is_device_ptr(samples);
    if (on_device && !WA_HIP_OK(hipStreamSynchronize(st->stream))) return -1;
    const float * d_samples = on_device ? samples : long_upload(*st, samples, n_samples);
    if (!d_samples) { WA_ERROR("%s: failed to copy the audio to the device\n", __func__); return -1; }

    int64_t t = wa_time_us();
    std::vector<wa_vad_seg> segs;
    if (!wa_vad_segments_for(ctx, st, params, d_samples, n_samples, segs)) { WA_ERROR("%s: failed to compute VAD\n", __func__); return -1; }
    L.stats[4] = wa_time_us() - t;
    if (segs.empty()) return 0;

    t = wa_time_us();
    const std::vector<wa_long_chunk> plan = wa_long_plan(segs.data(), (int) segs.size(), n_samples, params.vad_params.samples_overlap, max_chunk_samples);
    std::vector<wa_long_src> srcs;
    std::vector<wa_long_pick> order;
    single_source(segs.data(), n_samples, plan, srcs, order);
    if (!wa_long_pack_any(*st, on_device ? nullptr : samples, d_samples, srcs, order, params.vad_params.samples_overlap, __func__)) return -1;
    L.stats[5] = wa_time_us() - t;
    L.stats[2] = (int64_t) L.chunks.size();
    WA_INFO("%s: %d speech segments in %d chunks of at most %d ms\n", __func__, (int) segs.size(), (int) L.chunks.size(), max_chunk_ms);

    t = wa_time_us();
    std::vector<std::vector<wa_segment>> results;
    const int rc = wa_long_waves(ctx, params, n_parallel, results);
    if (rc != 0) return rc;

    // the chunks' segments in chunk order, their times mapped into the caller's audio through the chunk's own table: a segment lasts
    // at least 10 cs (the getters' rule) and does not start before the previous one ended
    for (size_t c = 0; c < L.chunks.size(); ++c) {
        wa_long_rec & r = L.chunks[c];
        r.n_result = (int) results[c].size();
        for (wa_segment & seg : results[c]) {
            wa_long_map_segment(seg, r.table);
            if (!st->result_all.empty()) seg.t0 = std::max(seg.t0, st->result_all.back().t1);
            st->result_all.push_back(std::move(seg));
            if (params.new_segment_callback) params.new_segment_callback(ctx, st, 1, params.new_segment_callback_user_data);
        }
    }
    L.stats[6] = wa_time_us() - t;                  // as before the waves became wa_long_waves: member states, waves and mapping
    return 0;
}

extern "C" {

int whisper_amd_full_long(struct whisper_context * ctx, struct whisper_full_params params, const float * samples, int n_samples, int max_chunk_ms,
                          int n_parallel) {
    if (!ctx || !ctx->state || !samples || n_samples <= 0) { WA_ERROR("%s: refused: null context, state or samples\n", __func__); return -1; }
    if (params.offset_ms != 0 || params.duration_ms != 0) { WA_ERROR("%s: refused: offset_ms / duration_ms are not supported here\n", __func__); return -1; }
    const int rc = wa_guard(__func__, -1, [&] { return long_full(ctx, params, samples, n_samples, max_chunk_ms, n_parallel); });
    if (rc != 0) ctx->state->result_all.clear();
    return rc;
}

int whisper_amd_full_long_audio(struct whisper_context * ctx, struct whisper_full_params params, const void * data, int64_t n_frames, int channels,
                                int sample_rate, int format, int max_chunk_ms, int n_parallel) {
    if (!ctx || !ctx->state) { WA_ERROR("%s: refused: null context or state\n", __func__); return -1; }
    int64_t n = 0;
    const float * pcm = whisper_amd_audio_to_pcm(ctx->state, data, n_frames, channels, sample_rate, format, &n);
    if (!pcm) return -1;
    if (n > INT_MAX) { WA_ERROR("%s: refused: %lld samples at 16 kHz are more than whisper_full takes\n", __func__, (long long) n); return -1; }
    return whisper_amd_full_long(ctx, params, pcm, (int) n, max_chunk_ms, n_parallel);
}

int whisper_amd_long_n_chunks(struct whisper_context * ctx) { return ctx && ctx->state && ctx->state->lng ? (int) ctx->state->lng->chunks.size() : 0; }

int whisper_amd_long_chunk_info(struct whisper_context * ctx, int i, int64_t out[6]) {
    if (!out || i < 0 || i >= whisper_amd_long_n_chunks(ctx)) return -1;
    const wa_long_rec & r = ctx->state->lng->chunks[(size_t) i];
    out[0] = r.first; out[1] = r.count; out[2] = r.packed; out[3] = r.t0; out[4] = r.t1; out[5] = r.n_result;
    return 0;
}

int64_t whisper_amd_long_chunk_copy(struct whisper_context * ctx, int i, float * dst, int64_t cap) {
    if (i < 0 || i >= whisper_amd_long_n_chunks(ctx) || cap < 0 || (cap > 0 && !dst)) return -1;
    whisper_state * st = ctx->state;
    const wa_long_rec & r = st->lng->chunks[(size_t) i];
    const int64_t n = std::min<int64_t>(cap, r.packed);
    if (!WA_HIP_OK(hipSetDevice(ctx->device)) || !WA_HIP_OK(hipStreamSynchronize(st->stream))) return -1;
    if (n > 0 && !WA_HIP_OK(hipMemcpy(dst, st->lng->d_chunks + r.off, (size_t) n * sizeof(float), hipMemcpyDeviceToHost))) return -1;
    return r.packed;
}

void whisper_amd_long_stats(struct whisper_context * ctx, int64_t out[8]) {
    if (!out) return;
    for (int k = 0; k < 8; ++k) out[k] = ctx && ctx->state && ctx->state->lng ? ctx->state->lng->stats[k] : 0;
}

int whisper_amd_long_plan(const int64_t * segs_cs, int n_segs, int n_samples, float samples_overlap, int max_chunk_samples, int32_t * first,
                          int32_t * count, int64_t * packed, int cap) {
    if (n_segs < 0 || (n_segs > 0 && !segs_cs) || n_samples < 0 || cap < 0) return -1;
    return wa_guard(__func__, -1, [&] {
        const std::vector<wa_vad_seg> segs = long_segs(segs_cs, n_segs);
        const std::vector<wa_long_chunk> plan = wa_long_plan(segs.data(), n_segs, n_samples, samples_overlap, max_chunk_samples);
        for (size_t c = 0; c < plan.size() && c < (size_t) cap; ++c) {
            if (first) first[c] = plan[c].first;
            if (count) count[c] = plan[c].count;
            if (packed) packed[c] = plan[c].packed;
        }
        return (int) plan.size();
    });
}

int whisper_amd_long_pack(struct whisper_state * st, const float * samples, int n_samples, const int64_t * segs_cs, int n_segs, float samples_overlap,
                          const int32_t * first, const int32_t * count, int n_chunks, int where) {
    if (!st || !st->ctx || !samples || n_samples <= 0 || !segs_cs || n_segs <= 0 || !first || !count || n_chunks <= 0 || (where != 0 && where != 1)) return -1;
    return wa_guard(__func__, -1, [&] {
        const std::vector<wa_vad_seg> segs = long_segs(segs_cs, n_segs);
        std::vector<wa_long_chunk> plan;
        for (int c = 0; c < n_chunks; ++c) {
            if (first[c] < 0 || count[c] <= 0 || (int64_t) first[c] + count[c] > n_segs) return -1;
            plan.push_back({ first[c], count[c], wa_vad_layout_length(segs.data() + first[c], count[c], samples_overlap, n_samples) });
        }
        if (!WA_HIP_OK(hipSetDevice(st->ctx->device))) return -1;
        const bool on_device = wa_is_device_ptr(samples);
        wa_long_of(*st).stats[7] = 0;
        std::vector<wa_long_src> srcs;
        std::vector<wa_long_pick> order;
        single_source(segs.data(), n_samples, plan, srcs, order);
        if (!wa_long_pack(*st, on_device ? nullptr : samples, on_device ? samples : nullptr, srcs, order, samples_overlap, where)) {
            wa_long_of(*st).chunks.clear();
            return -1;
        }
        wa_long_of(*st).stats[2] = n_chunks;
        return 0;
    });
}

int whisper_amd_long_tile(void) { return WA_LONG_TILE; }

struct whisper_state * whisper_amd_context_state(struct whisper_context * ctx) { return ctx ? ctx->state : nullptr; }

} // extern "C"

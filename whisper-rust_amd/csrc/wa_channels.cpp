// wa_channels.cpp - two-channel recordings: the whisper_amd_audio_split / whisper_amd_channel_* /
// whisper_amd_full_long_channels entry points of include/whisper_amd.h.
//
// A stereo call recording carries one speaker per channel.  whisper_amd_audio_split turns the interleaved recording into two planes of
// 16 kHz F32 in one launch (wa_channels.hip), each plane bit for bit what whisper_amd_audio_to_pcm gives for that channel as a mono
// recording; whisper_amd_channel_energy sums |x| over spans of both planes in one launch, in the fixed order of wa_channels.h;
// whisper_amd_channel_speakers is the reference cli's --diarize rule on those sums.  whisper_amd_full_long_channels is
// whisper_amd_full_long for both channels in one call: one split, the VAD per plane, one pack launch for the chunks of both channels, and
// ONE list of chunks through the lock-step waves, so that two half-empty waves become one full one.
// The host functions of wa_channels.h serve WHISPER_AMD_CHANNELS_HOST=1 (read at each call) and any call whose HIP path fails (logged, counted).
#include "wa_long_host.h"
#include "wa_channels.h"

#include <climits>
#include <cstring>

struct wa_channels_state {
    float * d_planes = nullptr; size_t d_planes_cap = 0;            // floats: plane c at d_planes + c * stride
    int64_t n = -1, stride = 0;                                     // samples per plane of the last split, -1: none yet
    long long * d_spans = nullptr; size_t d_spans_cap = 0;          // the energy kernel's spans
    double * d_energy = nullptr; size_t d_energy_cap = 0;           // and its sums
    int64_t split_path = 0, split_h2d = 0;                          // of the last split: 0 host, 1 kernel; bytes of the recording copied host -> device
    int64_t n_split_fallback = 0, n_energy_launch = 0, n_energy_fallback = 0;       // since the state was created
    int64_t stats[11] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };        // whisper_amd_channels_stats
};

static wa_channels_state & chan_of(whisper_state & st) {
    if (!st.chn) st.chn = new wa_channels_state;
    return *st.chn;
}

void wa_channels_free(whisper_state & st) {
    if (!st.chn) return;
    if (st.ctx) (void) hipSetDevice(st.ctx->device);
    if (st.stream) (void) hipStreamSynchronize(st.stream);
    if (st.chn->d_planes) (void) hipFree(st.chn->d_planes);
    if (st.chn->d_spans) (void) hipFree(st.chn->d_spans);
    if (st.chn->d_energy) (void) hipFree(st.chn->d_energy);
    delete st.chn;
    st.chn = nullptr;
}

static bool channels_host_only() {
    const char * env = getenv("WHISPER_AMD_CHANNELS_HOST");
    return env && atoi(env) != 0;
}

static size_t frame_bytes(int format) { return wa_audio_frame_bytes(format, 2); }

// the kernels: input staged in HBM when it arrives in host memory, everything on the state's stream
static bool split_device_path(whisper_context & ctx, whisper_state & st, wa_channels_state & C, const void * data, bool on_device, int64_t n_frames, int format,
                              const wa_audio_plan & p, int64_t n_out, int64_t stride) {
    const float * d_taps = nullptr;
    if (p.K && !(d_taps = wa_audio_taps_device(ctx, p))) return false;
    const void * d_in = data;
    if (!on_device) {
        const size_t bytes = (size_t) n_frames * frame_bytes(format);
        if (!wa_dev_reserve(st.d_audio_in, st.d_audio_in_cap, bytes)) return false;
        if (!WA_HIP_OK(hipMemcpyAsync(st.d_audio_in, data, bytes, hipMemcpyHostToDevice, st.stream))) return false;
        C.split_h2d = (int64_t) bytes;
        d_in = st.d_audio_in;
    }
    if (!(wa_audio_format_base(format) ? wa_ch_split_launch(st.stream, d_in, n_frames, format, p, d_taps, n_out, stride, C.d_planes)
                                       : wa_ch_split_fmt_launch(st.stream, d_in, n_frames, format, p, d_taps, n_out, stride, C.d_planes))) return false;
    // the caller may release a host buffer on return; device input stays stream-ordered
    return on_device || WA_HIP_OK(hipStreamSynchronize(st.stream));
}

static bool split_host_path(whisper_state & st, wa_channels_state & C, const void * data, bool on_device, int64_t n_frames, int rate, int format, int64_t n_out,
                            int64_t stride) {
    std::vector<uint8_t> in;
    if (on_device) {
        in.resize((size_t) n_frames * frame_bytes(format));
        if (!WA_HIP_OK(hipStreamSynchronize(st.stream)) || !WA_HIP_OK(hipMemcpy(in.data(), data, in.size(), hipMemcpyDeviceToHost))) return false;
        data = in.data();
    }
    std::vector<float> out((size_t) (2 * stride), 0.0f);
    if (wa_ch_split_ref(data, n_frames, rate, format, nullptr, out.data(), stride) != n_out) return false;
    C.split_h2d = 0;                // the planes cross, the recording does not
    return WA_HIP_OK(hipMemcpyAsync(C.d_planes, out.data(), out.size() * sizeof(float), hipMemcpyHostToDevice, st.stream)) &&
           WA_HIP_OK(hipStreamSynchronize(st.stream));
}

// arguments checked by the caller (wa_ch_args_ok); null: failed (logged)
static const float * channels_split(whisper_state * st, const void * data, int64_t n_frames, int rate, int format, int64_t * n_samples, int64_t * stride_out,
                                    const char * who) {
    whisper_context & ctx = *st->ctx;
    wa_channels_state & C = chan_of(*st);
    wa_audio_plan p;
    wa_audio_plan_make(rate, p);
    const int64_t n_out = wa_audio_n_out(n_frames, rate), stride = wa_ch_stride(n_out);
    if (!WA_HIP_OK(hipSetDevice(ctx.device))) return nullptr;
    if (!wa_dev_reserve(C.d_planes, C.d_planes_cap, (size_t) std::max<int64_t>(2 * stride, 256))) return nullptr;
    C.n = -1;
    C.split_h2d = 0;
    if (n_out > 0) {
        const bool on_device = wa_is_device_ptr(data);
        bool served = false;
        if (!channels_host_only()) {
            served = split_device_path(ctx, *st, C, data, on_device, n_frames, format, p, n_out, stride);
            if (served) C.split_path = 1;
            else { C.n_split_fallback++; (void) hipGetLastError(); WA_WARN("%s: the device path failed, taking the host path\n", who); }
        }
        if (!served) {
            if (!split_host_path(*st, C, data, on_device, n_frames, rate, format, n_out, stride)) { WA_ERROR("%s: the host path failed\n", who); return nullptr; }
            C.split_path = 0;
        }
    }
    C.n = n_out;
    C.stride = stride;
    if (n_samples) *n_samples = n_out;
    if (stride_out) *stride_out = stride;
    return C.d_planes;
}

// energy[2 i + c] of spans[2 i], spans[2 i + 1] over the state's planes; where: 0 the host function, 1 the kernel, else the kernel unless
// WHISPER_AMD_CHANNELS_HOST=1, with the host function behind it
static bool channels_energy(whisper_state & st, const std::vector<long long> & spans, int where, double * energy) {
    wa_channels_state & C = chan_of(st);
    const int n_spans = (int) (spans.size() / 2);
    if (n_spans == 0) return true;
    if (!WA_HIP_OK(hipSetDevice(st.ctx->device))) return false;
    bool served = false;
    if (where == 1 || (where != 0 && !channels_host_only())) {
        served = wa_dev_reserve(C.d_spans, C.d_spans_cap, spans.size()) && wa_dev_reserve(C.d_energy, C.d_energy_cap, spans.size())
            && WA_HIP_OK(hipMemcpyAsync(C.d_spans, spans.data(), spans.size() * sizeof(long long), hipMemcpyHostToDevice, st.stream))
            && wa_ch_energy_launch(st.stream, C.d_planes, C.n, C.stride, C.d_spans, n_spans, C.d_energy);
        if (served) C.n_energy_launch++;
        served = served && WA_HIP_OK(hipMemcpyAsync(energy, C.d_energy, spans.size() * sizeof(double), hipMemcpyDeviceToHost, st.stream))
            && WA_HIP_OK(hipStreamSynchronize(st.stream));
        if (served || where == 1) return served;
        C.n_energy_fallback++;
        (void) hipGetLastError();
        WA_WARN("%s: the device path failed, taking the host path\n", __func__);
    }
    std::vector<float> x((size_t) (2 * C.stride));
    if (!WA_HIP_OK(hipStreamSynchronize(st.stream))) return false;
    if (!x.empty() && !WA_HIP_OK(hipMemcpy(x.data(), C.d_planes, x.size() * sizeof(float), hipMemcpyDeviceToHost))) return false;
    for (int i = 0; i < n_spans; ++i)
        for (int c = 0; c < 2; ++c) energy[2 * i + c] = wa_ch_energy_ref(x.data() + c * C.stride, C.n, spans[2 * (size_t) i], spans[2 * (size_t) i + 1]);
    return true;
}

static int channels_full(whisper_context * ctx, whisper_full_params params, const whisper_amd_channels_params & cp, const void * data, int64_t n_frames,
                         int rate, int format) {
    whisper_state * st = ctx->state;
    wa_long_state & L = wa_long_of(*st);
    wa_channels_state & C = chan_of(*st);
    st->result_all.clear();
    L.chunks.clear();
    L.seg_channel.clear();
    for (int k : { 0, 2, 3, 4, 5, 6, 7 }) L.stats[k] = 0;
    for (int k : { 0, 2, 3, 4, 5, 6, 7, 8, 9 }) C.stats[k] = 0;
    const int max_chunk_ms = cp.max_chunk_ms <= 0 ? 30000 : cp.max_chunk_ms;
    const int n_parallel = std::min(cp.n_parallel <= 0 ? 8 : cp.n_parallel, WA_MAX_DECODERS);
    const int max_chunk_samples = (int) std::min<int64_t>((int64_t) max_chunk_ms * (WHISPER_SAMPLE_RATE / 1000), INT_MAX);
    const float overlap = params.vad_params.samples_overlap;
    const int64_t packs0 = L.n_pack_launches, energies0 = C.n_energy_launch;
    auto publish = [&]() {
        C.stats[0] = C.split_path; C.stats[1] = C.n_split_fallback; C.stats[2] = C.n_energy_launch - energies0; C.stats[3] = L.n_pack_launches - packs0;
        C.stats[7] = (int64_t) L.chunks.size(); C.stats[8] = L.stats[3]; C.stats[9] = C.split_h2d; C.stats[10] = C.n_energy_fallback;
        L.stats[2] = (int64_t) L.chunks.size(); L.stats[7] = C.split_h2d;
    };

    // 1. both planes in HBM; complete before the VAD, which runs on a stream of its own, reads them
    int64_t n64 = 0, stride = 0;
    const float * planes = channels_split(st, data, n_frames, rate, format, &n64, &stride, __func__);
    publish();
    if (!planes || !WA_HIP_OK(hipStreamSynchronize(st->stream))) return -1;
    const int n = (int) n64;

    // 2. the VAD per plane, where it lies
    int64_t t = wa_time_us();
    std::vector<wa_vad_seg> found[2], kept[2];
    for (int c = 0; c < 2; ++c) {
        if (!wa_vad_segments_for(ctx, st, params, planes + c * stride, n, found[c])) { WA_ERROR("%s: failed to compute VAD\n", __func__); return -1; }
        C.stats[4 + c] = (int64_t) found[c].size();
    }
    L.stats[4] = wa_time_us() - t;
    if (found[0].empty() && found[1].empty()) return 0;

    // 3. the gate: one energy launch over every segment of both channels
    t = wa_time_us();
    if (cp.crosstalk_ratio > 0.0) {
        std::vector<long long> spans;
        for (int c = 0; c < 2; ++c)
            for (const wa_vad_seg & s : found[c]) {
                spans.push_back(wa_vad_cs_to_samples(s.start));
                spans.push_back(std::min<long long>(wa_vad_cs_to_samples(s.end), n));
            }
        std::vector<double> e(spans.size());
        if (!channels_energy(*st, spans, -1, e.data())) { WA_ERROR("%s: failed to compute the channel energies\n", __func__); publish(); return -1; }
        size_t i = 0;
        for (int c = 0; c < 2; ++c)
            for (const wa_vad_seg & s : found[c]) {
                if (wa_ch_gate_drops(e[2 * i + c], e[2 * i + (1 - c)], cp.crosstalk_ratio)) C.stats[6]++;
                else kept[c].push_back(s);
                ++i;
            }
    } else {
        kept[0] = found[0];
        kept[1] = found[1];
    }

    // 4. a plan per channel, one pack for both: the chunks in the order (original start, channel)
    std::vector<wa_long_chunk> plan[2];
    std::vector<wa_long_src> srcs;
    std::vector<wa_long_pick> order;
    for (int c = 0; c < 2; ++c) {
        plan[c] = wa_long_plan(kept[c].data(), (int) kept[c].size(), n, overlap, max_chunk_samples);
        srcs.push_back({ kept[c].data(), n, (int64_t) c * stride, c, &plan[c] });
        for (size_t k = 0; k < plan[c].size(); ++k) order.push_back({ c, (int) k });
    }
    std::stable_sort(order.begin(), order.end(), [&](const wa_long_pick & a, const wa_long_pick & b) {
        const int64_t ta = kept[a.src][(size_t) plan[a.src][(size_t) a.chunk].first].start, tb = kept[b.src][(size_t) plan[b.src][(size_t) b.chunk].first].start;
        return ta != tb ? ta < tb : a.src < b.src;
    });
    if (order.empty()) { publish(); return 0; }
    const bool packed = wa_long_pack_any(*st, nullptr, planes, srcs, order, overlap, __func__);
    publish();
    if (!packed) return -1;
    L.stats[5] = wa_time_us() - t;
    WA_INFO("%s: %d + %d speech segments (%d dropped by the gate) in %d chunks of at most %d ms\n", __func__, (int) found[0].size(), (int) found[1].size(),
            (int) C.stats[6], (int) L.chunks.size(), max_chunk_ms);

    // 5. one list of chunks through the waves
    t = wa_time_us();
    std::vector<std::vector<wa_segment>> results;
    const int rc = wa_long_waves(ctx, params, n_parallel, results);
    publish();
    if (rc != 0) return rc;

    // 6. times mapped through each chunk's table, clamped inside the channel, merged by (t0, channel, order within the channel)
    std::vector<wa_ch_item> items[2];
    std::vector<wa_segment *> segs[2];
    for (size_t c = 0; c < L.chunks.size(); ++c) {
        wa_long_rec & r = L.chunks[c];
        r.n_result = (int) results[c].size();
        for (wa_segment & seg : results[c]) {
            wa_long_map_segment(seg, r.table);
            items[r.channel].push_back({ seg.t0, seg.t1, r.channel, 0 });
            segs[r.channel].push_back(&seg);
        }
    }
    for (const wa_ch_item & it : wa_ch_merge(items)) {
        wa_segment & seg = *segs[it.channel][(size_t) it.index];
        seg.t0 = it.t0;
        seg.t1 = it.t1;
        st->result_all.push_back(std::move(seg));
        L.seg_channel.push_back((int8_t) it.channel);
        if (params.new_segment_callback) params.new_segment_callback(ctx, st, 1, params.new_segment_callback_user_data);
    }
    L.stats[6] = wa_time_us() - t;
    return 0;
}

extern "C" {

const float * whisper_amd_audio_split(struct whisper_state * st, const void * data, int64_t n_frames, int sample_rate, int format, int64_t * n_samples,
                                      int64_t * stride) {
    if (!st || !st->ctx || !n_samples || !stride || !wa_ch_args_ok(data, n_frames, sample_rate, format)) {
        WA_ERROR("%s: refused: %lld frames, %d Hz, format %d%s\n", __func__, (long long) n_frames, sample_rate, format,
                 !st || !n_samples || !stride ? " (null state, n_samples or stride)" : !data && n_frames > 0 ? " (null data)" : "");
        return nullptr;
    }
    const char * who = __func__;
    return wa_guard(who, (const float *) nullptr, [&] { return channels_split(st, data, n_frames, sample_rate, format, n_samples, stride, who); });
}

int64_t whisper_amd_audio_split_copy(struct whisper_state * st, int channel, float * dst, int64_t cap) {
    if (!st || !st->ctx || !st->chn || st->chn->n < 0 || (channel != 0 && channel != 1) || cap < 0 || (cap > 0 && !dst)) return -1;
    const wa_channels_state & C = *st->chn;
    const int64_t n = std::min(cap, C.n);
    if (!WA_HIP_OK(hipSetDevice(st->ctx->device)) || !WA_HIP_OK(hipStreamSynchronize(st->stream))) return -1;
    if (n > 0 && !WA_HIP_OK(hipMemcpy(dst, C.d_planes + channel * C.stride, (size_t) n * sizeof(float), hipMemcpyDeviceToHost))) return -1;
    return C.n;
}

int whisper_amd_channel_energy(struct whisper_state * st, const int64_t * is0, const int64_t * is1, int n_spans, int where, double * energy) {
    if (!st || !st->ctx || !st->chn || st->chn->n < 0 || n_spans < 0 || (n_spans > 0 && (!is0 || !is1 || !energy))) {
        WA_ERROR("%s: refused: null arguments, or no whisper_amd_audio_split on this state yet\n", __func__);
        return -1;
    }
    return wa_guard(__func__, -1, [&] {
        std::vector<long long> spans((size_t) n_spans * 2);
        for (int i = 0; i < n_spans; ++i) { spans[2 * (size_t) i] = is0[i]; spans[2 * (size_t) i + 1] = is1[i]; }
        return channels_energy(*st, spans, where, energy) ? 0 : -1;
    });
}

int whisper_amd_channel_speakers(struct whisper_state * st, const int64_t * t0_cs, const int64_t * t1_cs, int n, double ratio, double * energy,
                                 int8_t * speaker) {
    if (!st || !st->ctx || !st->chn || st->chn->n < 0 || n < 0 || (n > 0 && (!t0_cs || !t1_cs || !speaker))) {
        WA_ERROR("%s: refused: null arguments, or no whisper_amd_audio_split on this state yet\n", __func__);
        return -1;
    }
    return wa_guard(__func__, -1, [&] {
        const int64_t n_samples = st->chn->n;
        std::vector<long long> spans((size_t) n * 2);
        for (int i = 0; i < n; ++i) {
            spans[2 * (size_t) i] = wa_ch_cs_to_sample(t0_cs[i], n_samples);
            spans[2 * (size_t) i + 1] = wa_ch_cs_to_sample(t1_cs[i], n_samples);
        }
        std::vector<double> e((size_t) n * 2, 0.0);
        if (!channels_energy(*st, spans, -1, e.data())) return -1;
        for (int i = 0; i < n; ++i) speaker[i] = (int8_t) wa_ch_label(e[2 * (size_t) i], e[2 * (size_t) i + 1], ratio);
        if (energy && n > 0) memcpy(energy, e.data(), e.size() * sizeof(double));
        return 0;
    });
}

void whisper_amd_channels_default_params(struct whisper_amd_channels_params * p) {
    if (!p) return;
    p->max_chunk_ms = 30000; p->n_parallel = 8; p->crosstalk_ratio = 0.0;
}

int whisper_amd_full_long_channels(struct whisper_context * ctx, struct whisper_full_params params, const struct whisper_amd_channels_params * cp,
                                   const void * data, int64_t n_frames, int sample_rate, int format) {
    if (!ctx || !ctx->state || !cp || !data || n_frames <= 0) { WA_ERROR("%s: refused: null context, state, parameters or recording\n", __func__); return -1; }
    if (params.offset_ms != 0 || params.duration_ms != 0) { WA_ERROR("%s: refused: offset_ms / duration_ms are not supported here\n", __func__); return -1; }
    if (!(cp->crosstalk_ratio >= 0.0)) { WA_ERROR("%s: refused: crosstalk_ratio %g\n", __func__, cp->crosstalk_ratio); return -1; }
    if (!wa_ch_args_ok(data, n_frames, sample_rate, format)) {
        WA_ERROR("%s: refused: %lld frames, %d Hz, format %d\n", __func__, (long long) n_frames, sample_rate, format);
        return -1;
    }
    if (wa_audio_n_out(n_frames, sample_rate) > INT_MAX) {
        WA_ERROR("%s: refused: %lld samples at 16 kHz are more than whisper_full takes\n", __func__, (long long) wa_audio_n_out(n_frames, sample_rate));
        return -1;
    }
    const int rc = wa_guard(__func__, -1, [&] { return channels_full(ctx, params, *cp, data, n_frames, sample_rate, format); });
    if (rc != 0) {
        ctx->state->result_all.clear();
        if (ctx->state->lng) { ctx->state->lng->seg_channel.clear(); ctx->state->lng->chunks.clear(); }
    }
    return rc;
}

int whisper_amd_long_segment_channel(struct whisper_context * ctx, int i) {
    if (!ctx || !ctx->state || !ctx->state->lng) return -1;
    const std::vector<int8_t> & ch = ctx->state->lng->seg_channel;
    return i >= 0 && (size_t) i < ch.size() && ch.size() == ctx->state->result_all.size() ? ch[(size_t) i] : -1;
}

int whisper_amd_long_chunk_channel(struct whisper_context * ctx, int i) {
    if (i < 0 || i >= whisper_amd_long_n_chunks(ctx)) return -1;
    return ctx->state->lng->chunks[(size_t) i].channel;
}

void whisper_amd_channels_stats(struct whisper_context * ctx, int64_t out[11]) {
    if (!out) return;
    for (int k = 0; k < 11; ++k) out[k] = ctx && ctx->state && ctx->state->chn ? ctx->state->chn->stats[k] : 0;
}

int whisper_amd_channels_tile(void) { return WA_CH_TILE; }
int whisper_amd_channels_energy_lanes(void) { return WA_CH_LANES; }

} // extern "C"

// wa_audio.cpp - audio front end: the whisper_amd_audio_* entry points of include/whisper_amd.h.
//
// whisper-rs callers turn a recording into 16 kHz mono F32 on the host before whisper_full (src/utilities.rs: convert_integer_to_float_audio,
// convert_stereo_to_mono_audio) and the examples refuse any other rate.  Here int16 or F32 input with one or two channels at 8 .. 192 kHz
// (and, in the kernels of wa_audio_fmt.hip, 8-, 24- and 32-bit PCM, F64 and G.711) is converted, down-mixed and resampled by the kernels of wa_audio.hip on the state's stream, into a buffer of the state that
// whisper_full_with_state reads in place.  The arithmetic is wa_audio.h's; wa_audio_ref, the same arithmetic on the host, serves
// WHISPER_AMD_AUDIO_HOST=1 (read when the state is created) and any call whose HIP path fails: the failure is logged and the call succeeds.
#include "wa_internal.h"
#include "wa_audio.h"
#include "wa_wav.h"

#include <climits>
#include <cstddef>
#include <cstring>

static_assert(WA_AUDIO_I16 == WHISPER_AMD_PCM_I16 && WA_AUDIO_F32 == WHISPER_AMD_PCM_F32, "the format codes of wa_audio.h are the header's");
static_assert(WA_AUDIO_U8 == WHISPER_AMD_PCM_U8 && WA_AUDIO_S24 == WHISPER_AMD_PCM_S24 && WA_AUDIO_S32 == WHISPER_AMD_PCM_S32 &&
              WA_AUDIO_F64 == WHISPER_AMD_PCM_F64 && WA_AUDIO_ULAW == WHISPER_AMD_PCM_ULAW && WA_AUDIO_ALAW == WHISPER_AMD_PCM_ALAW,
              "the format codes of wa_audio.h are the header's");
static_assert(sizeof(wa_wav_info) == sizeof(whisper_amd_wav_info) && offsetof(wa_wav_info, n_frames) == offsetof(whisper_amd_wav_info, n_frames) &&
              offsetof(wa_wav_info, channels) == offsetof(whisper_amd_wav_info, channels) && offsetof(wa_wav_info, bits) == offsetof(whisper_amd_wav_info, bits),
              "wa_wav.h's record is the header's");

void wa_audio_free(whisper_context & ctx) {
    std::lock_guard<std::mutex> lock(ctx.audio_taps_m);
    for (auto & kv : ctx.audio_taps) if (kv.second) (void) hipFree(kv.second);
    ctx.audio_taps.clear();
}

// the device copy of a rate's table: built and uploaded by the first call at that rate on this context, kept until whisper_free
const float * wa_audio_taps_device(whisper_context & ctx, const wa_audio_plan & p) {
    std::lock_guard<std::mutex> lock(ctx.audio_taps_m);
    auto it = ctx.audio_taps.find(p.rate);
    if (it != ctx.audio_taps.end()) return it->second;
    std::vector<float> taps;
    wa_audio_taps(p, taps);
    float * d = nullptr;
    if (!WA_HIP_OK(hipMalloc((void **) &d, taps.size() * sizeof(float)))) return nullptr;
    if (!WA_HIP_OK(hipMemcpy(d, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice))) { (void) hipFree(d); return nullptr; }
    ctx.audio_taps[p.rate] = d;
    return d;
}

// the kernels: input staged in HBM when it arrives in host memory, everything on the state's stream
static bool audio_device_path(whisper_context & ctx, whisper_state & st, const void * data, bool on_device, int64_t n_frames, int channels, int format,
                              const wa_audio_plan & p, int64_t n_out) {
    const float * d_taps = nullptr;
    if (p.K && !(d_taps = wa_audio_taps_device(ctx, p))) return false;
    const void * d_in = data;
    if (!on_device) {
        const size_t bytes = (size_t) n_frames * wa_audio_frame_bytes(format, channels);
        if (!wa_dev_reserve(st.d_audio_in, st.d_audio_in_cap, bytes)) return false;
        if (!WA_HIP_OK(hipMemcpyAsync(st.d_audio_in, data, bytes, hipMemcpyHostToDevice, st.stream))) return false;
        d_in = st.d_audio_in;
    }
    if (!(wa_audio_format_base(format) ? wa_audio_launch(st.stream, d_in, n_frames, channels, format, p, d_taps, n_out, st.d_audio)
                                       : wa_audio_fmt_launch(st.stream, d_in, n_frames, channels, format, p, d_taps, n_out, st.d_audio))) return false;
    // the caller may release a host buffer on return; device input stays stream-ordered
    return on_device || WA_HIP_OK(hipStreamSynchronize(st.stream));
}

static bool audio_host_path(whisper_state & st, const void * data, bool on_device, int64_t n_frames, int channels, int rate, int format, int64_t n_out) {
    std::vector<uint8_t> in;
    if (on_device) {
        in.resize((size_t) n_frames * wa_audio_frame_bytes(format, channels));
        if (!WA_HIP_OK(hipStreamSynchronize(st.stream)) || !WA_HIP_OK(hipMemcpy(in.data(), data, in.size(), hipMemcpyDeviceToHost))) return false;
        data = in.data();
    }
    std::vector<float> out((size_t) n_out);
    if (wa_audio_ref(data, n_frames, channels, rate, format, nullptr, out.data()) != n_out) return false;
    return WA_HIP_OK(hipMemcpyAsync(st.d_audio, out.data(), out.size() * sizeof(float), hipMemcpyHostToDevice, st.stream)) &&
           WA_HIP_OK(hipStreamSynchronize(st.stream));
}

int64_t whisper_amd_audio_n_samples(int64_t n_frames, int sample_rate) { return wa_audio_n_out(n_frames, sample_rate); }

const float * whisper_amd_audio_to_pcm(struct whisper_state * st, const void * data, int64_t n_frames, int channels, int sample_rate, int format,
                                       int64_t * n_samples) {
    if (!st || !st->ctx || !n_samples || !wa_audio_args_ok(data, n_frames, channels, sample_rate, format)) {
        WA_ERROR("%s: refused: %lld frames, %d channels, %d Hz, format %d%s\n", __func__, (long long) n_frames, channels, sample_rate, format,
                 !st || !n_samples ? " (null state or n_samples)" : !data && n_frames > 0 ? " (null data)" : "");
        return nullptr;
    }
    try {
        whisper_context & ctx = *st->ctx;
        wa_audio_plan p;
        wa_audio_plan_make(sample_rate, p);
        const int64_t n_out = wa_audio_n_out(n_frames, sample_rate);
        if (!WA_HIP_OK(hipSetDevice(ctx.device))) return nullptr;
        if (!wa_dev_reserve(st->d_audio, st->d_audio_cap, (size_t) std::max<int64_t>(n_out, 256))) return nullptr;
        st->audio_n = -1;
        if (n_out > 0) {
            const bool on_device = wa_is_device_ptr(data);
            bool served = false;
            if (!st->audio_host) {
                served = audio_device_path(ctx, *st, data, on_device, n_frames, channels, format, p, n_out);
                if (served) st->n_audio_device++;
                else { st->n_audio_fallback++; (void) hipGetLastError(); WA_WARN("%s: the device path failed, taking the host path\n", __func__); }
            }
            if (!served) {
                if (!audio_host_path(*st, data, on_device, n_frames, channels, sample_rate, format, n_out)) {
                    WA_ERROR("%s: the host path failed\n", __func__);
                    return nullptr;
                }
                st->n_audio_host++;
            }
        }
        st->audio_n = n_out;
        *n_samples = n_out;
        return st->d_audio;
    } catch (const std::exception & e) {
        WA_ERROR("%s: exception: %s\n", __func__, e.what());
        return nullptr;
    }
}

int whisper_amd_full_audio(struct whisper_context * ctx, struct whisper_state * st, struct whisper_full_params params, const void * data,
                           int64_t n_frames, int channels, int sample_rate, int format) {
    if (!ctx || !st || st->ctx != ctx) { WA_ERROR("%s: refused: null context or state, or a state of another context\n", __func__); return -1; }
    int64_t n = 0;
    const float * pcm = whisper_amd_audio_to_pcm(st, data, n_frames, channels, sample_rate, format, &n);
    if (!pcm) return -1;
    if (n > INT_MAX) { WA_ERROR("%s: refused: %lld samples at 16 kHz are more than whisper_full takes\n", __func__, (long long) n); return -1; }
    return whisper_full_with_state(ctx, st, params, pcm, (int) n);
}

int64_t whisper_amd_audio_copy(struct whisper_state * st, float * dst, int64_t cap) {
    if (!st || !st->ctx || st->audio_n < 0 || cap < 0 || (cap > 0 && !dst)) return -1;
    const int64_t n = std::min(cap, st->audio_n);
    if (!WA_HIP_OK(hipSetDevice(st->ctx->device)) || !WA_HIP_OK(hipStreamSynchronize(st->stream))) return -1;
    if (n > 0 && !WA_HIP_OK(hipMemcpy(dst, st->d_audio, (size_t) n * sizeof(float), hipMemcpyDeviceToHost))) return -1;
    return st->audio_n;
}

int64_t whisper_amd_audio_taps(int sample_rate, float * dst, int64_t cap, int * L, int * M, int * K) {
    wa_audio_plan p;
    if (!wa_audio_plan_make(sample_rate, p) || cap < 0 || (cap > 0 && !dst)) return -1;
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (K) *K = p.K;
    const int64_t n = (int64_t) p.L * p.K;
    if (cap > 0 && n > 0) {
        std::vector<float> taps;
        wa_audio_taps(p, taps);
        memcpy(dst, taps.data(), (size_t) std::min(cap, n) * sizeof(float));
    }
    return n;
}

int whisper_amd_audio_tile(void) { return WA_AUDIO_TILE; }

int whisper_amd_wav_parse(const void * image, int64_t size, struct whisper_amd_wav_info * out) {
    return wa_guard(__func__, -1, [&] {
        wa_wav_info w;
        const int rc = wa_wav_parse(image, size, out ? &w : nullptr);
        if (rc == 0) {
            out->data_offset = w.data_offset; out->n_frames = w.n_frames; out->channels = w.channels; out->sample_rate = w.sample_rate;
            out->format = w.format; out->bits = w.bits;
        }
        return rc;
    });
}

void whisper_amd_audio_stats(struct whisper_state * st, long out[3]) {
    if (!out) return;
    out[0] = st ? st->n_audio_device : 0; out[1] = st ? st->n_audio_host : 0; out[2] = st ? st->n_audio_fallback : 0;
}

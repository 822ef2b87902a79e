// wa_vad.cpp - whisper_vad_context and the whisper_vad_* API: device weights, the slab pipeline around k_vad_front (wa_vad.hip) and
// the host recurrence (wa_vad_host.cpp); the VAD step of whisper_full / whisper_full_parallel (ref: whisper.cpp:6615-6793).
//
// whisper_vad_detect_speech cuts the audio into slabs of `slab` windows (4096; WHISPER_AMD_VAD_SLAB overrides it when the context is
// created).  Slab k + 1's samples go to the device and its front end runs on the context's stream while the calling thread walks the
// LSTM over slab k's gate inputs in a pinned buffer: two buffers of each kind, one event each.
#include "wa_internal.h"
#include "wa_vad.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

struct whisper_vad_segments { std::vector<wa_vad_seg> data; };

struct whisper_vad_context {
    int64_t t_vad_us = 0;                  // detect_speech, wall time (as the reference's field)
    int64_t t_front_wait_us = 0;           // of it: the calling thread waiting for the device
    int64_t t_host_us = 0;                 // of it: the recurrence
    int device = 0, n_threads = 4, slab = 4096;
    wa_vad_model model;
    std::string path_model;
    void * d_weights = nullptr;
    wa_vad_dev dev;
    hipStream_t stream = nullptr;
    float * d_samples[2] = { nullptr, nullptr }, * d_out[2] = { nullptr, nullptr }, * h_out[2] = { nullptr, nullptr };
    hipEvent_t ev[2] = { nullptr, nullptr };
    std::vector<float> probs;
};

// -------------------------------------------------------------------------------------------------
// creation
// -------------------------------------------------------------------------------------------------
static bool vad_upload(whisper_vad_context & v) {
    const wa_vad_model & m = v.model;
    // one allocation, every tensor on a 256-byte boundary; layer 0's rows padded from 387 to WA_VAD_LD0 halfs (16-byte row starts)
    std::vector<uint8_t> img;
    auto put = [&](const void * src, size_t bytes) { const size_t at = (img.size() + 255) & ~(size_t) 255; img.resize(at + bytes); memcpy(img.data() + at, src, bytes); return at; };
    std::vector<uint16_t> w0((size_t) 128 * WA_VAD_LD0, 0);
    for (int r = 0; r < 128; ++r) memcpy(&w0[(size_t) r * WA_VAD_LD0], &m.enc_w[0][(size_t) r * 387], 387 * sizeof(uint16_t));
    size_t o_w[4], o_b[4];
    const size_t o_stft = put(m.stft.data(), m.stft.size() * 2);
    o_w[0] = put(w0.data(), w0.size() * 2);
    for (int i = 1; i < 4; ++i) o_w[i] = put(m.enc_w[i].data(), m.enc_w[i].size() * 2);
    for (int i = 0; i < 4; ++i) o_b[i] = put(m.enc_b[i].data(), m.enc_b[i].size() * 4);
    const size_t o_wih = put(m.w_ih.data(), m.w_ih.size() * 4), o_bih = put(m.b_ih.data(), m.b_ih.size() * 4);
    img.resize(img.size() + 256);          // the kernel's look-ahead load never leaves a row, the slack is for good measure
    if (!WA_HIP_OK(hipMalloc(&v.d_weights, img.size()))) return false;
    if (!WA_HIP_OK(hipMemcpy(v.d_weights, img.data(), img.size(), hipMemcpyHostToDevice))) return false;
    const uint8_t * base = (const uint8_t *) v.d_weights;
    v.dev.stft = (const uint16_t *) (base + o_stft);
    for (int i = 0; i < 4; ++i) { v.dev.enc_w[i] = (const uint16_t *) (base + o_w[i]); v.dev.enc_b[i] = (const float *) (base + o_b[i]); }
    v.dev.w_ih = (const float *) (base + o_wih);
    v.dev.b_ih = (const float *) (base + o_bih);
    return true;
}

whisper_vad_context * wa_vad_create(whisper_model_loader * loader, int n_threads, int device) {
    auto * v = new whisper_vad_context;
    v->n_threads = n_threads;
    v->device = device;
    std::string err;
    if (!wa_vad_model_load(loader, v->model, err)) {
        WA_ERROR("%s: %s\n", __func__, err.c_str());
        delete v;
        return nullptr;
    }
    WA_INFO("%s: model type: %s, version: %s\n", __func__, v->model.type.c_str(), v->model.version.c_str());
    if (const char * s = getenv("WHISPER_AMD_VAD_SLAB")) v->slab = std::max(1, std::min(1 << 16, atoi(s)));
    int n_dev = 0;
    bool ok = WA_HIP_OK(hipGetDeviceCount(&n_dev)) && device >= 0 && device < n_dev && WA_HIP_OK(hipSetDevice(device));
    if (!ok) WA_ERROR("%s: no usable HIP device %d (this backend has no CPU path for VAD)\n", __func__, device);
    ok = ok && vad_upload(*v) && WA_HIP_OK(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
    for (int i = 0; i < 2 && ok; ++i) {
        ok = WA_HIP_OK(hipMalloc(&v->d_samples[i], (size_t) v->slab * WA_VAD_WINDOW * sizeof(float)))
          && WA_HIP_OK(hipMalloc(&v->d_out[i], (size_t) v->slab * WA_VAD_GATES * sizeof(float)))
          && WA_HIP_OK(hipHostMalloc(&v->h_out[i], (size_t) v->slab * WA_VAD_GATES * sizeof(float), hipHostMallocDefault))
          && WA_HIP_OK(hipEventCreateWithFlags(&v->ev[i], hipEventDisableTiming));
    }
    if (!ok) { whisper_vad_free(v); return nullptr; }
    return v;
}

namespace {
struct file_loader {
    FILE * f = nullptr;
    whisper_model_loader l;
    explicit file_loader(const char * path) {
        f = fopen(path, "rb");
        l.context = this;
        l.read  = [](void * c, void * out, size_t n) -> size_t { return fread(out, 1, n, ((file_loader *) c)->f); };
        l.eof   = [](void * c) -> bool { return feof(((file_loader *) c)->f) != 0; };
        l.close = [](void * c) { auto * s = (file_loader *) c; if (s->f) { fclose(s->f); s->f = nullptr; } };
    }
    ~file_loader() { if (f) fclose(f); }
};
}

whisper_vad_context * wa_vad_create_from_file(const char * path, int n_threads, int device) {
    if (!path) { WA_ERROR("%s: no VAD model path\n", __func__); return nullptr; }
    WA_INFO("%s: loading VAD model from '%s'\n", __func__, path);
    file_loader fl(path);
    if (!fl.f) { WA_ERROR("%s: failed to open VAD model '%s'\n", __func__, path); return nullptr; }
    whisper_vad_context * v = wa_vad_create(&fl.l, n_threads, device);
    if (v) v->path_model = path;
    return v;
}

// -------------------------------------------------------------------------------------------------
// the slab pipeline: consume(first window, number of windows, their [n][512] gate inputs in pinned memory)
// -------------------------------------------------------------------------------------------------
template <class F>
static bool vad_run_slabs(whisper_vad_context & v, const float * samples, int n_samples, F consume) {
    const int n_chunks = wa_vad_n_chunks(n_samples);
    if (n_chunks == 0) return true;
    if (!WA_HIP_OK(hipSetDevice(v.device))) return false;
    const int n_slabs = (n_chunks + v.slab - 1) / v.slab;
    // audio that already lies in HBM (whisper_amd_audio_to_pcm's result, whisper_amd_full_long's buffer) is read in place: a slab starts at a
    // multiple of 512 floats of it and the kernel reads nothing at or past n_valid
    const bool on_device = wa_is_device_ptr(samples);
    auto enqueue = [&](int k) {
        const int b = k & 1, c0 = k * v.slab, nc = std::min(v.slab, n_chunks - c0);
        const int64_t s0 = (int64_t) c0 * WA_VAD_WINDOW;
        const int n_valid = (int) std::min<int64_t>((int64_t) nc * WA_VAD_WINDOW, (int64_t) n_samples - s0);
        return (on_device || WA_HIP_OK(hipMemcpyAsync(v.d_samples[b], samples + s0, (size_t) n_valid * sizeof(float), hipMemcpyHostToDevice, v.stream)))
            && wa_vad_front_launch(v.dev, on_device ? samples + s0 : v.d_samples[b], n_valid, nc, v.d_out[b], (void *) v.stream)
            && WA_HIP_OK(hipMemcpyAsync(v.h_out[b], v.d_out[b], (size_t) nc * WA_VAD_GATES * sizeof(float), hipMemcpyDeviceToHost, v.stream))
            && WA_HIP_OK(hipEventRecord(v.ev[b], v.stream));
    };
    bool ok = enqueue(0);
    for (int k = 0; k < n_slabs && ok; ++k) {
        if (k + 1 < n_slabs) ok = enqueue(k + 1);
        const int64_t t0 = wa_time_us();
        ok = WA_HIP_OK(hipEventSynchronize(v.ev[k & 1])) && ok;
        v.t_front_wait_us += wa_time_us() - t0;
        if (ok) consume(k * v.slab, std::min(v.slab, n_chunks - k * v.slab), (const float *) v.h_out[k & 1]);
    }
    if (!ok) (void) hipStreamSynchronize(v.stream);       // nothing of this call may still be writing the buffers
    return ok;
}

// -------------------------------------------------------------------------------------------------
// C API (ref: whisper.cpp:4445-4452, 4731-4773, 5100-5200, 5438-5475)
// -------------------------------------------------------------------------------------------------
struct whisper_vad_context_params whisper_vad_default_context_params(void) {
    whisper_vad_context_params r; r.n_threads = 4; r.use_gpu = false; r.gpu_device = 0; return r;
}
// use_gpu is not looked at: its default is false and this backend has no CPU path - the front end always runs on gpu_device
struct whisper_vad_context * whisper_vad_init_from_file_with_params(const char * path_model, struct whisper_vad_context_params params) {
    try { return wa_vad_create_from_file(path_model, params.n_threads, params.gpu_device); }
    catch (const std::exception & e) { WA_ERROR("%s: exception: %s\n", __func__, e.what()); return nullptr; }
}
struct whisper_vad_context * whisper_vad_init_with_params(struct whisper_model_loader * loader, struct whisper_vad_context_params params) {
    if (!loader || !loader->read) return nullptr;
    try { return wa_vad_create(loader, params.n_threads, params.gpu_device); }
    catch (const std::exception & e) { WA_ERROR("%s: exception: %s\n", __func__, e.what()); return nullptr; }
}

bool whisper_vad_detect_speech(struct whisper_vad_context * vctx, const float * samples, int n_samples) {
    if (!vctx || n_samples < 0 || (n_samples > 0 && !samples)) return false;
    const int n_chunks = wa_vad_n_chunks(n_samples);
    WA_INFO("%s: detecting speech in %d samples, %d windows\n", __func__, n_samples, n_chunks);
    vctx->probs.assign((size_t) n_chunks, 0.0f);
    wa_vad_lstm st; st.reset();                         // the LSTM state is zero at the start of every call
    const int64_t t_start = wa_time_us();
    const bool ok = vad_run_slabs(*vctx, samples, n_samples, [&](int c0, int nc, const float * gates) {
        const int64_t t0 = wa_time_us();
        for (int i = 0; i < nc; ++i) vctx->probs[(size_t) c0 + i] = wa_vad_step(vctx->model, st, gates + (size_t) i * WA_VAD_GATES);
        vctx->t_host_us += wa_time_us() - t0;
    });
    vctx->t_vad_us += wa_time_us() - t_start;
    WA_INFO("%s: vad time = %.2f ms processing %d samples\n", __func__, 1e-3f * vctx->t_vad_us, n_samples);
    return ok;
}
int     whisper_vad_n_probs(struct whisper_vad_context * vctx) { return (int) vctx->probs.size(); }
float * whisper_vad_probs  (struct whisper_vad_context * vctx) { return vctx->probs.data(); }

struct whisper_vad_segments * whisper_vad_segments_from_probs(struct whisper_vad_context * vctx, struct whisper_vad_params params) {
    if (!vctx) return nullptr;
    auto * s = new whisper_vad_segments;
    s->data = wa_vad_segments_from_probs(vctx->probs.data(), (int) vctx->probs.size(), vctx->model.n_window, params);
    return s;
}
struct whisper_vad_segments * whisper_vad_segments_from_samples(struct whisper_vad_context * vctx, struct whisper_vad_params params, const float * samples, int n_samples) {
    if (!whisper_vad_detect_speech(vctx, samples, n_samples)) { WA_ERROR("%s: failed to detect speech\n", __func__); return nullptr; }
    return whisper_vad_segments_from_probs(vctx, params);
}
int   whisper_vad_segments_n_segments(struct whisper_vad_segments * s) { return (int) s->data.size(); }
float whisper_vad_segments_get_segment_t0(struct whisper_vad_segments * s, int i) { return (float) s->data[i].start; }
float whisper_vad_segments_get_segment_t1(struct whisper_vad_segments * s, int i) { return (float) s->data[i].end; }
void  whisper_vad_free_segments(struct whisper_vad_segments * s) { delete s; }

void whisper_vad_free(struct whisper_vad_context * v) {
    if (!v) return;
    (void) hipSetDevice(v->device);
    if (v->stream) (void) hipStreamSynchronize(v->stream);
    for (int i = 0; i < 2; ++i) {
        if (v->d_samples[i]) (void) hipFree(v->d_samples[i]);
        if (v->d_out[i]) (void) hipFree(v->d_out[i]);
        if (v->h_out[i]) (void) hipHostFree(v->h_out[i]);
        if (v->ev[i]) (void) hipEventDestroy(v->ev[i]);
    }
    if (v->d_weights) (void) hipFree(v->d_weights);
    if (v->stream) (void) hipStreamDestroy(v->stream);
    delete v;
}

// -------------------------------------------------------------------------------------------------
// extensions (include/whisper_amd.h)
// -------------------------------------------------------------------------------------------------
int whisper_amd_vad_tile(void) { return WA_VAD_TILE; }

int64_t whisper_amd_vad_front(struct whisper_vad_context * vctx, const float * samples, int n_samples, float * dst, int64_t cap) {
    if (!vctx || n_samples < 0 || (n_samples > 0 && !samples)) return -1;
    const int64_t n = (int64_t) wa_vad_n_chunks(n_samples) * WA_VAD_GATES;
    if (dst && cap > 0) {
        const bool ok = vad_run_slabs(*vctx, samples, n_samples, [&](int c0, int nc, const float * gates) {
            const int64_t at = (int64_t) c0 * WA_VAD_GATES, len = std::min((int64_t) nc * WA_VAD_GATES, cap - at);
            if (len > 0) memcpy(dst + at, gates, (size_t) len * sizeof(float));
        });
        if (!ok) return -1;
    }
    return n;
}
void whisper_amd_vad_timings(struct whisper_vad_context * vctx, int64_t out_us[3]) {
    out_us[0] = vctx->t_vad_us; out_us[1] = vctx->t_front_wait_us; out_us[2] = vctx->t_host_us;
}

int                  wa_vad_ctx_device(const whisper_vad_context * v) { return v->device; }
const wa_vad_model & wa_vad_ctx_model (const whisper_vad_context * v) { return v->model; }
const wa_vad_dev &   wa_vad_ctx_dev   (const whisper_vad_context * v) { return v->dev; }

// -------------------------------------------------------------------------------------------------
// whisper_full / whisper_full_parallel with vad = true (ref: whisper.cpp:6615-6793): the speech-only audio and the state's table
// -------------------------------------------------------------------------------------------------
// the state's VAD context (made from params.vad_model_path by the first call) over `samples`, host or device: its segments
bool wa_vad_segments_for(whisper_context * ctx, whisper_state * st, const whisper_full_params & params, const float * samples, int n_samples,
                         std::vector<wa_vad_seg> & segs) {
    segs.clear();
    st->vad_mapping_table.clear();
    st->has_vad_segments = false;
    if (!st->vad_context) {
        st->vad_context = wa_vad_create_from_file(params.vad_model_path, whisper_vad_default_context_params().n_threads, ctx->device);
        if (!st->vad_context) { WA_ERROR("%s: failed to initialize VAD context\n", __func__); return false; }
    }
    if (!whisper_vad_detect_speech(st->vad_context, samples, n_samples)) { WA_ERROR("%s: failed to detect speech\n", __func__); return false; }
    segs = wa_vad_segments_from_probs(st->vad_context->probs.data(), (int) st->vad_context->probs.size(), st->vad_context->model.n_window, params.vad_params);
    return true;
}

bool wa_vad_for_full(whisper_context * ctx, whisper_state * st, const whisper_full_params & params, const float * samples, int n_samples,
                     std::vector<float> & filtered) {
    WA_INFO("%s: VAD is enabled, processing speech segments only\n", __func__);
    std::vector<wa_vad_seg> segs;
    if (!wa_vad_segments_for(ctx, st, params, samples, n_samples, segs)) return false;
    filtered.clear();
    if (!segs.empty()) {
        st->has_vad_segments = true;
        wa_vad_filter_audio(segs, params.vad_params.samples_overlap, samples, n_samples, filtered, st->vad_mapping_table);
        WA_INFO("%s: %d speech segments, audio reduced from %d to %d samples, %d mapping points\n", __func__, (int) segs.size(), n_samples,
                (int) filtered.size(), (int) st->vad_mapping_table.size());
    }
    return true;
}

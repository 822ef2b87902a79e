// wa_tts.cpp - heuristic token timestamps (params.token_timestamps): where the windowed |PCM| energy and the records of the
// boundary scans (wa_tts.h) come from, and whisper_amd_signal_energy / whisper_amd_token_snap / whisper_amd_tts_stats of include/whisper_amd.h.
//
// The energy kernel runs over the call's PCM where it lies in HBM - device PCM in place, host PCM in the copy the mel front end staged - and
// its result stays in a buffer of the state.  Per finished segment one launch of the snap kernel turns the text tokens' sample ends into
// 24-byte records, which come back through pinned memory with one wait for the state's stream; wa_full.cpp finalises them.  Everything is
// issued on the state's stream and nothing waits for the device as a whole, so the members of a lock-step wave do not meet here.
// The same records come from the host functions of wa_tts.h under WHISPER_AMD_TTS_HOST=1 (read once per process) and after any failed
// launch, copy or allocation (logged, counted): device PCM is then copied back once for the call.
#include "wa_internal.h"
#include "wa_tts.h"

#include <cstring>

static_assert(sizeof(wa_tts_record) == 24 && sizeof(struct whisper_amd_tts_record) == 24, "a record is 24 bytes on both sides of the C boundary");

static bool tts_host_switch() {
    static const bool on = [] { const char * g = getenv("WHISPER_AMD_TTS_HOST"); return g && g[0] == '1'; }();
    return on;
}

void wa_tts_free(whisper_state & st) {
    if (st.d_energy) { (void) hipFree(st.d_energy); st.d_energy = nullptr; st.d_energy_cap = 0; }
    if (st.d_tts_io) { (void) hipFree(st.d_tts_io); st.d_tts_io = nullptr; st.d_tts_io_cap = 0; }
    if (st.h_tts_io) { (void) hipHostFree(st.h_tts_io); st.h_tts_io = nullptr; st.h_tts_io_cap = 0; }
    st.energy_n = 0;
}

// `samples` in host memory: the pointer itself, or a copy of device PCM in `keep` (one stream-ordered copy, counted); null: the copy failed
static const float * tts_host_pcm(whisper_state & st, const float * samples, int n, std::vector<float> & keep) {
    if (!wa_is_device_ptr(samples)) return samples;
    keep.resize((size_t) n);
    if (!WA_HIP_OK(hipMemcpyAsync(keep.data(), samples, (size_t) n * sizeof(float), hipMemcpyDeviceToHost, st.stream)) ||
        !WA_HIP_OK(hipStreamSynchronize(st.stream))) return nullptr;
    st.tts_pending = false;
    st.tts_bytes_d2h += (int64_t) n * (int64_t) sizeof(float);
    return keep.data();
}

// `samples` in device memory: the pointer itself, the copy the mel front end staged for this call (`staged_ok`: the caller stands right behind
// wa_mel_compute on these samples), or one upload into that staging buffer; null: the upload failed
static const float * tts_device_pcm(whisper_state & st, const float * samples, int n, bool staged_ok) {
    if (wa_is_device_ptr(samples)) return samples;
    if (staged_ok && st.d_pcm && st.d_pcm_n == n) return st.d_pcm;
    st.d_pcm_n = 0;
    if (!wa_dev_reserve(st.d_pcm, st.d_pcm_cap, (size_t) n)) return nullptr;
    if (!WA_HIP_OK(hipMemcpyAsync(st.d_pcm, samples, (size_t) n * sizeof(float), hipMemcpyHostToDevice, st.stream)) ||
        !WA_HIP_OK(hipStreamSynchronize(st.stream))) return nullptr;     // (the caller may release its buffer on return)
    st.d_pcm_n = n;
    return st.d_pcm;
}

// the energies of d_pcm[0, n) into st.d_energy, stream-ordered; nothing is waited for
static bool tts_energy_device(whisper_state & st, const float * d_pcm, int n) {
    if (!d_pcm || n > WA_TTS_MAX_N || !wa_dev_reserve(st.d_energy, st.d_energy_cap, (size_t) n)) return false;
    if (!wa_tts_energy_launch(st.stream, d_pcm, n, st.d_energy)) return false;
    st.tts_pending = true;
    st.n_tts_energy++;
    st.energy.clear();
    st.energy_n = n;
    return true;
}

static bool tts_energy_host(whisper_state & st, const float * samples, int n) {
    std::vector<float> keep;
    const float * pcm = tts_host_pcm(st, samples, n, keep);
    if (!pcm) return false;
    st.energy = wa_signal_energy(pcm, n, WA_TTS_HALF);
    st.energy_n = 0;
    return true;
}

bool wa_tts_begin(whisper_state & st, const float * samples, int n_samples) {
    st.tts_pcm = samples; st.tts_pcm_n = n_samples;
    if (!tts_host_switch()) {
        if (tts_energy_device(st, tts_device_pcm(st, samples, n_samples, true), n_samples)) return true;
        st.n_tts_fallback++;
        WA_WARN("%s: the device path failed, taking the host path\n", __func__);
    }
    return tts_energy_host(st, samples, n_samples);
}

bool wa_tts_have_energy(const whisper_state & st) { return st.energy_n > 0 || !st.energy.empty(); }
int  wa_tts_n_samples(const whisper_state & st) { return st.energy_n > 0 ? st.energy_n : (int) st.energy.size(); }

void wa_tts_end(whisper_state & st) {
    if (st.tts_pending) { (void) hipStreamSynchronize(st.stream); st.tts_pending = false; }   // the caller's PCM is read no longer
    st.tts_pcm = nullptr; st.tts_pcm_n = 0;
}

static size_t tts_pad256(size_t n) { return (n + 255) / 256 * 256; }

// k_tts_snap over st.d_energy on the state's stream: token ends up, records down, one stream synchronise
static bool tts_snap_device(whisper_state & st, const int32_t * s_lo, const int32_t * s_hi, const int32_t * has_prev, int n_tokens, wa_tts_record * out) {
    const size_t n_tok = (size_t) n_tokens * sizeof(int32_t), o_rec = tts_pad256(3 * n_tok), need = o_rec + (size_t) n_tokens * sizeof(wa_tts_record);
    if (!wa_dev_reserve(st.d_tts_io, st.d_tts_io_cap, need)) return false;
    if (need > st.h_tts_io_cap) {
        if (st.h_tts_io) { (void) hipHostFree(st.h_tts_io); st.h_tts_io = nullptr; st.h_tts_io_cap = 0; }
        if (!WA_HIP_OK(hipHostMalloc((void **) &st.h_tts_io, need))) { st.h_tts_io = nullptr; return false; }
        st.h_tts_io_cap = need;
    }
    hipStream_t s = st.stream;
    memcpy(st.h_tts_io, s_lo, n_tok); memcpy(st.h_tts_io + n_tok, s_hi, n_tok); memcpy(st.h_tts_io + 2 * n_tok, has_prev, n_tok);
    auto * d_rec = (wa_tts_record *) (st.d_tts_io + o_rec);
    if (!WA_HIP_OK(hipMemcpyAsync(st.d_tts_io, st.h_tts_io, 3 * n_tok, hipMemcpyHostToDevice, s))) return false;
    const bool launched = wa_tts_snap_launch(s, st.d_energy, st.energy_n, (const int32_t *) st.d_tts_io, n_tokens, d_rec);
    const bool copied = launched && WA_HIP_OK(hipMemcpyAsync(st.h_tts_io + o_rec, d_rec, (size_t) n_tokens * sizeof(wa_tts_record), hipMemcpyDeviceToHost, s));
    if (!WA_HIP_OK(hipStreamSynchronize(s)) || !copied) return false;
    st.tts_pending = false;
    memcpy(out, st.h_tts_io + o_rec, (size_t) n_tokens * sizeof(wa_tts_record));
    st.n_tts_snap++;
    return true;
}

bool wa_tts_records(whisper_state & st, const int32_t * s_lo, const int32_t * s_hi, const int32_t * has_prev, int n_tokens, wa_tts_record * out) {
    if (n_tokens <= 0) return true;
    if (st.energy_n > 0) {
        if (tts_snap_device(st, s_lo, s_hi, has_prev, n_tokens, out)) return true;
        st.n_tts_fallback++;
        WA_WARN("%s: the device path failed, taking the host path for the rest of the call\n", __func__);
        if (!st.tts_pcm || st.tts_pcm_n != st.energy_n || !tts_energy_host(st, st.tts_pcm, st.tts_pcm_n)) return false;
    }
    if (st.energy.empty()) return false;
    for (int j = 0; j < n_tokens; ++j) out[j] = wa_tts_record_host(st.energy.data(), (int) st.energy.size(), s_lo[j], s_hi[j], has_prev[j] != 0);
    return true;
}

// ---- the two steps alone (include/whisper_amd.h) ----
static int tts_entry_energy(struct whisper_state * st, const float * pcm, int n, int where, std::vector<float> & host_e) {
    if (!st || !pcm || n <= 0 || n > WA_TTS_MAX_N || (where != 0 && where != 1)) return WHISPER_AMD_TTS_REFUSED;
    if (!st->ctx || !WA_HIP_OK(hipSetDevice(st->ctx->device))) return WHISPER_AMD_TTS_HIP_ERROR;
    if (where == 0) {
        std::vector<float> keep;
        const float * h = tts_host_pcm(*st, pcm, n, keep);
        if (!h) return WHISPER_AMD_TTS_HIP_ERROR;
        host_e = wa_signal_energy(h, n, WA_TTS_HALF);
        return 0;
    }
    return tts_energy_device(*st, tts_device_pcm(*st, pcm, n, false), n) ? 0 : WHISPER_AMD_TTS_HIP_ERROR;
}

int whisper_amd_signal_energy(struct whisper_state * st, const float * pcm, int n, int where, float * out) {
    return wa_guard(__func__, WHISPER_AMD_TTS_HIP_ERROR, [&]() -> int {
        if (!out) return WHISPER_AMD_TTS_REFUSED;
        std::vector<float> e;
        const int rc = tts_entry_energy(st, pcm, n, where, e);
        if (rc != 0) return rc;
        if (where == 0) { memcpy(out, e.data(), (size_t) n * sizeof(float)); return 0; }
        const bool ok = WA_HIP_OK(hipMemcpyAsync(out, st->d_energy, (size_t) n * sizeof(float), hipMemcpyDeviceToHost, st->stream)) &&
                        WA_HIP_OK(hipStreamSynchronize(st->stream));
        st->tts_pending = false;
        return ok ? 0 : WHISPER_AMD_TTS_HIP_ERROR;
    });
}

int whisper_amd_token_snap(struct whisper_state * st, const float * pcm, int n, const int32_t * s_lo, const int32_t * s_hi, const int32_t * has_prev,
                           int n_tokens, int where, struct whisper_amd_tts_record * records_out) {
    return wa_guard(__func__, WHISPER_AMD_TTS_HIP_ERROR, [&]() -> int {
        if (!s_lo || !s_hi || !has_prev || !records_out || n_tokens <= 0) return WHISPER_AMD_TTS_REFUSED;
        for (int j = 0; j < n_tokens; ++j) if (s_lo[j] < 0 || s_lo[j] >= n || s_hi[j] < 0 || s_hi[j] >= n) return WHISPER_AMD_TTS_REFUSED;
        std::vector<float> e;
        const int rc = tts_entry_energy(st, pcm, n, where, e);
        if (rc != 0) return rc;
        std::vector<wa_tts_record> rec((size_t) n_tokens);
        if (where == 0) for (int j = 0; j < n_tokens; ++j) rec[j] = wa_tts_record_host(e.data(), n, s_lo[j], s_hi[j], has_prev[j] != 0);
        else if (!tts_snap_device(*st, s_lo, s_hi, has_prev, n_tokens, rec.data())) return WHISPER_AMD_TTS_HIP_ERROR;
        memcpy(records_out, rec.data(), (size_t) n_tokens * sizeof(wa_tts_record));
        return 0;
    });
}

void whisper_amd_tts_stats(struct whisper_state * st, int64_t out[4]) {
    out[0] = st->n_tts_energy; out[1] = st->n_tts_snap; out[2] = st->n_tts_fallback; out[3] = st->tts_bytes_d2h;
}

int whisper_amd_tts_tile(void) { return WA_TTS_TILE; }

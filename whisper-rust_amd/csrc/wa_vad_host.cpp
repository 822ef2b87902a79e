// wa_vad_host.cpp - VAD host part (wa_vad.h): model parser, LSTM recurrence, speech segments, speech-only audio and time mapping.
// Plain C++; every floating-point operation below is one the reference performs, in its order.  Built with -ffp-contract=off: the
// only fused multiply-adds are the written ones (the W_hh h chains, which ggml_vec_dot_f32 forms with vfmadd on an AVX2 build).
#include "wa_vad.h"
#include "wa_long_plan.h"

#include <immintrin.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

// -------------------------------------------------------------------------------------------------
// model file (ref: whisper.cpp:4775-5098): magic, type string, 3 version ints, n_window, n_context, layer table, 4 ints, tensors
// -------------------------------------------------------------------------------------------------
static const char * WA_VAD_SHAPE =
    "supported: n_window 512, 4 encoder layers (129->128, 128->64, 64->64, 64->128, kernel 3), lstm 128/128, final conv 128->1, "
    "F16 stft basis [256,1,258] and conv weights, F32 LSTM weights and biases";

namespace {
struct vad_reader {
    whisper_model_loader * l;
    bool ok = true;
    bool bytes(void * dst, size_t n) {
        if (!ok) return false;
        if (n && l->read(l->context, dst, n) != n) ok = false;
        return ok;
    }
    bool i32(int32_t & v) { return bytes(&v, 4); }
};
struct vad_slot { const char * name; int type; int ne[3]; void * dst; size_t n; };
}

bool wa_vad_model_load(whisper_model_loader * loader, wa_vad_model & m, std::string & err) {
    vad_reader r{ loader };
    auto refuse = [&](const std::string & what) { err = what + " (" + WA_VAD_SHAPE + ")"; return false; };
    uint32_t magic = 0;
    if (!r.bytes(&magic, 4) || magic != 0x67676d6c) { err = "invalid model data (bad magic)"; return false; }
    int32_t len = 0;
    if (!r.i32(len) || len < 0 || len > 256) return refuse("truncated or malformed header");
    m.type.resize(len);
    int32_t ver[3] = { 0, 0, 0 };
    if (!r.bytes(&m.type[0], len) || !r.i32(ver[0]) || !r.i32(ver[1]) || !r.i32(ver[2]) || !r.i32(m.n_window) || !r.i32(m.n_context))
        return refuse("truncated header");
    m.version = std::to_string(ver[0]) + "." + std::to_string(ver[1]) + "." + std::to_string(ver[2]);
    int32_t n_layers = 0;
    if (!r.i32(n_layers)) return refuse("truncated header");
    if (m.n_window != WA_VAD_WINDOW || n_layers != 4) return refuse("unsupported n_window / number of encoder layers");
    for (int i = 0; i < 4; ++i) {
        int32_t cin = 0, cout = 0, ks = 0;
        if (!r.i32(cin) || !r.i32(cout) || !r.i32(ks)) return refuse("truncated layer table");
        if (cin != WA_VAD_ENC_IN[i] || cout != WA_VAD_ENC_OUT[i] || ks != 3) return refuse("unsupported encoder layer " + std::to_string(i));
    }
    int32_t tail[4] = { 0, 0, 0, 0 };
    for (int i = 0; i < 4; ++i) if (!r.i32(tail[i])) return refuse("truncated header");
    if (tail[0] != WA_VAD_HOP || tail[1] != WA_VAD_HID || tail[2] != WA_VAD_HID || tail[3] != 1) return refuse("unsupported LSTM / final conv sizes");

    m.stft.assign((size_t) 2 * WA_VAD_BINS * WA_VAD_NFFT, 0);
    for (int i = 0; i < 4; ++i) { m.enc_w[i].assign((size_t) WA_VAD_ENC_OUT[i] * WA_VAD_ENC_IN[i] * 3, 0); m.enc_b[i].assign(WA_VAD_ENC_OUT[i], 0.0f); }
    m.w_ih.assign((size_t) WA_VAD_GATES * WA_VAD_HID, 0.0f); m.w_hh = m.w_ih;
    m.b_ih.assign(WA_VAD_GATES, 0.0f); m.b_hh = m.b_ih;
    m.w_f.assign(WA_VAD_HID, 0);
    vad_slot slots[15] = {
        { "_model.stft.forward_basis_buffer",     1, { WA_VAD_NFFT, 1, 2 * WA_VAD_BINS }, m.stft.data(), m.stft.size() },
        { "_model.encoder.0.reparam_conv.weight", 1, { 3, 129, 128 }, m.enc_w[0].data(), m.enc_w[0].size() },
        { "_model.encoder.0.reparam_conv.bias",   0, { 128, 1, 1 },   m.enc_b[0].data(), 128 },
        { "_model.encoder.1.reparam_conv.weight", 1, { 3, 128, 64 },  m.enc_w[1].data(), m.enc_w[1].size() },
        { "_model.encoder.1.reparam_conv.bias",   0, { 64, 1, 1 },    m.enc_b[1].data(), 64 },
        { "_model.encoder.2.reparam_conv.weight", 1, { 3, 64, 64 },   m.enc_w[2].data(), m.enc_w[2].size() },
        { "_model.encoder.2.reparam_conv.bias",   0, { 64, 1, 1 },    m.enc_b[2].data(), 64 },
        { "_model.encoder.3.reparam_conv.weight", 1, { 3, 64, 128 },  m.enc_w[3].data(), m.enc_w[3].size() },
        { "_model.encoder.3.reparam_conv.bias",   0, { 128, 1, 1 },   m.enc_b[3].data(), 128 },
        { "_model.decoder.rnn.weight_ih",         0, { 128, 512, 1 }, m.w_ih.data(), m.w_ih.size() },
        { "_model.decoder.rnn.weight_hh",         0, { 128, 512, 1 }, m.w_hh.data(), m.w_hh.size() },
        { "_model.decoder.rnn.bias_ih",           0, { 512, 1, 1 },   m.b_ih.data(), 512 },
        { "_model.decoder.rnn.bias_hh",           0, { 512, 1, 1 },   m.b_hh.data(), 512 },
        { "_model.decoder.decoder.2.weight",      1, { 128, 1, 1 },   m.w_f.data(), 128 },
        { "_model.decoder.decoder.2.bias",        0, { 1, 1, 1 },     &m.b_f, 1 },
    };
    bool seen[15] = { false };
    int n_loaded = 0;
    for (;;) {
        int32_t n_dims = 0, length = 0, ttype = 0;
        if (!r.i32(n_dims)) break;                                  // end of file
        if (loader->eof && loader->eof(loader->context)) break;
        if (!r.i32(length) || !r.i32(ttype)) return refuse("truncated tensor record");
        if (n_dims < 1 || n_dims > 3 || length < 1 || length > 256) return refuse("malformed tensor record");
        int32_t ne[3] = { 1, 1, 1 };
        for (int i = 0; i < n_dims; ++i) if (!r.i32(ne[i])) return refuse("truncated tensor record");
        std::string name((size_t) length, '\0');
        if (!r.bytes(&name[0], (size_t) length)) return refuse("truncated tensor record");
        int k = -1;
        for (int i = 0; i < 15; ++i) if (name == slots[i].name) k = i;
        if (k < 0) return refuse("unknown tensor '" + name + "'");
        const vad_slot & s = slots[k];
        if (seen[k]) return refuse("tensor '" + name + "' appears twice");
        if (ne[0] != s.ne[0] || ne[1] != s.ne[1] || ne[2] != s.ne[2] || ttype != s.type) return refuse("tensor '" + name + "' has an unsupported shape or type");
        if (!r.bytes(s.dst, s.n * (s.type == 1 ? 2 : 4))) return refuse("tensor '" + name + "' is truncated");
        seen[k] = true; ++n_loaded;
    }
    if (n_loaded != 15) {
        std::string missing;
        for (int i = 0; i < 15; ++i) if (!seen[i]) { missing = slots[i].name; break; }
        return refuse(n_loaded == 0 ? std::string("the file holds no tensors") : "tensor '" + missing + "' is missing");
    }
    return true;
}

// -------------------------------------------------------------------------------------------------
// recurrence (ref: whisper.cpp:4582-4625, 4655-4658; ggml_vec_dot_f32 / _f16 of the AVX2 build: 32 FMA chains s[k mod 32] in k order,
// then (s[l] + s[16+l]) + (s[8+l] + s[24+l]) per lane l, lanes l and l+4 added, two horizontal adds)
// -------------------------------------------------------------------------------------------------
static inline float tree32(const float * s) {
    float a[8];
    for (int l = 0; l < 8; ++l) a[l] = (s[l] + s[16 + l]) + (s[8 + l] + s[24 + l]);
    const float t0 = a[0] + a[4], t1 = a[1] + a[5], t2 = a[2] + a[6], t3 = a[3] + a[7];
    return (t0 + t1) + (t2 + t3);
}

static void hid_gates_scalar(const float * w, const float * h, float * out) {
    for (int r = 0; r < WA_VAD_GATES; ++r) {
        float s[32];
        for (int i = 0; i < 32; ++i) s[i] = 0.0f;
        const float * wr = w + (size_t) r * WA_VAD_HID;
        for (int k = 0; k < WA_VAD_HID; ++k) s[k & 31] = fmaf(wr[k], h[k], s[k & 31]);
        out[r] = tree32(s);
    }
}

__attribute__((target("avx2,fma"))) static void hid_gates_avx2(const float * w, const float * h, float * out) {
    __m256 hv[16];
    for (int i = 0; i < 16; ++i) hv[i] = _mm256_loadu_ps(h + 8 * i);
    for (int r = 0; r < WA_VAD_GATES; ++r) {
        const float * wr = w + (size_t) r * WA_VAD_HID;
        __m256 s0 = _mm256_setzero_ps(), s1 = s0, s2 = s0, s3 = s0;
        for (int i = 0; i < 16; i += 4) {
            s0 = _mm256_fmadd_ps(_mm256_loadu_ps(wr + 8 * i),      hv[i],     s0);
            s1 = _mm256_fmadd_ps(_mm256_loadu_ps(wr + 8 * i + 8),  hv[i + 1], s1);
            s2 = _mm256_fmadd_ps(_mm256_loadu_ps(wr + 8 * i + 16), hv[i + 2], s2);
            s3 = _mm256_fmadd_ps(_mm256_loadu_ps(wr + 8 * i + 24), hv[i + 3], s3);
        }
        const __m256 a = _mm256_add_ps(_mm256_add_ps(s0, s2), _mm256_add_ps(s1, s3));
        __m128 t = _mm_add_ps(_mm256_castps256_ps128(a), _mm256_extractf128_ps(a, 1));
        t = _mm_hadd_ps(t, t);
        t = _mm_hadd_ps(t, t);
        out[r] = _mm_cvtss_f32(t);
    }
}

// F16 <-> F32 on bit patterns (no _Float16 in older g++): exact, and round-to-nearest-even as _cvtss_sh in the reference's im2col
static inline float f16_to_f32(uint16_t u) {
    const uint32_t sign = (uint32_t) (u & 0x8000) << 16, em = u & 0x7fff;
    uint32_t x;
    if (em >= 0x7c00) x = sign | 0x7f800000u | ((em & 0x3ff) << 13);
    else if (em >= 0x0400) x = sign | ((em << 13) + ((127 - 15) << 23));
    else { const float f = (float) em * (1.0f / 16777216.0f); memcpy(&x, &f, 4); x |= sign; }     // subnormal: em 2^-24, exact
    float r; memcpy(&r, &x, 4); return r;
}
static inline uint16_t f32_to_f16(float v) {
    uint32_t x; memcpy(&x, &v, 4);
    const uint32_t sign = x & 0x80000000u; x ^= sign;
    uint32_t o;
    if (x >= ((127u + 16u) << 23)) o = x > 0x7f800000u ? 0x7e00 : 0x7c00;
    else if (x < (113u << 23)) {                       // result is subnormal: the F32 add does the rounding
        const uint32_t magic = ((127u - 15u) + (23u - 10u) + 1u) << 23;
        float f, mf; memcpy(&f, &x, 4); memcpy(&mf, &magic, 4);
        f += mf; memcpy(&x, &f, 4); o = x - magic;
    } else {
        const uint32_t odd = (x >> 13) & 1;
        x += ((uint32_t) (15 - 127) << 23) + 0xfff; x += odd; o = x >> 13;
    }
    return (uint16_t) (o | (sign >> 16));
}
static inline float round_f16(float v) { return f16_to_f32(f32_to_f16(v)); }
static inline float sigmoidf_ref(float x) { return 1.f / (1.f + expf(-x)); }                      // unary-ops.cpp:31

float wa_vad_step(const wa_vad_model & m, wa_vad_lstm & st, const float * gate_in) {
    static const bool simd = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    float hid[WA_VAD_GATES];
    if (simd) hid_gates_avx2(m.w_hh.data(), st.h, hid); else hid_gates_scalar(m.w_hh.data(), st.h, hid);
    float s[32];
    for (int i = 0; i < 32; ++i) s[i] = 0.0f;
    for (int j = 0; j < WA_VAD_HID; ++j) {
        const float gi = gate_in[j]                  + (hid[j]                  + m.b_hh[j]);
        const float gf = gate_in[WA_VAD_HID + j]     + (hid[WA_VAD_HID + j]     + m.b_hh[WA_VAD_HID + j]);
        const float gg = gate_in[2 * WA_VAD_HID + j] + (hid[2 * WA_VAD_HID + j] + m.b_hh[2 * WA_VAD_HID + j]);
        const float go = gate_in[3 * WA_VAD_HID + j] + (hid[3 * WA_VAD_HID + j] + m.b_hh[3 * WA_VAD_HID + j]);
        const float i_t = sigmoidf_ref(gi), f_t = sigmoidf_ref(gf), g_t = tanhf(gg), o_t = sigmoidf_ref(go);
        const float fc = f_t * st.c[j], ig = i_t * g_t;
        const float c = fc + ig;
        const float h = o_t * tanhf(c);
        st.c[j] = c;
        st.h[j] = h;
        // the output dot (K = 128, F16 operands): relu(h) rounded to F16 once by the final conv's im2col
        const float x = round_f16(h > 0.f ? h : 0.f);
        s[j & 31] = fmaf(x, f16_to_f32(m.w_f[j]), s[j & 31]);
    }
    return sigmoidf_ref(tree32(s) + m.b_f);
}

// -------------------------------------------------------------------------------------------------
// speech segments (ref: whisper.cpp:5202-5436), integer for integer
// -------------------------------------------------------------------------------------------------
static int     cs_to_samples(int64_t cs)  { return wa_vad_cs_to_samples(cs); }
static int64_t samples_to_cs(int samples) { return wa_vad_samples_to_cs(samples); }

std::vector<wa_vad_seg> wa_vad_segments_from_probs(const float * probs, int n_probs, int n_window, const whisper_vad_params & params) {
    const float threshold               = params.threshold;
    const int   min_speech_duration_ms  = params.min_speech_duration_ms;
    const int   min_silence_duration_ms = params.min_silence_duration_ms;
    const float max_speech_duration_s   = params.max_speech_duration_s;
    const int   speech_pad_ms           = params.speech_pad_ms;
    const int   sample_rate             = WHISPER_SAMPLE_RATE;
    const int   min_silence_samples     = sample_rate * min_silence_duration_ms / 1000;
    const int   audio_length_samples    = n_probs * n_window;
    const int   min_speech_samples      = sample_rate * min_speech_duration_ms / 1000;
    const int   speech_pad_samples      = sample_rate * speech_pad_ms / 1000;

    int max_speech_samples;
    if (max_speech_duration_s > 100000.0f) {
        max_speech_samples = INT_MAX / 2;
    } else {
        const int64_t temp = (int64_t) sample_rate * (int64_t) (max_speech_duration_s) - n_window - 2 * speech_pad_samples;
        max_speech_samples = (temp > INT_MAX) ? INT_MAX / 2 : (int) temp;
        if (max_speech_samples < 0) max_speech_samples = INT_MAX / 2;
    }
    const int min_silence_samples_at_max_speech = sample_rate * 98 / 1000;

    float neg_threshold = threshold - 0.15f;
    if (neg_threshold < 0.01f) neg_threshold = 0.01f;

    struct speech { int start, end; };
    std::vector<speech> speeches;
    bool is_speech_segment = false, has_curr_speech = false;
    int  temp_end = 0, prev_end = 0, next_start = 0, curr_speech_start = 0;

    for (int i = 0; i < n_probs; i++) {
        const float curr_prob   = probs[i];
        const int   curr_sample = n_window * i;

        if ((curr_prob >= threshold) && temp_end) {
            temp_end = 0;
            if (next_start < prev_end) next_start = curr_sample;
        }
        if ((curr_prob >= threshold) && !is_speech_segment) {
            is_speech_segment = true;
            curr_speech_start = curr_sample;
            has_curr_speech = true;
            continue;
        }
        if (is_speech_segment && (curr_sample - curr_speech_start) > max_speech_samples) {
            if (prev_end) {
                speeches.push_back({ curr_speech_start, prev_end });
                has_curr_speech = true;
                if (next_start < prev_end) { is_speech_segment = false; has_curr_speech = false; }
                else curr_speech_start = next_start;
                prev_end = next_start = temp_end = 0;
            } else {
                speeches.push_back({ curr_speech_start, curr_sample });
                prev_end = next_start = temp_end = 0;
                is_speech_segment = false;
                has_curr_speech = false;
                continue;
            }
        }
        if ((curr_prob < neg_threshold) && is_speech_segment) {
            if (!temp_end) temp_end = curr_sample;
            if ((curr_sample - temp_end) > min_silence_samples_at_max_speech) prev_end = temp_end;
            if ((curr_sample - temp_end) < min_silence_samples) continue;
            if ((temp_end - curr_speech_start) > min_speech_samples) speeches.push_back({ curr_speech_start, temp_end });
            prev_end = next_start = temp_end = 0;
            is_speech_segment = false;
            has_curr_speech = false;
            continue;
        }
    }
    if (has_curr_speech && (audio_length_samples - curr_speech_start) > min_speech_samples) speeches.push_back({ curr_speech_start, audio_length_samples });

    // merge neighbours less than 200 ms apart
    if (speeches.size() > 1) {
        for (int i = 0; i < (int) speeches.size() - 1; i++) {
            const int max_merge_gap_samples = sample_rate * 200 / 1000;
            if (speeches[i + 1].start - speeches[i].end < max_merge_gap_samples) {
                speeches[i].end = speeches[i + 1].end;
                speeches.erase(speeches.begin() + i + 1);
                i--;
            }
        }
    }
    for (int i = 0; i < (int) speeches.size(); i++) {
        if (speeches[i].end - speeches[i].start < min_speech_samples) { speeches.erase(speeches.begin() + i); i--; }
    }

    std::vector<wa_vad_seg> segments(speeches.size());
    for (int i = 0; i < (int) speeches.size(); i++) {
        if (i == 0) speeches[i].start = (speeches[i].start > speech_pad_samples) ? (speeches[i].start - speech_pad_samples) : 0;
        if (i < (int) speeches.size() - 1) {
            const int silence_duration = speeches[i + 1].start - speeches[i].end;
            if (silence_duration < 2 * speech_pad_samples) {
                speeches[i].end += silence_duration / 2;
                speeches[i + 1].start = (speeches[i + 1].start > silence_duration / 2) ? (speeches[i + 1].start - silence_duration / 2) : 0;
            } else {
                speeches[i].end = (speeches[i].end + speech_pad_samples < audio_length_samples) ? (speeches[i].end + speech_pad_samples) : audio_length_samples;
                speeches[i + 1].start = (speeches[i + 1].start > speech_pad_samples) ? (speeches[i + 1].start - speech_pad_samples) : 0;
            }
        } else {
            speeches[i].end = (speeches[i].end + speech_pad_samples < audio_length_samples) ? (speeches[i].end + speech_pad_samples) : audio_length_samples;
        }
        segments[i].start = samples_to_cs(speeches[i].start);
        segments[i].end   = samples_to_cs(speeches[i].end);
    }
    return segments;
}

// -------------------------------------------------------------------------------------------------
// speech-only audio + time mapping (ref: whisper.cpp:6644-6790, 7882-7921)
// -------------------------------------------------------------------------------------------------
void wa_vad_filter_audio(const std::vector<wa_vad_seg> & segs, float samples_overlap, const float * samples, int n_samples,
                         std::vector<float> & filtered, std::vector<wa_vad_map_point> & table) {
    filtered.clear();
    table.clear();
    if (segs.empty()) return;
    // lengths, pieces and table: wa_long_plan.h states them once, for this copy and for the device's (wa_long.hip).  The length handed to the
    // transcription is the reference's; the sample a last segment reaching the end of the audio would copy past it is cut off.
    std::vector<wa_long_piece> pieces;
    const int total = wa_vad_layout_make(segs.data(), (int) segs.size(), samples_overlap, n_samples, &pieces, &table);
    std::vector<float> buf((size_t) total, 0.0f);
    for (const wa_long_piece & p : pieces)
        if (p.src >= 0) memcpy(buf.data() + p.dst, samples + p.src, (size_t) p.len * sizeof(float));
    filtered.swap(buf);
}

int64_t wa_vad_map_time(int64_t processed_time, const std::vector<wa_vad_map_point> & table) {
    if (table.empty()) return processed_time;
    if (processed_time <= table.front().processed_time) return table.front().original_time;
    if (processed_time >= table.back().processed_time)  return table.back().original_time;
    auto upper = std::lower_bound(table.begin(), table.end(), processed_time,
                                  [](const wa_vad_map_point & e, int64_t t) { return e.processed_time < t; });
    if (upper->processed_time == processed_time) return upper->original_time;
    auto lower = upper - 1;
    const int64_t processed_diff = upper->processed_time - lower->processed_time;
    const int64_t original_diff  = upper->original_time - lower->original_time;
    const int64_t offset         = processed_time - lower->processed_time;
    if (processed_diff == 0) return lower->original_time;
    return lower->original_time + (offset * original_diff) / processed_diff;
}

// wa_audio.h - audio front end: int16 or F32 PCM, one or two channels, 8 .. 192 kHz -> 16 kHz mono F32.
//
// Plain C++ (no HIP, no device types): tests/native/audio_math.cpp compiles this header alone with g++.  It holds the filter plan, the
// filter taps and wa_audio_ref, the host restatement of conversion plus resampling that the kernels of wa_audio.hip are held to bit for
// bit and that serves a call whose HIP path fails (wa_audio.cpp).
//
// Rates: g = gcd(R, 16000), L = 16000 / g, M = R / g; accepted: 8000 <= R <= 192000 with L <= 640 (8, 11.025, 12, 16, 22.05, 24, 32,
// 44.1, 48, 88.2, 96, 176.4, 192 kHz among them).  R == 16000 takes no filter.
// Prototype: a Kaiser-windowed sinc on the grid of rate R L = 16000 M, WA_AUDIO_ZEROS zero crossings of the window's span per side counted
// at the lower of the two rates, beta WA_AUDIO_BETA, the cut-off below the lower rate's Nyquist frequency by WA_AUDIO_ROLL of it so that
// the stop band starts AT that frequency; computed in double, scaled by L, rounded once to F32, stored phase-major taps[L][K] with
// K = 2 Z ceil(max(L, M) / L) taps per phase.
// One output sample n: t = n M, p = t mod L, i0 = t / L, y[n] = the F32 fmaf chain over k = 0 .. K-1 ascending of
// taps[p][k] * x[i0 - K/2 + 1 + k] from 0.0f, x zero outside the input; ceil(n_frames 16000 / R) outputs.
// Sample conversion, every operation rounded on its own: I16 mono (float) s / 32768.0f; F32 stereo (l + r) / 2.0f;
// I16 stereo ((float) l + (float) r) / 2.0f / 32768.0f.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#define WA_AUDIO_RATE   16000      // output rate
#define WA_AUDIO_ZEROS  32         // Z
#define WA_AUDIO_BETA   11.0
#define WA_AUDIO_ROLL   0.115      // cut-off = (1 - ROLL) x the lower rate's Nyquist frequency
#define WA_AUDIO_MAX_L  640
#define WA_AUDIO_I16    0          // = WHISPER_AMD_PCM_I16
#define WA_AUDIO_F32    1          // = WHISPER_AMD_PCM_F32

// device kernel k_audio_resample (wa_audio.hip): outputs per workgroup (exported: whisper_amd_audio_tile) and the floats of LDS it owns
#define WA_AUDIO_TILE   1024
#define WA_AUDIO_LDS    14336

struct wa_audio_plan { int rate = 0, L = 0, M = 0, K = 0; };      // K == 0: rate == 16000, no filter

inline bool wa_audio_plan_make(int rate, wa_audio_plan & p) {
    if (rate < 8000 || rate > 192000) return false;
    int a = rate, b = WA_AUDIO_RATE;
    while (b) { const int r = a % b; a = b; b = r; }
    const int L = WA_AUDIO_RATE / a, M = rate / a;
    if (L > WA_AUDIO_MAX_L) return false;
    const int q = L > M ? L : M;
    p.rate = rate; p.L = L; p.M = M;
    p.K = rate == WA_AUDIO_RATE ? 0 : 2 * WA_AUDIO_ZEROS * ((q + L - 1) / L);
    return true;
}

inline bool wa_audio_args_ok(const void * data, int64_t n_frames, int channels, int rate, int format) {
    wa_audio_plan p;
    return n_frames >= 0 && (data || n_frames == 0) && (channels == 1 || channels == 2) && (format == WA_AUDIO_I16 || format == WA_AUDIO_F32) &&
           wa_audio_plan_make(rate, p) && n_frames <= INT64_MAX / WA_AUDIO_MAX_L;
}

// ceil(n_frames 16000 / R) = ceil(n_frames L / M); -1: refused
inline int64_t wa_audio_n_out(int64_t n_frames, int rate) {
    wa_audio_plan p;
    if (n_frames < 0 || n_frames > INT64_MAX / WA_AUDIO_MAX_L || !wa_audio_plan_make(rate, p)) return -1;
    return (n_frames * p.L + p.M - 1) / p.M;
}

// input frames a tile of WA_AUDIO_TILE outputs reads (the kernel's LDS span): the first taps of its last output lie at most
// ((TILE - 1) M + L - 1) / L frames behind those of its first
inline int wa_audio_span(const wa_audio_plan & p) { return (int) (((int64_t) (WA_AUDIO_TILE - 1) * p.M + p.L - 1) / p.L) + p.K; }

inline double wa_audio_bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double) k * (double) k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

// taps[L][K]; empty for 16 kHz
inline void wa_audio_taps(const wa_audio_plan & p, std::vector<float> & taps) {
    taps.assign((size_t) p.L * p.K, 0.0f);
    if (!p.K) return;
    const double pi = 3.14159265358979323846;
    const int    q  = p.L > p.M ? p.L : p.M;                       // fine-grid samples per sample of the lower rate
    const double W  = (double) WA_AUDIO_ZEROS * q;                 // half width of the window on the fine grid
    const double fc = 0.5 * (1.0 - WA_AUDIO_ROLL) / q;             // cut-off in cycles per fine-grid sample
    const double i0b = wa_audio_bessel_i0(WA_AUDIO_BETA);
    for (int ph = 0; ph < p.L; ++ph)
        for (int k = 0; k < p.K; ++k) {
            const double tau = (double) ((int64_t) (p.K / 2 - 1 - k) * p.L + ph);      // output instant minus input instant
            const double r = tau / W;
            double h = 0.0;
            if (r > -1.0 && r < 1.0) {
                const double a = 2.0 * fc * tau;
                const double s = a == 0.0 ? 1.0 : std::sin(pi * a) / (pi * a);
                h = (double) p.L * 2.0 * fc * s * wa_audio_bessel_i0(WA_AUDIO_BETA * std::sqrt(1.0 - r * r)) / i0b;
            }
            taps[(size_t) ph * p.K + k] = (float) h;
        }
}

// frame i as mono F32
inline float wa_audio_frame(const void * data, int64_t i, int channels, int format) {
    if (format == WA_AUDIO_I16) {
        const int16_t * s = (const int16_t *) data;
        if (channels == 1) return (float) s[i] / 32768.0f;
        const float sum = (float) s[2 * i] + (float) s[2 * i + 1];
        const float mid = sum / 2.0f;
        return mid / 32768.0f;
    }
    const float * f = (const float *) data;
    if (channels == 1) return f[i];
    const float sum = f[2 * i] + f[2 * i + 1];
    return sum / 2.0f;
}

// Conversion plus resampling on the host: `out` receives wa_audio_n_out(n_frames, rate) samples; returns that count, -1 on refused arguments.
// `taps`: the table of wa_audio_taps for this rate, or null to build it here.
inline int64_t wa_audio_ref(const void * data, int64_t n_frames, int channels, int rate, int format, const float * taps, float * out) {
    if (!wa_audio_args_ok(data, n_frames, channels, rate, format)) return -1;
    wa_audio_plan p;
    wa_audio_plan_make(rate, p);
    const int64_t n_out = wa_audio_n_out(n_frames, rate);
    if (!p.K) {
        for (int64_t i = 0; i < n_frames; ++i) out[i] = wa_audio_frame(data, i, channels, format);
        return n_out;
    }
    std::vector<float> own;
    if (!taps) { wa_audio_taps(p, own); taps = own.data(); }
    // mono F32 with K zeros on both sides: the chain reads x[i0 - K/2 + 1 .. i0 + K/2]
    std::vector<float> x((size_t) n_frames + 2 * (size_t) p.K, 0.0f);
    for (int64_t i = 0; i < n_frames; ++i) x[(size_t) (i + p.K)] = wa_audio_frame(data, i, channels, format);
    for (int64_t n = 0; n < n_out; ++n) {
        const int64_t t = n * p.M, i0 = t / p.L;
        const float * h = taps + (size_t) (t % p.L) * p.K, * xs = x.data() + (size_t) (i0 - p.K / 2 + 1 + p.K);
        float acc = 0.0f;
        for (int k = 0; k < p.K; ++k) acc = std::fmaf(h[k], xs[k], acc);
        out[n] = acc;
    }
    return n_out;
}

// -------------------------------------------------------------------------------------------------
// device front end (wa_audio.hip).  No HIP types here: the stream travels as void *.
// -------------------------------------------------------------------------------------------------
// d_out[0 .. n_out) from d_data, both device pointers; d_taps: the device copy of wa_audio_taps' table (unused at 16 kHz); on `stream`.
// false: a launch failed or the shape is not served.  The arguments are the caller's to check (wa_audio_args_ok).
bool wa_audio_launch(void * stream, const void * d_data, long long n_frames, int channels, int format, const wa_audio_plan & p, const float * d_taps,
                     long long n_out, float * d_out);

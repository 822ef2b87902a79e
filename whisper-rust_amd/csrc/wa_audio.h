// wa_audio.h - audio front end: PCM (unsigned 8-bit, signed 16-, 24- and 32-bit, F32, F64) or G.711 (mu-law, A-law), one or two
// channels, 8 .. 192 kHz -> 16 kHz mono F32.
//
// Plain C++ (no HIP, no device types): tests/native/audio_math.cpp compiles this header alone with g++.  It holds the filter plan, the
// filter taps and wa_audio_ref, the host restatement of conversion plus resampling that the kernels of wa_audio.hip are held to bit for
// bit and that serves a call whose HIP path fails (wa_audio.cpp).  The conversion of the formats beyond I16 and F32 (WA_AUDIO_HD) is also
// compiled for the device when hipcc reads this file: wa_audio_fmt.hip runs the text the host runs.
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
// The other formats follow the same two rules.  A sample becomes a value v in F32 and the format has a scale S, a power of two:
//   U8    v = (float) ((int) u - 128)                                   S = 128
//   S24   v = (float) s, s the 3 little-endian bytes sign-extended (exact)     S = 8388608
//   S32   v = (float) s, rounded to nearest even                        S = 2147483648
//   F64   v = (float) x, rounded to nearest even; NaN and Inf pass through as F32's do      no scale
//   ULAW  v = (float) e, e = wa_audio_ulaw(b) the G.711 expansion to int16    S = 32768
//   ALAW  v = (float) e, e = wa_audio_alaw(b)                           S = 32768
// mono v / S (F64: v); stereo ((vl + vr) / 2.0f) / S (F64: (vl + vr) / 2.0f) - the I16 and F32 stereo rules.  Because S is a power of two and
// nothing underflows, U8 / S24 / S32 / F64 input gives the bits of F32 input holding the per-sample v / S (F64: v), and G.711 input gives
// the bits of I16 input holding e.
// Alignment.  HOST pointers may have any alignment in every format (a WAV data chunk lies where its header ends): the device path copies
// bytes and the host functions here read samples through memcpy.  DEVICE pointers: U8, ULAW, ALAW and S24 any byte address; I16, S32, F32
// and F64 the natural alignment of the sample.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define WA_AUDIO_HD __host__ __device__
#else
#define WA_AUDIO_HD
#endif

#define WA_AUDIO_RATE   16000      // output rate
#define WA_AUDIO_ZEROS  32         // Z
#define WA_AUDIO_BETA   11.0
#define WA_AUDIO_ROLL   0.115      // cut-off = (1 - ROLL) x the lower rate's Nyquist frequency
#define WA_AUDIO_MAX_L  640
#define WA_AUDIO_I16    0          // = WHISPER_AMD_PCM_I16
#define WA_AUDIO_F32    1          // = WHISPER_AMD_PCM_F32
#define WA_AUDIO_U8     3          // = WHISPER_AMD_PCM_U8 ... (2 stays refused)
#define WA_AUDIO_S24    4
#define WA_AUDIO_S32    5
#define WA_AUDIO_F64    6
#define WA_AUDIO_ULAW   7
#define WA_AUDIO_ALAW   8

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

// bytes of one sample; 0: not a format
inline int wa_audio_sample_bytes(int format) {
    switch (format) {
        case WA_AUDIO_U8: case WA_AUDIO_ULAW: case WA_AUDIO_ALAW: return 1;
        case WA_AUDIO_I16: return 2;
        case WA_AUDIO_S24: return 3;
        case WA_AUDIO_S32: case WA_AUDIO_F32: return 4;
        case WA_AUDIO_F64: return 8;
        default: return 0;
    }
}
// bytes of one frame: every staging size and copy of a recording is n_frames times this
inline size_t wa_audio_frame_bytes(int format, int channels) { return (size_t) wa_audio_sample_bytes(format) * (size_t) channels; }
// I16 and F32 are served by the kernels of wa_audio.hip / wa_channels.hip / wa_stream.hip, the others by those of wa_audio_fmt.hip
inline bool wa_audio_format_base(int format) { return format == WA_AUDIO_I16 || format == WA_AUDIO_F32; }
// The end of a live session pushes K/2 silent frames.  A-law has no code that expands to 0 and U8's and mu-law's zero bytes are not silence,
// so those frames travel as F32 zeros; I16 sessions keep their int16 zeros.  Either gives +0.0f.
inline int wa_audio_silence_format(int format) { return format == WA_AUDIO_I16 ? WA_AUDIO_I16 : WA_AUDIO_F32; }

inline bool wa_audio_args_ok(const void * data, int64_t n_frames, int channels, int rate, int format) {
    wa_audio_plan p;
    return n_frames >= 0 && (data || n_frames == 0) && (channels == 1 || channels == 2) && wa_audio_sample_bytes(format) > 0 &&
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

// G.711 expansions to int16, plain integer arithmetic (ITU-T G.711; the values of Python's audioop.ulaw2lin / alaw2lin for all 256 codes)
WA_AUDIO_HD inline int wa_audio_ulaw(unsigned b) {
    const unsigned u = ~b & 0xffu;
    int t = (int) (((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u);
    t -= 0x84;
    return (u & 0x80u) ? -t : t;
}
WA_AUDIO_HD inline int wa_audio_alaw(unsigned b) {
    const unsigned a = (b ^ 0x55u) & 0xffu, x = (a >> 4) & 7u;
    int t = (int) ((a & 15u) << 4) + 8;
    if (x) t = (t + 0x100) << (x - 1);
    return (a & 0x80u) ? t : -t;
}

// sample `idx` of U8 / S24 / S32 / F64 / ULAW / ALAW data as the value v of the table at the top.  Host code reads through memcpy (any
// alignment); device code reads S32 and F64 with one aligned load.
WA_AUDIO_HD inline float wa_audio_value(const void * data, int64_t idx, int format) {
    const unsigned char * b = (const unsigned char *) data;
    switch (format) {
        case WA_AUDIO_U8:   return (float) ((int) b[idx] - 128);
        case WA_AUDIO_S24: {
            const unsigned char * q = b + 3 * idx;
            return (float) ((int) q[0] | ((int) q[1] << 8) | ((int) (signed char) q[2] * 65536));
        }
        case WA_AUDIO_S32: {
#if defined(__HIP_DEVICE_COMPILE__)
            return (float) ((const int *) data)[idx];
#else
            int32_t s; memcpy(&s, b + 4 * idx, 4); return (float) s;
#endif
        }
        case WA_AUDIO_F64: {
#if defined(__HIP_DEVICE_COMPILE__)
            return (float) ((const double *) data)[idx];
#else
            double x; memcpy(&x, b + 8 * idx, 8); return (float) x;
#endif
        }
        case WA_AUDIO_ULAW: return (float) wa_audio_ulaw(b[idx]);
        default:            return (float) wa_audio_alaw(b[idx]);
    }
}
// the scale S; 1 for F64 (no division is made)
WA_AUDIO_HD inline float wa_audio_scale(int format) {
    return format == WA_AUDIO_U8 ? 128.0f : format == WA_AUDIO_S24 ? 8388608.0f : format == WA_AUDIO_S32 ? 2147483648.0f
         : format == WA_AUDIO_F64 ? 1.0f : 32768.0f;
}
// frame i of those formats as mono F32, and channel c of stereo frame i
WA_AUDIO_HD inline float wa_audio_frame_fmt(const void * data, int64_t i, int channels, int format) {
    float v;
    if (channels == 1) v = wa_audio_value(data, i, format);
    else {
        const float sum = wa_audio_value(data, 2 * i, format) + wa_audio_value(data, 2 * i + 1, format);
        v = sum / 2.0f;
    }
    return format == WA_AUDIO_F64 ? v : v / wa_audio_scale(format);
}
WA_AUDIO_HD inline float wa_audio_channel_fmt(const void * data, int64_t i, int c, int format) {
    const float v = wa_audio_value(data, 2 * i + c, format);
    return format == WA_AUDIO_F64 ? v : v / wa_audio_scale(format);
}

inline float wa_audio_load_i16(const void * data, int64_t idx) { int16_t s; memcpy(&s, (const unsigned char *) data + 2 * idx, 2); return (float) s; }
inline float wa_audio_load_f32(const void * data, int64_t idx) { float f; memcpy(&f, (const unsigned char *) data + 4 * idx, 4); return f; }

// frame i as mono F32
inline float wa_audio_frame(const void * data, int64_t i, int channels, int format) {
    if (format == WA_AUDIO_I16) {
        if (channels == 1) return wa_audio_load_i16(data, i) / 32768.0f;
        const float sum = wa_audio_load_i16(data, 2 * i) + wa_audio_load_i16(data, 2 * i + 1);
        const float mid = sum / 2.0f;
        return mid / 32768.0f;
    }
    if (format != WA_AUDIO_F32) return wa_audio_frame_fmt(data, i, channels, format);
    if (channels == 1) return wa_audio_load_f32(data, i);
    const float sum = wa_audio_load_f32(data, 2 * i) + wa_audio_load_f32(data, 2 * i + 1);
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
// the same for the formats that are not wa_audio_format_base (wa_audio_fmt.hip)
bool wa_audio_fmt_launch(void * stream, const void * d_data, long long n_frames, int channels, int format, const wa_audio_plan & p, const float * d_taps,
                         long long n_out, float * d_out);

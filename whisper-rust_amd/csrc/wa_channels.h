// wa_channels.h - two-channel recordings: both channels of an interleaved stereo recording as two planes of 16 kHz F32, the
// energy of spans of either plane, the reference cli's --diarize rule, and the gate and merge rules of whisper_amd_full_long_channels.
//
// Plain C++ (no HIP, no device types): tests/native/channels_math.cpp compiles this header alone with g++.  Every function here is the host
// restatement the kernels of wa_channels.hip are held to bit for bit, and serves a call whose HIP path fails (wa_channels.cpp).
//
// Split.  Plane c of a recording is wa_audio.h's result for channel c taken as a MONO recording of the same rate and format: sample
// conversion (float) s[2 i + c] / 32768.0f or f[2 i + c] (the other formats: v / S of sample 2 i + c, wa_audio.h's table), then - at rates other than 16 kHz - the same F32 fmaf chain over the same taps
// (wa_audio_taps), k ascending from 0.0f, x zero outside the input.  Plane c lies at out + c * stride, stride = wa_ch_stride(n_out).
//
// Energy.  E_c[a, b) = sum over j in [a, b) of |x_c[j]| in F64, a and b clamped to [0, n], 0.0 where a >= b, in ONE order that depends on
// a and b alone:
//   - lane l, l = 0 .. WA_CH_LANES - 1, sums the samples j of [a, b) with j mod WA_CH_LANES == l, j ascending, from 0.0
//     ((double) fabsf(x[j]), each addition rounded to F64);
//   - the lanes are folded by the tree  for (s = WA_CH_LANES / 2; s >= 1; s /= 2) for (l < s) v[l] += v[l + s];  E = v[0].
// The lane of a sample is fixed by its index in the plane, not by where the span starts, and nothing depends on how a launch is cut.  A
// sequential sum of the same n samples differs from this one by at most n 2^-53 relative to first order (both are sums of non-negative
// terms; each has at most n - 1 roundings on any path).
//
// Speakers (the reference cli's --diarize rule, examples/cli/cli.cpp): centiseconds to samples by clamp((int) (t * 16000 / 100), 0, n - 1)
// evaluated as the cli does (int64 product, int division), energies over [is0, is1), then in F64 e0 > ratio * e1 -> 0, else
// e1 > ratio * e0 -> 1, else -1; ratio <= 0 means 1.1.
//
// Gate: a VAD segment of channel c over its own span [cs_to_samples(start), min(cs_to_samples(end), n)) is dropped when
// E_c < g * E_other (the other speaker bleeding through); g <= 0 drops nothing.
//
// Merge: per channel, in the channel's own order, t1 = max(t1, t0 + 10), then t0 = max(t0, t1 of the previous segment OF THE SAME
// CHANNEL); the two lists are then merged by (t0, channel), each channel keeping its own order (wa_ch_merge).
#pragma once

#include "wa_audio.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#define WA_CH_TILE   512        // outputs (per channel) per workgroup of k_audio_split (exported: whisper_amd_channels_tile)
#define WA_CH_LDS    15360      // floats of LDS k_audio_split owns: two planes of the input span, and the taps where they fit beside them
#define WA_CH_LANES  256        // lanes of the energy order (exported: whisper_amd_channels_energy_lanes)
#define WA_CH_ALIGN  64         // floats: plane 1 starts on a 256-byte boundary

inline int64_t wa_ch_stride(int64_t n_out) { return (n_out + WA_CH_ALIGN - 1) / WA_CH_ALIGN * WA_CH_ALIGN; }

inline bool wa_ch_args_ok(const void * data, int64_t n_frames, int rate, int format) {
    return wa_audio_args_ok(data, n_frames, 2, rate, format) && n_frames <= INT64_MAX / 4 / WA_AUDIO_MAX_L;
}

// input frames a tile of WA_CH_TILE outputs reads (one plane of the kernel's LDS span), as wa_audio_span
inline int wa_ch_span(const wa_audio_plan & p) { return (int) (((int64_t) (WA_CH_TILE - 1) * p.M + p.L - 1) / p.L) + p.K; }

// channel c of frame i as F32
inline float wa_ch_frame(const void * data, int64_t i, int c, int format) {
    if (format == WA_AUDIO_I16) return wa_audio_load_i16(data, 2 * i + c) / 32768.0f;
    if (format != WA_AUDIO_F32) return wa_audio_channel_fmt(data, i, c, format);
    return wa_audio_load_f32(data, 2 * i + c);
}

// Both planes on the host: out[c * stride + n], n < wa_audio_n_out(n_frames, rate); returns that count, -1 on refused arguments.
// `taps`: the table of wa_audio_taps for this rate, or null to build it here.  The floats between a plane's end and the stride are not written.
inline int64_t wa_ch_split_ref(const void * data, int64_t n_frames, int rate, int format, const float * taps, float * out, int64_t stride) {
    if (!wa_ch_args_ok(data, n_frames, rate, format)) return -1;
    wa_audio_plan p;
    wa_audio_plan_make(rate, p);
    const int64_t n_out = wa_audio_n_out(n_frames, rate);
    if (stride < n_out) return -1;
    if (!p.K) {
        for (int c = 0; c < 2; ++c)
            for (int64_t i = 0; i < n_frames; ++i) out[c * stride + i] = wa_ch_frame(data, i, c, format);
        return n_out;
    }
    std::vector<float> own;
    if (!taps) { wa_audio_taps(p, own); taps = own.data(); }
    std::vector<float> x((size_t) n_frames + 2 * (size_t) p.K);
    for (int c = 0; c < 2; ++c) {
        std::fill(x.begin(), x.end(), 0.0f);
        for (int64_t i = 0; i < n_frames; ++i) x[(size_t) (i + p.K)] = wa_ch_frame(data, i, c, format);
        for (int64_t n = 0; n < n_out; ++n) {
            const int64_t t = n * p.M, i0 = t / p.L;
            const float * h = taps + (size_t) (t % p.L) * p.K, * xs = x.data() + (size_t) (i0 - p.K / 2 + 1 + p.K);
            float acc = 0.0f;
            for (int k = 0; k < p.K; ++k) acc = std::fmaf(h[k], xs[k], acc);
            out[c * stride + n] = acc;
        }
    }
    return n_out;
}

// E[a, b) of one plane of n samples, in the order stated at the top
inline double wa_ch_energy_ref(const float * x, int64_t n, int64_t a, int64_t b) {
    a = std::max<int64_t>(a, 0);
    b = std::min<int64_t>(b, n);
    if (a >= b) return 0.0;
    double v[WA_CH_LANES];
    for (int l = 0; l < WA_CH_LANES; ++l) {
        double s = 0.0;
        int64_t j = a + ((l - a % WA_CH_LANES) + WA_CH_LANES) % WA_CH_LANES;     // the first index >= a of lane l
        for (; j < b; j += WA_CH_LANES) s += (double) std::fabs(x[j]);
        v[l] = s;
    }
    for (int s = WA_CH_LANES / 2; s >= 1; s /= 2)
        for (int l = 0; l < s; ++l) v[l] += v[l + s];
    return v[0];
}

// the reference cli's timestamp_to_sample (examples/common-whisper.cpp): clamp((int) (t * 16000 / 100), 0, n_samples - 1).  The quotient is
// kept in int64 and clamped there: it equals the cli's value wherever the cli's int cast is defined (quotients up to INT_MAX, t up to
// 13.4 million cs = 37 h); beyond that, where the cast is implementation-defined, it is n_samples - 1, the value the clamp is there to give.
inline int64_t wa_ch_cs_to_sample(int64_t t_cs, int64_t n_samples) {
    const int64_t hi = std::max<int64_t>(n_samples - 1, 0);
    if (t_cs <= 0) return 0;
    if (t_cs > hi) return hi;                                // t * 160 >= t: past the end already; below, t <= hi < 2^63 / 16000
    return std::min<int64_t>(t_cs * WA_AUDIO_RATE / 100, hi);
}

// 0, 1, or -1 = undecided
inline int wa_ch_label(double e0, double e1, double ratio) {
    if (!(ratio > 0.0)) ratio = 1.1;
    if (e0 > ratio * e1) return 0;
    if (e1 > ratio * e0) return 1;
    return -1;
}

// true: the segment of a channel with energy e_own over its span, e_other on the other channel over the same span, is dropped
inline bool wa_ch_gate_drops(double e_own, double e_other, double g) { return g > 0.0 && e_own < g * e_other; }

struct wa_ch_item {
    int64_t t0, t1;             // centiseconds, already mapped into the caller's audio
    int channel, index;         // index within the channel's own list
};

// The clamps inside each channel's list (in its order), then the two lists merged: the next segment is the head of channel 0 unless the
// head of channel 1 has a smaller t0.  items[c] is channel c's list; item.channel / .index are set here.  A channel's segments keep their
// order in the merged list ALWAYS - it is whisper_amd_full_long's order for that channel.  Where every channel's clamped t0 does not
// decrease this is the order (t0, channel, index within the channel).  It can decrease only where a clamp pushed a t0 past its own t1
// (t1 is not extended again, as whisper_amd_full_long does not): the next segment of that channel is clamped against that smaller t1.
inline std::vector<wa_ch_item> wa_ch_merge(std::vector<wa_ch_item> items[2]) {
    for (int c = 0; c < 2; ++c) {
        int64_t prev = INT64_MIN;
        for (size_t i = 0; i < items[c].size(); ++i) {
            wa_ch_item & it = items[c][i];
            if (it.t1 - it.t0 < 10) it.t1 = it.t0 + 10;
            if (i > 0) it.t0 = std::max(it.t0, prev);
            prev = it.t1;
            it.channel = c; it.index = (int) i;
        }
    }
    std::vector<wa_ch_item> all;
    size_t at[2] = { 0, 0 };
    while (at[0] < items[0].size() || at[1] < items[1].size()) {
        const int c = at[0] >= items[0].size() ? 1 : at[1] >= items[1].size() ? 0 : items[1][at[1]].t0 < items[0][at[0]].t0 ? 1 : 0;
        all.push_back(items[c][at[c]++]);
    }
    return all;
}

// -------------------------------------------------------------------------------------------------
// device side (wa_channels.hip).  No HIP types here: the stream travels as void *.
// -------------------------------------------------------------------------------------------------
// d_out[c * stride + n], n < n_out, c = 0, 1, from the interleaved stereo d_data, in ONE launch on `stream`; d_taps: the device copy of
// wa_audio_taps' table (unused at 16 kHz).  false: the launch failed or the shape is not served (nothing was launched).
bool wa_ch_split_launch(void * stream, const void * d_data, long long n_frames, int format, const wa_audio_plan & p, const float * d_taps, long long n_out,
                        long long stride, float * d_out);
// the same for the formats that are not wa_audio_format_base (wa_audio_fmt.hip)
bool wa_ch_split_fmt_launch(void * stream, const void * d_data, long long n_frames, int format, const wa_audio_plan & p, const float * d_taps, long long n_out,
                            long long stride, float * d_out);
// d_energy[2 * i + c] = E_c[d_spans[2 * i], d_spans[2 * i + 1]) for i < n_spans over the planes d_planes + c * stride of n samples each, in ONE launch
bool wa_ch_energy_launch(void * stream, const float * d_planes, long long n, long long stride, const long long * d_spans, int n_spans, double * d_energy);

// wa_stream.h - live streaming sessions: the sliding windows of the reference's examples/stream/stream.cpp (its step mode)
// on a 16 kHz ring that lives on the device, fed in packets of any size, rate and format the audio front end takes (wa_audio.h).
//
// Plain C++ (no HIP, no device types): tests/native/stream_plan.cpp compiles this header alone with g++.  It holds the session plan, the ring
// arithmetic, the push planner and wa_stream_ref, the host restatement of packet push, ring and window gather that the kernels of
// wa_stream.hip are held to bit for bit and that serves a session whose HIP path fails (wa_stream.cpp).
//
// Sizes (stream.cpp's clamps): keep_ms = min(keep_ms, step_ms), length_ms = max(length_ms, step_ms); n_step, n_len, n_keep = (int) ((1e-3 ms) * 16000)
// in double; n_new_line = max(1, length_ms / step_ms - 1).
// Window k consumes n_step new samples (the last window after a flush: what is left): take = min(old, max(0, n_keep + n_len - new)), the window
// is the last `take` samples of the previous window followed by the new ones, old = the window's length.  iter += 1; when iter % n_new_line
// == 0 the line is committed: old = the window's last n_keep samples (and the prompt becomes the window's tokens, wa_stream.cpp).
// Without drops window k is the range [e - len, e) of the session's 16 kHz axis, e = (k + 1) n_step, len <= n_keep + n_len.
//
// The ring: capacity n_keep + n_len + backlog samples, addressed by the RING AXIS r: sample r lies in slot r mod capacity.  The ring axis is the
// session's absolute 16 kHz axis with the dropped samples taken out: a drop (drop_late, stream.cpp's "cannot process audio fast enough" rule:
// more than 2 n_step new samples pending at a step) moves the write head back over the pending samples, so a window is ALWAYS one range of
// the ring axis - at most two ring pieces - while on the absolute axis the window after a drop is two ranges.  (The gather kernel takes up to
// four pieces per session: two ranges that both wrap; the session itself never needs more than two.)
//
// The push planner: a packet of F frames at rate R behind T frames already fed.  Output n reads frames floor(n M / L) - K/2 + 1 ..
// floor(n M / L) + K/2, so it is final once floor(n M / L) + K/2 <= T + F - 1: wa_stream_final(T + F) = ceil((T + F - K/2) L / M) outputs are
// final (0 while T + F <= K/2; T + F itself at 16 kHz).  The first output that is not final reads no frame before T + F - K + 1: the carry is
// the last K - 1 frames as mono F32.  At the end of input ceil(T L / M) outputs exist, the frames behind the end zero: a flush is a push of
// K/2 zero frames.
#pragma once

#include "wa_audio.h"

#include <algorithm>
#include <cstring>
#include <utility>

#define WA_STREAM_TILE      1024       // outputs per workgroup of k_stream_push and k_stream_window (exported: whisper_amd_stream_tile)
#define WA_STREAM_PIECES    4          // ring pieces per session of one k_stream_window launch
#define WA_STREAM_SESSIONS  8          // sessions per k_stream_window launch: the lock-step group's width
#define WA_STREAM_MAX_WINDOW_MS 30000  // keep_ms + length_ms: what one whisper_full window holds

// deliberately wrong variants (tests/native/stream_plan.cpp shows that each changes an expected value); 0 everywhere else
#define WA_STREAM_WRONG_EARLY   1      // an output released one frame early
#define WA_STREAM_WRONG_CARRY   2      // a carry one frame short
#define WA_STREAM_WRONG_COMMIT  3      // the commit taken on iter % n_new_line == 1
#define WA_STREAM_WRONG_TAKE    4      // take computed from n_len alone

struct wa_stream_sizes { int step_ms = 0, length_ms = 0, keep_ms = 0, n_step = 0, n_len = 0, n_keep = 0, n_new_line = 1; };

// false: step_ms <= 0, a negative length or keep, or a window of more than 30 s
inline bool wa_stream_sizes_make(int step_ms, int length_ms, int keep_ms, wa_stream_sizes & z) {
    if (step_ms <= 0 || length_ms < 0 || keep_ms < 0) return false;
    keep_ms = std::min(keep_ms, step_ms);
    length_ms = std::max(length_ms, step_ms);
    if ((int64_t) keep_ms + length_ms > WA_STREAM_MAX_WINDOW_MS) return false;
    z.step_ms = step_ms; z.length_ms = length_ms; z.keep_ms = keep_ms;
    z.n_step = (int) ((1e-3 * step_ms) * WA_AUDIO_RATE);
    z.n_len  = (int) ((1e-3 * length_ms) * WA_AUDIO_RATE);
    z.n_keep = (int) ((1e-3 * keep_ms) * WA_AUDIO_RATE);
    z.n_new_line = std::max(1, length_ms / step_ms - 1);
    return z.n_step > 0;
}

struct wa_stream_range { int64_t start = 0, len = 0; };        // on the absolute 16 kHz axis

struct wa_stream_step {
    int take = 0, n_new = 0, len = 0;
    bool commit = false;
    int64_t r0 = 0;                        // the window's first sample on the ring axis
    int64_t dropped = 0;                   // samples this step discarded instead of running a window
    std::vector<wa_stream_range> ranges;   // the window on the absolute axis: one range, more where samples were dropped inside its span
};

struct wa_stream_plan {
    wa_stream_sizes z;
    bool drop_late = false;
    int64_t r_old = 0;         // ring axis: where the previous window ended = where the unconsumed samples begin
    int64_t r_w = 0;           // ring axis: the write head
    int64_t old_len = 0;       // samples in front of r_old that the next window may take
    int64_t iter = 0, dropped = 0;
    std::vector<std::pair<int64_t, int64_t>> drops;     // (ring position, samples taken out in front of it), ascending

    void reset() { r_old = r_w = old_len = iter = dropped = 0; drops.clear(); }
    int64_t pending() const { return r_w - r_old; }
    // windows due: whole steps, and after the end of input one more for what is left
    int64_t due(bool flushed) const { return pending() / z.n_step + (flushed && pending() % z.n_step > 0 ? 1 : 0); }
    int64_t to_abs(int64_t r) const {
        int64_t a = r;
        for (const auto & d : drops) if (d.first <= r) a += d.second;
        return a;
    }
    void drop_pending() {
        const int64_t n = pending();
        if (n <= 0) return;
        if (!drops.empty() && drops.back().first == r_old) drops.back().second += n; else drops.push_back({ r_old, n });
        dropped += n;
        r_w = r_old;
    }
};

// The next window, if one is due.  false: none (s.dropped > 0: the drop rule discarded the pending samples instead).
inline bool wa_stream_next(wa_stream_plan & P, bool flushed, wa_stream_step & s, int wrong = 0) {
    s = wa_stream_step();
    const wa_stream_sizes & z = P.z;
    const int64_t pending = P.pending();
    if (P.drop_late && pending > 2 * (int64_t) z.n_step) { s.dropped = pending; P.drop_pending(); return false; }
    const int64_t n_new = pending >= z.n_step ? z.n_step : flushed ? pending : 0;
    if (n_new <= 0) return false;
    const int64_t room = (wrong == WA_STREAM_WRONG_TAKE ? 0 : z.n_keep) + (int64_t) z.n_len - n_new;
    const int64_t take = std::min(P.old_len, std::max<int64_t>(0, room));
    s.take = (int) take; s.n_new = (int) n_new; s.len = (int) (take + n_new);
    s.r0 = P.r_old - take;
    int64_t a = s.r0;                               // the absolute ranges: cut where samples were taken out
    for (const auto & d : P.drops) if (d.first > s.r0 && d.first < s.r0 + s.len) {
        s.ranges.push_back({ P.to_abs(a), d.first - a });
        a = d.first;
    }
    s.ranges.push_back({ P.to_abs(a), s.r0 + s.len - a });
    P.r_old += n_new;
    P.old_len = s.len;
    P.iter += 1;
    s.commit = P.iter % z.n_new_line == (wrong == WA_STREAM_WRONG_COMMIT ? 1 : 0);
    if (s.commit) P.old_len = std::min<int64_t>(z.n_keep, s.len);
    return true;
}

// ring-axis range [r0, r0 + len), len <= cap, as at most two pieces of the ring; returns their number
inline int wa_stream_ring_pieces(int64_t r0, int64_t len, int64_t cap, int32_t slot[2], int32_t plen[2]) {
    if (len <= 0) return 0;
    const int64_t s0 = r0 % cap, first = std::min(len, cap - s0);
    slot[0] = (int32_t) s0; plen[0] = (int32_t) first;
    if (first == len) return 1;
    slot[1] = 0; plen[1] = (int32_t) (len - first);
    return 2;
}

// outputs that are final once T frames have arrived
inline int64_t wa_stream_final(const wa_audio_plan & p, int64_t T, int wrong = 0) {
    if (!p.K) return T;
    const int64_t half = p.K / 2 - (wrong == WA_STREAM_WRONG_EARLY ? 1 : 0);
    return T <= half ? 0 : ((T - half) * p.L + p.M - 1) / p.M;
}
inline int wa_stream_carry_len(const wa_audio_plan & p) { return p.K ? p.K - 1 : 0; }
inline int wa_stream_flush_frames(const wa_audio_plan & p) { return p.K / 2; }

// The host restatement: conversion by wa_audio_frame, the fmaf chain of wa_audio_ref over the same table, the ring, the gather.
struct wa_stream_ref {
    wa_audio_plan ap;
    int channels = 1, format = WA_AUDIO_F32;
    std::vector<float> taps, carry, ring;
    int64_t T = 0, n_out = 0;          // frames fed, outputs made final

    bool init(int rate, int ch, int fmt, int64_t ring_cap) {
        if (!wa_audio_args_ok(nullptr, 0, ch, rate, fmt) || ring_cap < 0) return false;
        wa_audio_plan_make(rate, ap);
        channels = ch; format = fmt;
        wa_audio_taps(ap, taps);
        ring.assign((size_t) ring_cap, 0.0f);
        reset();
        return true;
    }
    void reset() { carry.assign((size_t) wa_stream_carry_len(ap), 0.0f); T = 0; n_out = 0; }
    int64_t n_new(int64_t n_frames, int wrong = 0) const { return wa_stream_final(ap, T + n_frames, wrong) - n_out; }

    // one packet: writes the n_new(n_frames) outputs it makes final to `out`, returns their number
    int64_t push(const void * data, int64_t n_frames, float * out, int wrong = 0) {
        const int64_t made = n_new(n_frames, wrong);
        if (!ap.K) {
            for (int64_t i = 0; i < n_frames; ++i) out[i] = wa_audio_frame(data, i, channels, format);
        } else {
            const int64_t C = (int64_t) carry.size();
            std::vector<float> x((size_t) (C + n_frames));          // frames T - C .. T + n_frames - 1
            std::copy(carry.begin(), carry.end(), x.begin());
            if (wrong == WA_STREAM_WRONG_CARRY && C > 0) x[0] = 0.0f;
            for (int64_t i = 0; i < n_frames; ++i) x[(size_t) (C + i)] = wa_audio_frame(data, i, channels, format);
            for (int64_t j = 0; j < made; ++j) {
                const int64_t t = (n_out + j) * ap.M, i0 = t / ap.L;
                const float * h = taps.data() + (size_t) (t % ap.L) * ap.K;
                const int64_t first = i0 - ap.K / 2 + 1 - (T - C);  // index into x of the chain's first frame
                float acc = 0.0f;
                for (int k = 0; k < ap.K; ++k) {
                    const int64_t at = first + k;
                    acc = std::fmaf(h[k], at >= 0 && at < C + n_frames ? x[(size_t) at] : 0.0f, acc);
                }
                out[j] = acc;
            }
            std::copy(x.end() - C, x.end(), carry.begin());
        }
        T += n_frames; n_out += made;
        return made;
    }
    // the end of input: the outputs whose chains reach behind it; at most ceil(K/2 L / M) + 1 of them
    int64_t flush(float * out) {
        const int64_t Z = wa_stream_flush_frames(ap);
        if (Z == 0) return 0;
        const int fmt = format;
        format = wa_audio_silence_format(fmt);     // zero bytes are silence in I16 and F32 only: the other formats' zero frames travel as F32
        const std::vector<uint8_t> zeros((size_t) Z * wa_audio_frame_bytes(format, channels), 0);
        const int64_t T0 = T, made = push(zeros.data(), Z, out);
        format = fmt;
        T = T0;                                    // the zero frames are no input: T keeps counting the caller's
        return made;
    }
    void ring_write(int64_t r, const float * src, int64_t n) {
        const int64_t cap = (int64_t) ring.size();
        for (int64_t j = 0; j < n; ++j) ring[(size_t) ((r + j) % cap)] = src[j];
    }
    void gather(int n_pieces, const int32_t * slot, const int32_t * plen, float * dst) const {
        for (int p = 0; p < n_pieces; ++p) { memcpy(dst, ring.data() + slot[p], (size_t) plen[p] * sizeof(float)); dst += plen[p]; }
    }
};

// -------------------------------------------------------------------------------------------------
// device side (wa_stream.hip).  No HIP types here: the stream travels as void *.
// -------------------------------------------------------------------------------------------------
// One packet: d_data holds n_frames frames behind T frames already fed; d_carry_in the last K - 1 frames before them (mono F32), d_carry_out
// receives the last K - 1 after them (two buffers: no workgroup reads what another writes); the n_new outputs n_first .. become final and go to
// ring slots (r_w + j) mod cap.  The caller has checked the counts against wa_stream_final.  false: a launch failed or the shape is not served.
bool wa_stream_push_launch(void * stream, const void * d_data, long long n_frames, int channels, int format, const wa_audio_plan & p, const float * d_taps,
                           long long T, const float * d_carry_in, float * d_carry_out, long long n_first, long long n_new, float * d_ring, long long cap,
                           long long r_w);
// the same for the formats that are not wa_audio_format_base (wa_audio_fmt.hip)
bool wa_stream_push_fmt_launch(void * stream, const void * d_data, long long n_frames, int channels, int format, const wa_audio_plan & p, const float * d_taps,
                               long long T, const float * d_carry_in, float * d_carry_out, long long n_first, long long n_new, float * d_ring, long long cap,
                               long long r_w);

// the windows of up to WA_STREAM_SESSIONS sessions in one launch: per session the ring, its pieces in window order and the destination
struct wa_stream_window {
    const float * ring;
    float * dst;
    int32_t len, n_pieces;                         // len = the sum of plen
    int32_t slot[WA_STREAM_PIECES], plen[WA_STREAM_PIECES];
};
struct wa_stream_windows { wa_stream_window w[WA_STREAM_SESSIONS]; };
// The caller has checked every slot + plen against its ring.  false: the launch failed or the table is refused (nothing was launched).
bool wa_stream_window_launch(void * stream, const wa_stream_windows & tab, int n_sessions);

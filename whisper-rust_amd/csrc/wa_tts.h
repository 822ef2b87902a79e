// wa_tts.h - heuristic token timestamps (params.token_timestamps): the windowed |PCM| energy, the per-token record of the
// boundary scans over it, and the integer finalisation that turns a record into the token's two ends.
//
// Plain C++ (no HIP, no device types): tests/native/tts_math.cpp compiles this header alone with g++.  The host functions here are what
// the kernels of wa_tts.hip are held to bit for bit, and serve a call whose HIP path fails or is switched off (wa_tts.cpp).
//
// Energy.  e[i] = (((0.0f + |x[lo]|) + |x[lo + 1]|) + ... + |x[hi]|) / 65.0f with lo = max(i - 32, 0), hi = min(i + 32, n - 1): F32
// additions in ascending index order, no fma, the divisor the full window length also where the window is clipped (whisper.cpp:8326-8360).
//
// Record of a text token with sample ends s_lo, s_hi in [0, n) (wa_tts_record):
//   window  w_lo = max(s_lo - WA_TTS_REACH, 0), w_hi = min(s_hi + WA_TTS_REACH, n);
//   total   = sum of e[k], k in [w_lo, w_hi), ONE F32 chain in ascending order from 0.0f (0 for an empty or inverted window);
//   level   = (float) (0.5 * (double) total / (double) (w_hi - w_lo))  - NaN for an empty window (recorded as 0x7fc00000), -0.0 for an inverted one;
//   loud(k) = e[k] > level, quiet(k) = e[k] < level;
//   back_lo   k = s_lo; while (k > 0 && loud(k)) --k          (s_lo itself without a previous token: the scan is not used then)
//   fwd_lo    k = s_lo; while (quiet(k) && k < s_hi) ++k
//   fwd_hi    k = s_hi; while (k < n - 1 && loud(k)) ++k
//   back_hi   k = s_hi; while (quiet(k) && k > 0) --k         (the bound by the token's final start is the finalisation's)
//   flags     WA_TTS_LOUD_LO = loud(s_lo), WA_TTS_LOUD_HI = loud(s_hi), WA_TTS_HAS_PREV echoes the input.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#define WA_TTS_HALF   32          // the energy window is 2 * 32 + 1 samples
#define WA_TTS_TILE   1024        // outputs per workgroup of k_tts_energy (exported: whisper_amd_tts_tile)
#define WA_TTS_REACH  2000        // samples either side of a token that enter its level (WHISPER_SAMPLE_RATE / 8)
#define WA_TTS_RATE   16000
#define WA_TTS_MAX_N  (1 << 30)   // samples the entries accept: every index and every index + 64 stays an int

#define WA_TTS_LOUD_LO  1u
#define WA_TTS_LOUD_HI  2u
#define WA_TTS_HAS_PREV 4u

struct wa_tts_record { int32_t back_lo, fwd_lo, fwd_hi, back_hi; uint32_t flags; float level; };      // = struct whisper_amd_tts_record

// mean |x| over the window [i - half, i + half] clipped to the signal, always divided by the full window length
inline std::vector<float> wa_signal_energy(const float * signal, int n, int half) {
    std::vector<float> e((size_t) std::max(n, 0));
    const float full = (float) (2 * half + 1);
    for (int i = 0; i < n; ++i) {
        const int lo = std::max(i - half, 0), hi = std::min(i + half, n - 1);
        float acc = 0;
        for (int k = lo; k <= hi; ++k) acc += fabsf(signal[k]);
        e[i] = acc / full;
    }
    return e;
}

// the record on the host; 0 <= s_lo, s_hi < n
inline wa_tts_record wa_tts_record_host(const float * e, int n, int s_lo, int s_hi, bool has_prev) {
    const int w_lo = std::max(s_lo - WA_TTS_REACH, 0), w_hi = std::min(s_hi + WA_TTS_REACH, n);
    float total = 0.0f;
    for (int k = w_lo; k < w_hi; ++k) total += e[k];
    const float level = (float) (0.5 * (double) total / (double) (w_hi - w_lo));
    const auto loud = [&](int k) { return e[k] > level; };
    const auto quiet = [&](int k) { return e[k] < level; };
    wa_tts_record r;
    r.level = level == level ? level : std::numeric_limits<float>::quiet_NaN();      // (a NaN's sign and payload are the machine's: the record holds the canonical one)
    r.flags = (loud(s_lo) ? WA_TTS_LOUD_LO : 0u) | (loud(s_hi) ? WA_TTS_LOUD_HI : 0u) | (has_prev ? WA_TTS_HAS_PREV : 0u);
    int k = s_lo;
    if (has_prev) while (k > 0 && loud(k)) --k;
    r.back_lo = k;
    for (k = s_lo; quiet(k) && k < s_hi;) ++k;
    r.fwd_lo = k;
    for (k = s_hi; k < n - 1 && loud(k);) ++k;
    r.fwd_hi = k;
    for (k = s_hi; quiet(k) && k > 0;) --k;
    r.back_hi = k;
    return r;
}

// One text token's ends from its record: both slide to the nearest crossing of the level.  lo / hi: the token's ends (10 ms units) as the
// repair pass left them, replaced here; seg_lo: the segment's start; prev_hi: the previous token's FINAL end, next_lo: the next token's start
// BEFORE its own snap (read only where has_prev / has_next).  Tokens are finalised in order.
inline void wa_tts_finalise(const wa_tts_record & r, int s_lo, int s_hi, int64_t seg_lo, bool has_prev, int64_t prev_hi, bool has_next, int64_t next_lo,
                            int64_t & lo, int64_t & hi) {
    const auto to_time = [&](int smp) { return (100ll * smp) / WA_TTS_RATE + seg_lo; };
    if ((r.flags & WA_TTS_LOUD_LO) && has_prev) {        // speech already under way: the start moves back, but not into the previous token
        lo = to_time(r.back_lo);
        if (lo < prev_hi) lo = prev_hi; else s_lo = r.back_lo;
    } else {                                             // leading silence: the start moves forward
        s_lo = r.fwd_lo;
        lo = to_time(s_lo);
    }
    if (r.flags & WA_TTS_LOUD_HI) {                      // still speaking at the end: it moves forward, but not into the next token
        hi = to_time(r.fwd_hi);
        if (has_next && hi > next_lo) hi = next_lo;
    } else {                                             // trailing silence: the end moves back, not past the start just found
        hi = to_time(s_hi <= s_lo ? s_hi : std::max((int) r.back_hi, s_lo));
    }
}

// -------------------------------------------------------------------------------------------------
// device side (wa_tts.hip).  No HIP types here: the stream travels as void *.  false: the launch failed or was refused (nothing launched).
// -------------------------------------------------------------------------------------------------
// d_energy[i], i < n, from d_pcm[0, n), in ONE launch on `stream`; 0 < n <= WA_TTS_MAX_N
bool wa_tts_energy_launch(void * stream, const float * d_pcm, int n, float * d_energy);
// d_rec[j], j < n_tokens, from d_energy[0, n) and d_tok = s_lo[n_tokens] | s_hi[n_tokens] | has_prev[n_tokens] (every end in [0, n)), in ONE launch
bool wa_tts_snap_launch(void * stream, const float * d_energy, int n, const int32_t * d_tok, int n_tokens, wa_tts_record * d_rec);

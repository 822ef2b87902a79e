// wa_stream_vad.h - live sessions that cut at pauses: the speech-segment rules of whisper_vad_segments_from_probs
// (whisper.cpp:5202-5436; wa_vad_segments_from_probs in wa_vad_host.cpp is their offline statement and the yardstick) in incremental form.
//
// Plain C++ (no HIP, no device types): tests/native/stream_vad_plan.cpp compiles this header alone with g++.
//
// wa_svad_segmenter::push takes ONE probability - that of the next 512-sample window - and appends to `out` every segment that later audio can
// no longer change; flush(T) ends the input (T = samples on the session's 16 kHz axis) and hands out the rest.  Fed window by window and
// flushed, it gives the list of wa_vad_segments_from_probs on the whole sequence, for every input whose list holds no segment longer than the
// cap (below), in the same integer arithmetic:
//   - the first pass over the probabilities (threshold, negative threshold, min_silence, the 98 ms rule under max_speech, min_speech) is causal:
//     its loop body runs here once per push with its variables kept, and what it pushes is a RAW speech;
//   - the merge pass joins neighbours less than 3200 samples apart, left to right: the segmenter holds ONE merged speech, `cur`, and a raw
//     speech either extends it or closes it;
//   - the min_speech erase runs when `cur` is closed, after the merge as in the reference;
//   - padding: after the merge every gap is >= 3200 samples, so with speech_pad_samples <= 1600 (speech_pad_ms <= 100; more is refused by
//     wa_svad_params_ok) the branch `silence < 2 * speech_pad_samples` is never taken and a segment's padding looks at nothing but the segment:
//     start = start > pad ? start - pad : 0, end = min(end + pad, audio_length_samples);
//   - the clamp to audio_length_samples (n_probs * 512) binds only at the flush: a segment closed earlier has end + pad <= end + 1600 while at
//     least end + 3200 samples have been seen.
// When `cur` = [s, e) is closed.  After window i (its samples are [512 i, 512 i + 512)) has been pushed, `cur` is closed as soon as
//     512 (i + 1) - e >= 3200  and  no candidate speech is open (a candidate opened inside the gap has been pushed and merged - then e moved - or
//     discarded), or a raw speech that starts at or beyond e + 3200 has been pushed,
// whichever comes first: no later window can start a speech closer than 3200 samples to e.  The emission-delay bound that follows, in samples
// fed beyond the end e of the segment's last raw speech, when no candidate opens inside (e, e + 3200) and the probabilities behind e stay below
// the negative threshold: wa_svad_delay_bound = max(ceil512(min_silence_samples) + 512, 3584): the raw speech is pushed by the first window that
// starts min_silence_samples behind e, and the window [e + 3072, e + 3584) is the first whose end lies 3200 behind e (e is a multiple of 512).
// A candidate inside the gap delays the segment until the first pass has decided it, at most max_speech_samples + 512 samples after it opened.
//
// The length cap (the one departure from the offline list).  An utterance must fit the state's PCM buffer: cap_samples = max_utterance_ms * 16.
// max_speech_duration_s <= the cap keeps every raw speech within it (a raw speech spans at most max_speech_samples + 512 = 16000 (int)
// max_speech_duration_s - 2 pad samples), but the merge pass can re-join what max_speech split.  A merge whose padded result
// [start - start_pad, raw.end + pad), as an utterance range (wa_svad_range), would be longer than cap_samples is NOT made: `cur` is closed as it
// stands, the raw speech opens the next one, and `splits` counts the case.  The two then lie less than 3200 samples apart, so at that boundary -
// and only there - the reference's padding rule for close neighbours is applied, at once: silence = raw.start - cur.end; when silence <
// 2 pad, cur.end grows by silence / 2 and the next speech's start pad is silence / 2, else both get the whole pad.  (tools/stream_vad_ref.py
// restates list, range and split rule; equality with the offline list is claimed for inputs where `splits` stays 0.)
//
// The utterance of a segment: the samples [cs_to_samples(start_cs), min(cs_to_samples(end_cs), T)) of the session's axis - one contiguous range,
// none of wa_vad_filter_audio's overlap or inserted silence.  Before the flush T is not known and does not bind (see the clamp above).
#pragma once

#include "wa_long_plan.h"

#include <climits>

#define WA_SVAD_MAX_UTTERANCE_MS 30000     // the state's PCM buffer
#define WA_SVAD_MERGE_GAP        3200      // sample_rate * 200 / 1000
#define WA_SVAD_MAX_PAD_MS       100       // 2 * speech_pad_samples <= WA_SVAD_MERGE_GAP

// deliberately wrong variants (tests/native/stream_vad_plan.cpp shows that each changes an expected list); 0 everywhere else
#define WA_SVAD_WRONG_LOOKAHEAD  1         // the merge look-ahead one window short: `cur` closed a window early
#define WA_SVAD_WRONG_PAD_FIRST  2         // padding decided before the merge (the gap test sees padded ends)
#define WA_SVAD_WRONG_LE         3         // <= for < at 3200

// what open checks: false + a reason
inline bool wa_svad_params_ok(const whisper_vad_params & p, int max_utterance_ms, const char ** why) {
    const char * w = nullptr;
    if (max_utterance_ms <= 0 || max_utterance_ms > WA_SVAD_MAX_UTTERANCE_MS) w = "max_utterance_ms outside (0, 30000]";
    else if (p.speech_pad_ms < 0 || p.speech_pad_ms > WA_SVAD_MAX_PAD_MS) w = "speech_pad_ms outside [0, 100]";
    else if (p.min_speech_duration_ms < 0 || p.min_silence_duration_ms < 0 || p.min_speech_duration_ms > 1000000 || p.min_silence_duration_ms > 1000000)
        w = "a negative or absurd min_speech_duration_ms / min_silence_duration_ms";
    else if (!(p.max_speech_duration_s * 1000.0f <= (float) max_utterance_ms)) w = "max_speech_duration_s above max_utterance_ms";
    else if ((int64_t) WHISPER_SAMPLE_RATE * (int64_t) p.max_speech_duration_s - WA_VAD_WINDOW - 2 * (WHISPER_SAMPLE_RATE * p.speech_pad_ms / 1000) < 0)
        w = "max_speech_duration_s too small to bound a speech (the reference then drops the bound)";
    if (why) *why = w;
    return w == nullptr;
}

struct wa_svad_range { int64_t start = 0, len = 0; };
inline wa_svad_range wa_svad_range_of(const wa_vad_seg & g, int64_t T) {
    wa_svad_range r;
    r.start = wa_vad_cs_to_samples(g.start);
    int64_t end = wa_vad_cs_to_samples(g.end);
    if (T >= 0 && end > T) end = T;
    r.len = end > r.start ? end - r.start : 0;
    return r;
}

inline int wa_svad_delay_bound(const whisper_vad_params & p) {
    const int ms = WHISPER_SAMPLE_RATE * p.min_silence_duration_ms / 1000;
    const int a = (ms + WA_VAD_WINDOW - 1) / WA_VAD_WINDOW * WA_VAD_WINDOW + WA_VAD_WINDOW;
    const int b = (WA_SVAD_MERGE_GAP + WA_VAD_WINDOW - 1) / WA_VAD_WINDOW * WA_VAD_WINDOW;
    return a > b ? a : b;
}

struct wa_svad_out {
    wa_vad_seg seg;            // centiseconds, as wa_vad_segments_from_probs gives them
    int raw_end = 0;           // where the segment's last raw speech ended, before padding (samples)
    bool split = false;        // closed by the cap: the next utterance continues the same speech
};

struct wa_svad_segmenter {
    // the reference's constants
    float threshold = 0.5f, neg_threshold = 0.35f;
    int min_silence_samples = 0, min_speech_samples = 0, speech_pad_samples = 0, max_speech_samples = 0, min_silence_samples_at_max_speech = 0;
    int64_t cap_samples = 0;
    int wrong = 0;
    // the first pass's variables
    bool is_speech_segment = false, has_curr_speech = false;
    int temp_end = 0, prev_end = 0, next_start = 0, curr_speech_start = 0;
    int n_probs = 0;
    // the merge pass's
    bool has_cur = false;
    int cur_start = 0, cur_end = 0, cur_start_pad = 0, cur_end_pad = 0;
    int next_start_pad = 0;            // the start pad of the speech that follows a split
    bool cur_split = false;
    int64_t splits = 0;
    int64_t T_end = -1;                // the flush's T: what the last utterance's range is clamped to

    void init(const whisper_vad_params & params, int max_utterance_ms, int wrong_ = 0) {
        *this = wa_svad_segmenter();
        wrong = wrong_;
        const int sample_rate = WHISPER_SAMPLE_RATE, n_window = WA_VAD_WINDOW;
        threshold = params.threshold;
        min_silence_samples = sample_rate * params.min_silence_duration_ms / 1000;
        min_speech_samples  = sample_rate * params.min_speech_duration_ms / 1000;
        speech_pad_samples  = sample_rate * params.speech_pad_ms / 1000;
        if (params.max_speech_duration_s > 100000.0f) max_speech_samples = INT_MAX / 2;
        else {
            const int64_t temp = (int64_t) sample_rate * (int64_t) (params.max_speech_duration_s) - n_window - 2 * speech_pad_samples;
            max_speech_samples = (temp > INT_MAX) ? INT_MAX / 2 : (int) temp;
            if (max_speech_samples < 0) max_speech_samples = INT_MAX / 2;
        }
        min_silence_samples_at_max_speech = sample_rate * 98 / 1000;
        neg_threshold = threshold - 0.15f;
        if (neg_threshold < 0.01f) neg_threshold = 0.01f;
        cap_samples = (int64_t) max_utterance_ms * (sample_rate / 1000);
        next_start_pad = speech_pad_samples;
    }
    void reset() {
        is_speech_segment = has_curr_speech = false;
        temp_end = prev_end = next_start = curr_speech_start = 0;
        n_probs = 0;
        has_cur = cur_split = false;
        cur_start = cur_end = cur_start_pad = cur_end_pad = 0;
        next_start_pad = speech_pad_samples;
        splits = 0;
        T_end = -1;
    }

    // `cur` leaves: the min_speech erase, then the padding, then centiseconds.  audio_len < 0: not known yet and cannot bind.
    void close_cur(std::vector<wa_svad_out> & out, int64_t audio_len) {
        if (!has_cur) return;
        has_cur = false;
        if (cur_end - cur_start < min_speech_samples) return;
        const int start = cur_start > cur_start_pad ? cur_start - cur_start_pad : 0;
        int end = cur_end + cur_end_pad;
        if (audio_len >= 0 && !((int64_t) end < audio_len)) end = (int) audio_len;
        wa_svad_out o;
        o.seg.start = wa_vad_samples_to_cs(start);
        o.seg.end   = wa_vad_samples_to_cs(end);
        o.raw_end = cur_end;
        o.split = cur_split;
        out.push_back(o);
    }
    void open_cur(int start, int end) {
        has_cur = true; cur_split = false;
        cur_start = start; cur_end = end;
        cur_start_pad = next_start_pad; cur_end_pad = speech_pad_samples;
        next_start_pad = speech_pad_samples;
    }
    // a raw speech of the first pass
    void raw(int start, int end, std::vector<wa_svad_out> & out) {
        if (has_cur) {
            int gap = start - cur_end;
            if (wrong == WA_SVAD_WRONG_PAD_FIRST) gap -= 2 * speech_pad_samples;
            const bool close = wrong == WA_SVAD_WRONG_LE ? gap <= WA_SVAD_MERGE_GAP : gap < WA_SVAD_MERGE_GAP;
            if (close) {
                wa_vad_seg joined;
                joined.start = wa_vad_samples_to_cs(cur_start > cur_start_pad ? cur_start - cur_start_pad : 0);
                joined.end   = wa_vad_samples_to_cs(end + speech_pad_samples);
                if (wa_svad_range_of(joined, -1).len <= cap_samples) { cur_end = end; return; }
                // the cap: the merge is not made; the close-neighbour padding rule at this boundary
                const int silence = start - cur_end;
                if (silence < 2 * speech_pad_samples) { cur_end_pad = silence / 2; next_start_pad = silence / 2; }
                cur_split = true;
                ++splits;
            }
            close_cur(out, -1);
        }
        open_cur(start, end);
    }

    // the probability of window n_probs; appends what became final
    void push(float curr_prob, std::vector<wa_svad_out> & out) {
        const int i = n_probs++;
        step(curr_prob, WA_VAD_WINDOW * i, out);
        if (!has_cur) return;
        const int seen = WA_VAD_WINDOW * (wrong == WA_SVAD_WRONG_LOOKAHEAD ? i + 2 : i + 1);       // where the next window starts
        const int need = WA_SVAD_MERGE_GAP + (wrong == WA_SVAD_WRONG_PAD_FIRST ? 2 * speech_pad_samples : 0);
        const bool cand_far = is_speech_segment && curr_speech_start - cur_end >= need;
        if ((!is_speech_segment || cand_far) && seen - cur_end >= need) close_cur(out, -1);
    }
    // the loop body of whisper.cpp:5263-5352, statement for statement; speeches.push_back is raw()
    void step(float curr_prob, int curr_sample, std::vector<wa_svad_out> & out) {
        if ((curr_prob >= threshold) && temp_end) {
            temp_end = 0;
            if (next_start < prev_end) next_start = curr_sample;
        }
        if ((curr_prob >= threshold) && !is_speech_segment) {
            is_speech_segment = true;
            curr_speech_start = curr_sample;
            has_curr_speech = true;
            return;
        }
        if (is_speech_segment && (curr_sample - curr_speech_start) > max_speech_samples) {
            if (prev_end) {
                raw(curr_speech_start, prev_end, out);
                has_curr_speech = true;
                if (next_start < prev_end) { is_speech_segment = false; has_curr_speech = false; }
                else curr_speech_start = next_start;
                prev_end = next_start = temp_end = 0;
            } else {
                raw(curr_speech_start, curr_sample, out);
                prev_end = next_start = temp_end = 0;
                is_speech_segment = false;
                has_curr_speech = false;
                return;
            }
        }
        if ((curr_prob < neg_threshold) && is_speech_segment) {
            if (!temp_end) temp_end = curr_sample;
            if ((curr_sample - temp_end) > min_silence_samples_at_max_speech) prev_end = temp_end;
            if ((curr_sample - temp_end) < min_silence_samples) return;
            if ((temp_end - curr_speech_start) > min_speech_samples) raw(curr_speech_start, temp_end, out);
            prev_end = next_start = temp_end = 0;
            is_speech_segment = false;
            has_curr_speech = false;
            return;
        }
    }
    // the end of input: T samples, whose windows - the last one zero-filled - have all been pushed.  The list's own clamp is
    // audio_length_samples = n_probs * 512; T clamps the utterance ranges (wa_svad_range_of(seg, T_end))
    void flush(int64_t T, std::vector<wa_svad_out> & out) {
        T_end = T;
        const int audio_length_samples = n_probs * WA_VAD_WINDOW;
        if (has_curr_speech && (audio_length_samples - curr_speech_start) > min_speech_samples) raw(curr_speech_start, audio_length_samples, out);
        is_speech_segment = has_curr_speech = false;
        close_cur(out, audio_length_samples);
    }
};

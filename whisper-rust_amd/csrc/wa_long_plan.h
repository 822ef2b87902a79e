// wa_long_plan.h - the layout of the speech-only audio of a list of VAD segments, and the chunk planner of whisper_amd_full_long
// (DESIGN.md 4.11).  Pure host arithmetic, no HIP include: tests/native/long_plan.cpp compiles it with g++ alone.
//
// wa_vad_layout_make is the ONE statement of the length, piece and table arithmetic of the reference's VAD step (whisper.cpp:6644-6790):
// wa_vad_filter_audio (wa_vad_host.cpp) copies what it lists on the host, k_long_pack (wa_long.hip) on the device, and the planner
// below asks it for lengths.  For a list of n segments and the caller's n_samples:
//   - segment i covers samples [cs_to_samples(start), cs_to_samples(end) + (i < n - 1 ? overlap : 0)); the LAST segment of the list gets
//     no overlap extension, and no silence follows it;
//   - the length handed to the transcription sums these with the end clamped to n_samples - 1, plus 0.1 s of silence per gap; the copy
//     clamps the start to n_samples - 1 and the end to n_samples, and skips a segment that is left with no sample (its silence too).  So a
//     last segment that reaches the end of the audio copies one sample more than was counted - the reference writes it past its vector's
//     size - and it is cut off here: pieces are clipped to the length, samples of [0, length) that no piece covers are zero;
//   - the table maps centiseconds of the speech-only audio to the caller's: both ends of every copied segment, a point every 200 ms inside
//     segments longer than 1 s, both ends of every silence; sorted by processed time, first entry of equal times kept.
//
// Chunks (wa_long_plan): greedy, in order.  A chunk is a run [first, first + count) of consecutive segments; it takes the next segment while
// the length of the run - by the rules above, with the run as the list - stays <= max_chunk_samples.  A single segment longer than the cap
// is a chunk of its own (whisper_full's window loop covers it).  A chunk shorter than 100 ms yields no result segments, as whisper_full on it
// would; nothing is padded.
#pragma once

#include "wa_vad.h"

#include <algorithm>
#include <cstdint>
#include <vector>

inline int     wa_vad_cs_to_samples(int64_t cs)  { return (int) ((cs / 100.0) * WHISPER_SAMPLE_RATE + 0.5); }
inline int64_t wa_vad_samples_to_cs(int samples) { return (int64_t) ((samples / (double) WHISPER_SAMPLE_RATE) * 100.0 + 0.5); }

struct wa_long_piece {          // `len` samples at `dst` of the speech-only audio come from `src` of the caller's audio; src = -1: zeros
    int64_t dst, src, len;
};

// the length handed to the transcription (never negative)
inline int wa_vad_layout_length(const wa_vad_seg * segs, int n_seg, float samples_overlap, int n_samples) {
    if (n_seg <= 0) return 0;
    const int overlap_samples = samples_overlap * WHISPER_SAMPLE_RATE;
    int filtered_n_samples = 0;
    for (int i = 0; i < n_seg; i++) {
        const int segment_start_samples = wa_vad_cs_to_samples(segs[i].start);
        int segment_end_samples = wa_vad_cs_to_samples(segs[i].end);
        if (i < n_seg - 1) segment_end_samples += overlap_samples;
        segment_end_samples = std::min(segment_end_samples, n_samples - 1);
        filtered_n_samples += (segment_end_samples - segment_start_samples);
    }
    const int silence_samples = 0.1 * WHISPER_SAMPLE_RATE;
    const int total_silence_samples = (n_seg > 1) ? (n_seg - 1) * silence_samples : 0;
    return std::max(filtered_n_samples + total_silence_samples, 0);
}

// returns that length; `pieces` (when given) receives the copies in ascending dst order, clipped to it, silences included;
// `table` (when given) the mapping table
inline int wa_vad_layout_make(const wa_vad_seg * segs, int n_seg, float samples_overlap, int n_samples, std::vector<wa_long_piece> * pieces,
                              std::vector<wa_vad_map_point> * table) {
    if (pieces) pieces->clear();
    if (table) table->clear();
    if (n_seg <= 0) return 0;
    const int total = wa_vad_layout_length(segs, n_seg, samples_overlap, n_samples);
    const int overlap_samples = samples_overlap * WHISPER_SAMPLE_RATE;
    const int silence_samples = 0.1 * WHISPER_SAMPLE_RATE;
    if (table) table->reserve((size_t) n_seg * 4);
    auto put = [&](int64_t dst, int64_t src, int64_t len) {
        len = std::min<int64_t>(len, (int64_t) total - dst);
        if (pieces && len > 0) pieces->push_back({ dst, src, len });
    };

    int offset = 0;
    for (int i = 0; i < n_seg; i++) {
        int segment_start_samples = wa_vad_cs_to_samples(segs[i].start);
        int segment_end_samples   = wa_vad_cs_to_samples(segs[i].end);
        if (i < n_seg - 1) segment_end_samples += overlap_samples;
        segment_start_samples = std::min(segment_start_samples, n_samples - 1);
        segment_end_samples   = std::min(segment_end_samples, n_samples);
        const int segment_length = segment_end_samples - segment_start_samples;
        if (segment_length <= 0) continue;

        if (table) {
            const int64_t orig_start = segs[i].start, orig_end = segs[i].end;
            const int64_t vad_start = wa_vad_samples_to_cs(offset), vad_end = wa_vad_samples_to_cs(offset + segment_length);
            table->push_back({ vad_start, orig_start });
            table->push_back({ vad_end, orig_end });

            const int64_t min_segment_length = 100, point_interval = 20;     // a point every 200 ms inside segments longer than 1 s
            if (vad_end - vad_start > min_segment_length) {
                const int64_t segment_duration = vad_end - vad_start;
                const int num_points = (int) (segment_duration / point_interval) - 1;
                for (int j = 1; j <= num_points; j++) {
                    const int64_t vad_time = vad_start + j * point_interval;
                    if (vad_time >= vad_end) continue;
                    const int64_t vad_elapsed = vad_time - vad_start, vad_total = vad_end - vad_start, orig_total = orig_end - orig_start;
                    table->push_back({ vad_time, orig_start + (vad_elapsed * orig_total) / vad_total });
                }
            }
        }
        put(offset, segment_start_samples, segment_length);
        offset += segment_length;

        if (i < n_seg - 1) {
            if (table) {
                table->push_back({ wa_vad_samples_to_cs(offset), segs[i].end });
                table->push_back({ wa_vad_samples_to_cs(offset + silence_samples), segs[i + 1].start });
            }
            put(offset, -1, silence_samples);
            offset += silence_samples;
        }
    }
    if (table) {
        std::sort(table->begin(), table->end(), [](const wa_vad_map_point & a, const wa_vad_map_point & b) { return a.processed_time < b.processed_time; });
        table->erase(std::unique(table->begin(), table->end(), [](const wa_vad_map_point & a, const wa_vad_map_point & b) { return a.processed_time == b.processed_time; }), table->end());
    }
    return total;
}

struct wa_long_chunk {
    int first, count;           // segments [first, first + count)
    int packed;                 // wa_vad_layout_length of that run
};

inline std::vector<wa_long_chunk> wa_long_plan(const wa_vad_seg * segs, int n_seg, int n_samples, float samples_overlap, int max_chunk_samples) {
    std::vector<wa_long_chunk> plan;
    for (int first = 0; first < n_seg;) {
        int count = 1, packed = wa_vad_layout_length(segs + first, 1, samples_overlap, n_samples);
        while (first + count < n_seg) {
            const int next = wa_vad_layout_length(segs + first, count + 1, samples_overlap, n_samples);
            if (next > max_chunk_samples) break;
            packed = next;
            ++count;
        }
        plan.push_back({ first, count, packed });
        first += count;
    }
    return plan;
}

// wa_long_host.h - long recordings: what wa_long.cpp keeps on a state, and the steps of whisper_amd_full_long that
// whisper_amd_full_long_channels (wa_channels.cpp) runs too: the pack of every chunk in one launch, the lock-step waves, the time mapping.
#pragma once

#include "wa_internal.h"
#include "wa_long.h"

struct wa_long_rec {
    int first = 0, count = 0, packed = 0;      // segments [first, first + count) of its source's list, samples of speech-only audio
    int64_t off = 0;                           // its first float in d_chunks (a multiple of WA_LONG_ALIGN)
    int64_t t0 = 0, t1 = 0;                    // the caller's centiseconds: start of the first segment, end of the last
    int n_result = 0;                          // result segments it gave
    int channel = -1;                          // whisper_amd_full_long_channels: the channel it was cut from; -1: a call without channels
    std::vector<wa_vad_map_point> table;
};

struct wa_long_state {
    float * d_pcm = nullptr; size_t d_pcm_cap = 0;                  // host PCM, uploaded once
    float * d_chunks = nullptr; size_t d_chunks_cap = 0;            // every chunk of the last call
    wa_long_piece * d_pieces = nullptr; size_t d_pieces_cap = 0;    // the pack kernel's table
    std::vector<wa_long_rec> chunks;                                // the last call's
    int64_t stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };                  // whisper_amd_long_stats; [1] counts since the state was created
    int64_t n_pack_launches = 0;                                    // k_long_pack launches since the state was created
    std::vector<int8_t> seg_channel;                                // whisper_amd_full_long_channels: channel of every result segment; else empty
};

wa_long_state & wa_long_of(whisper_state & st);

// One source of chunks: a segment list over n_samples of audio that starts src_off floats into the buffer handed to wa_long_pack, and its plan.
struct wa_long_src {
    const wa_vad_seg * segs;
    int n_samples;
    int64_t src_off;
    int channel;
    const std::vector<wa_long_chunk> * plan;
};
struct wa_long_pick { int src, chunk; };       // chunk `chunk` of source `src`'s plan

// The chunks `order` names, in that order, into the state's chunk buffer and chunk list, in ONE launch (where = 1) or by the host function
// (where = 0).  One of h_samples / d_samples may be null: the kernel path uploads host audio first, the host path copies device audio down;
// h_samples is taken for a single source at offset 0 only.  Complete - synchronised - on return.
bool wa_long_pack(whisper_state & st, const float * h_samples, const float * d_samples, const std::vector<wa_long_src> & srcs,
                  const std::vector<wa_long_pick> & order, float samples_overlap, int where);

// wa_long_pack by the kernel unless WHISPER_AMD_LONG_HOST=1 is set (read here), by the host function when the kernel path fails (logged, counted)
bool wa_long_pack_any(whisper_state & st, const float * h_samples, const float * d_samples, const std::vector<wa_long_src> & srcs,
                      const std::vector<wa_long_pick> & order, float samples_overlap, const char * who);

// The state's chunk list in waves of n_parallel through the lock-step groups: results[c] receives chunk c's segments with their own times.
// Returns 0, or the first non-zero chunk code with the chunk list cleared; -1 when a member state could not be made.
int wa_long_waves(whisper_context * ctx, const whisper_full_params & params, int n_parallel, std::vector<std::vector<wa_segment>> & results);

// a result segment's times into the caller's audio through its chunk's table: at least 10 cs; token t0 / t1 / t_dtw that are >= 0 too
void wa_long_map_segment(wa_segment & seg, const std::vector<wa_vad_map_point> & table);

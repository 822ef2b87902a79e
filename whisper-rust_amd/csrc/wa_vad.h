// wa_vad.h - voice activity detection (Silero VAD as whisper.cpp 1.7.5 runs it): the host part.
//
// Behavioural contract: sys/whisper.cpp/src/whisper.cpp:4534-5450 (model, graph, detect_speech, segments_from_probs),
// 6615-6793 (the speech-only audio that whisper_full transcribes, with its time-mapping table), 7882-7960 (mapping a time back).
// The model is one shape only - the one the reference's graph hard-codes:
//   512-sample windows, reflect pad 64, STFT basis F16 [256,1,258] at stride 128 (4 frames), magnitude [4,129],
//   Conv1d k=3 pad=1: 129->128 s1, 128->64 s2, 64->64 s2, 64->128 s1 (F16 weights, F32 biases, ReLU),
//   LSTM 128->128 (F32 weights), final 128->1 (F16 weight), sigmoid.
// Split ("VAD"): everything that depends on one window alone - up to W_ih x + b_ih - is the device's k_vad_front
// (wa_vad.hip); the recurrence, which calls libm's expf and tanhf as the reference does, runs here on the host.
// Plain C++ (no HIP, no device types): tests/native/vad_math.cpp compiles wa_vad_host.cpp alone.
#pragma once

#include "../../include/whisper_amd.h"

#include <cstdint>
#include <string>
#include <vector>

#define WA_VAD_WINDOW 512      // samples per probability
#define WA_VAD_PAD    64       // reflect padding on both sides
#define WA_VAD_NFFT   256      // STFT kernel length
#define WA_VAD_HOP    128      // STFT stride (= lstm_input_size in the reference's graph)
#define WA_VAD_BINS   129      // magnitude channels; the basis has 2 x 129 rows
#define WA_VAD_HID    128      // LSTM width
#define WA_VAD_GATES  512      // 4 x WA_VAD_HID, gate order i, f, g, o

struct wa_vad_model {
    int32_t n_window = 0, n_context = 0;       // n_context is stored in the file and used nowhere (as in the reference)
    std::string type, version;
    std::vector<uint16_t> stft;                // F16 [258][256]
    std::vector<uint16_t> enc_w[4];            // F16 [C_out][C_in * 3], index ic * 3 + k: the order of an im2col row
    std::vector<float>    enc_b[4];
    std::vector<float>    w_ih, b_ih, w_hh, b_hh;   // F32 [512][128], [512]
    std::vector<uint16_t> w_f;                 // F16 [128]
    float                 b_f = 0.0f;
};
static const int WA_VAD_ENC_IN[4]     = { 129, 128, 64, 64 };
static const int WA_VAD_ENC_OUT[4]    = { 128, 64, 64, 128 };
static const int WA_VAD_ENC_STRIDE[4] = { 1, 2, 2, 1 };

// false + a reason in `err` for anything but the shape above (the reason names that shape), a truncated file, a missing tensor
bool wa_vad_model_load(whisper_model_loader * loader, wa_vad_model & m, std::string & err);

inline int wa_vad_n_chunks(int n_samples) { return n_samples / WA_VAD_WINDOW + (n_samples % WA_VAD_WINDOW != 0 ? 1 : 0); }

// LSTM state of one whisper_vad_detect_speech call; zero at its start
struct wa_vad_lstm {
    float h[WA_VAD_HID], c[WA_VAD_HID];
    void reset() { for (int i = 0; i < WA_VAD_HID; ++i) h[i] = c[i] = 0.0f; }
};
// one window: gate_in = W_ih x + b_ih (512 values, the front end's output); returns the speech probability and advances the state
float wa_vad_step(const wa_vad_model & m, wa_vad_lstm & s, const float * gate_in);

struct wa_vad_seg { int64_t start, end; };                  // centiseconds
std::vector<wa_vad_seg> wa_vad_segments_from_probs(const float * probs, int n_probs, int n_window, const whisper_vad_params & params);

struct wa_vad_map_point { int64_t processed_time, original_time; };    // centiseconds in the speech-only audio / in the caller's audio
// the audio whisper_full transcribes when vad = true (speech segments, 0.1 s of silence between them) and its table;
// `filtered` stays empty when there is no segment.  Lengths, pieces and table are wa_long_plan.h's wa_vad_layout_make, which the chunk planner and
// the pack kernel of whisper_amd_full_long use too
void wa_vad_filter_audio(const std::vector<wa_vad_seg> & segs, float samples_overlap, const float * samples, int n_samples,
                         std::vector<float> & filtered, std::vector<wa_vad_map_point> & table);
int64_t wa_vad_map_time(int64_t processed_time, const std::vector<wa_vad_map_point> & table);

// -------------------------------------------------------------------------------------------------
// device front end (wa_vad.hip).  No HIP types here: the stream travels as void *.
// -------------------------------------------------------------------------------------------------
#define WA_VAD_TILE   8        // windows per workgroup of k_vad_front (exported: whisper_amd_vad_tile)
#define WA_VAD_LD0    392      // device row stride (halfs) of encoder layer 0's weights: K = 387 padded to a multiple of 8

struct wa_vad_dev {            // device pointers; F16 rows of K halfs (layer 0: WA_VAD_LD0), index ic * 3 + k
    const uint16_t * stft = nullptr, * enc_w[4] = { nullptr, nullptr, nullptr, nullptr };
    const float    * enc_b[4] = { nullptr, nullptr, nullptr, nullptr }, * w_ih = nullptr, * b_ih = nullptr;
};
// out[c][512] = W_ih x_c + b_ih for windows c < n_chunks of d_samples; samples at and past n_valid count as zero
bool wa_vad_front_launch(const wa_vad_dev & w, const float * d_samples, int n_valid, int n_chunks, float * d_out, void * stream);

// The same front end on the ring windows of several live sessions in ONE launch (k_stream_vad_front; wa_stream_vad.cpp).
// Session i contributes first[i + 1] - first[i] consecutive windows: sample q of them lies in ring slot (slot + q) mod cap and counts as zero at
// and past n_valid (the partial window of a flush).  Window k's 512 gate inputs go to out + 512 k, memory the device can write (the session's
// pinned host buffer).  The table travels as a kernel argument.
#define WA_SVAD_SESSIONS     8        // sessions per launch
#define WA_SVAD_MAX_WINDOWS  1024     // windows of one session per launch (32 s of audio)
struct wa_svad_session {
    const float * ring;
    float * out;
    int32_t cap, slot, n_valid, pad_;
};
struct wa_svad_table {
    wa_svad_session s[WA_SVAD_SESSIONS];
    int32_t first[WA_SVAD_SESSIONS + 1];      // prefix counts of the flat (session, window) list; first[0] = 0
    int32_t n_sessions;
};
// false: the table is refused (nothing was launched) or the launch failed.  The caller has made sure the ring holds the samples.
bool wa_svad_front_launch(const wa_vad_dev & w, const wa_svad_table & t, void * stream);

// wa_dtw_host.h - the arithmetic of the DTW token timestamps on the host (wa_dtw_host.cpp; no HIP, no device: tests/native/dtw_math.cpp
// compiles it alone).  It is what the goldens pin to the reference engine, the fallback of the device path and the yardstick of its kernels.
//
// ref: whisper_exp_compute_token_level_timestamps_dtw whisper.cpp:8864-8892, dtw_and_backtrace 8647-8731, median_filter 8737-8770.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

// The alignment heads' cross-attention probabilities where they lie: x(k, t, j) = base[head_off[k] + t * tok_stride + j] for head k < n_heads,
// token t < n_tokens and audio index j < n_ctx.  The capture buffer [slot][token][head][n_ctx] is such a view without a copy (head_off =
// (slot, head) offsets, tok_stride = H * n_ctx); so is a plain cube [n_heads][n_tokens][n_ctx].
struct wa_dtw_view {
    const float * base;
    const long long * head_off;
    int n_heads;
    long long tok_stride;
    int n_tokens;
    int n_ctx;
};

// codes of whisper_amd_dtw_path (include/whisper_amd.h)
enum { WA_DTW_REFUSED = -1, WA_DTW_NOT_TAKEN = -2, WA_DTW_HIP_ERROR = -3 };

typedef std::vector<std::pair<int32_t, int32_t>> wa_dtw_path_t;       // (token index, time index), in path order

// what every path refuses: an even or non-positive width, M <= width (too few frames for the median filter), M > n_ctx, N = n_tokens - sot_len - 1 <= 0
bool wa_dtw_args_ok(int n_heads, int n_tokens, int n_ctx, int M, int sot_len, int medfilt_width);

// normalise over tokens, median over audio (reflect padding), mean over heads times -1: cost_in[t][j], t < n_tokens, j < M
void wa_dtw_host_cost(const wa_dtw_view & v, int M, int medfilt_width, std::vector<float> & cost_in);

// cost and trace table over rows [sot_len, sot_len + N) of cost_in; trace(i, j) in {0, 1, 2} at trace[j * (N + 1) + i], 0 <= i <= N, 0 <= j <= M
void wa_dtw_host_table(const float * cost_in, int M, int sot_len, int N, std::vector<uint8_t> & trace);

// The path from a trace whose cell (i, j), 1 <= i <= N, 1 <= j <= M, is tr11[(i - 1) * si + (j - 1) * sj]; the borders are the table's own
// (row 0: 2, column 0: 1) and are not read.  The host table above: tr11 = &trace[N + 2], si = 1, sj = N + 1.
void wa_dtw_backtrace(const uint8_t * tr11, long long si, long long sj, int N, int M, wa_dtw_path_t & path);

// all of it; the path length, or WA_DTW_REFUSED.  cost_out (may be null) receives cost_in.
int wa_dtw_host_path(const wa_dtw_view & v, int M, int sot_len, int medfilt_width, wa_dtw_path_t & path, std::vector<float> * cost_out = nullptr);

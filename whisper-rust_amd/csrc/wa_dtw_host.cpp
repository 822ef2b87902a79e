// wa_dtw_host.cpp - DTW token timestamps, host arithmetic (see wa_dtw_host.h).  No HIP include: tests/native/dtw_math.cpp links this file alone.
//
// The steps are the reference's, in its arithmetic order (F64 sums of ggml_norm / ggml_mean, single-rounded F32 steps):
//   ggml_norm over the token axis, eps 1e-9 (whisper.cpp:8864, ops.cpp:3225-3242);
//   7-wide median over the audio axis with reflect padding, per token (whisper.cpp:8737-8770).  The median of 7 is a 13-exchange selection
//   network on a row of frames (it vectorises); other widths sort;
//   mean over heads (F64 sum in head order, ops.cpp:2033-2041 / vec.h:908-914), times -1;
//   DTW + backtrace (whisper.cpp:8647-8731).
#include "wa_dtw_host.h"

#include <algorithm>
#include <cmath>
#include <thread>

bool wa_dtw_args_ok(int n_heads, int n_tokens, int n_ctx, int M, int sot_len, int medfilt_width) {
    if (n_heads <= 0 || n_tokens <= 0 || sot_len < 0 || medfilt_width <= 0 || medfilt_width % 2 == 0) return false;
    if (M <= 0 || M > n_ctx || medfilt_width >= M) return false;
    return n_tokens - sot_len - 1 > 0;
}

void wa_dtw_host_cost(const wa_dtw_view & v, int M, int medfilt_width, std::vector<float> & cost_in) {
    const int n_heads = v.n_heads, n_tokens = v.n_tokens, n_audio_tokens = M;
    // the heads token-fastest: w[t + n_tokens*(j + n_audio_tokens*k)] (layout of aheads_cross_QKs, whisper.cpp:8844-8856)
    std::vector<float> w((size_t) n_tokens * n_audio_tokens * n_heads);
    for (int k = 0; k < n_heads; ++k)
        for (int t = 0; t < n_tokens; ++t) {
            const float * row = v.base + v.head_off[k] + (long long) t * v.tok_stride;
            for (int j = 0; j < n_audio_tokens; ++j) w[t + (size_t) n_tokens * (j + (size_t) n_audio_tokens * k)] = row[j];
        }

    // Per alignment head (independent: spread over a few host threads - a medium model's 32 heads x 223 tokens x 750 frames took ~0.5 s
    // in one thread with a sort per median)
    std::vector<float> med((size_t) n_heads * n_tokens * n_audio_tokens);  // med[kk][t][j]
    auto one_head = [&](int kk) {
        for (int j = 0; j < n_audio_tokens; ++j) {
            float * x = &w[(size_t) n_tokens * (j + (size_t) n_audio_tokens * kk)];
            double sum = 0.0;
            for (int t = 0; t < n_tokens; ++t) sum += (double) x[t];
            const float mean = sum / n_tokens;
            double sum2 = 0.0;
            for (int t = 0; t < n_tokens; ++t) { const float v = x[t] - mean; x[t] = v; sum2 += (double) (v * v); }
            const float variance = sum2 / n_tokens;
            const float scale = 1.0f / sqrtf(variance + 1e-9f);
            for (int t = 0; t < n_tokens; ++t) x[t] = x[t] * scale;
        }
        const int hw = medfilt_width / 2, M_ = n_audio_tokens;
        std::vector<float> row((size_t) M_ + 2 * hw), filt((size_t) medfilt_width);
        for (int t = 0; t < n_tokens; ++t) {
            for (int j = 0; j < M_; ++j) row[hw + j] = w[t + (size_t) n_tokens * (j + (size_t) M_ * kk)];
            for (int o = 1; o <= hw; ++o) { row[hw - o] = row[hw + o]; row[hw + M_ - 1 + o] = row[hw + M_ - 1 - o]; }      // reflect (idx -> -idx, 2 (M - 1) - idx)
            float * out = &med[((size_t) kk * n_tokens + t) * M_];
            if (medfilt_width == 7) {
                const float * r = row.data();
                for (int j = 0; j < M_; ++j) {
                    float p0 = r[j], p1 = r[j + 1], p2 = r[j + 2], p3 = r[j + 3], p4 = r[j + 4], p5 = r[j + 5], p6 = r[j + 6];
#define WA_CX(a, b) do { const float lo_ = std::min(a, b), hi_ = std::max(a, b); a = lo_; b = hi_; } while (0)
                    WA_CX(p0, p5); WA_CX(p0, p3); WA_CX(p1, p6); WA_CX(p2, p4); WA_CX(p0, p1); WA_CX(p3, p5); WA_CX(p2, p6);
                    WA_CX(p2, p3); WA_CX(p3, p6); WA_CX(p4, p5); WA_CX(p1, p4); WA_CX(p1, p3); WA_CX(p3, p4);
#undef WA_CX
                    out[j] = p3;
                }
            } else {
                for (int j = 0; j < M_; ++j) {
                    std::copy(row.begin() + j, row.begin() + j + medfilt_width, filt.begin());
                    std::sort(filt.begin(), filt.end());
                    out[j] = filt[filt.size() / 2];
                }
            }
        }
    };
    {
        const int n_thr = std::max(1, std::min(n_heads, 8));
        std::vector<std::thread> th;
        for (int i = 1; i < n_thr; ++i) th.emplace_back([&, i] { for (int kk = i; kk < n_heads; kk += n_thr) one_head(kk); });
        for (int kk = 0; kk < n_heads; kk += n_thr) one_head(kk);
        for (auto & t_ : th) t_.join();
    }
    // mean over heads (F64 sum in head order), times -1
    cost_in.assign((size_t) n_tokens * n_audio_tokens, 0.0f);               // x[t][j]
    for (int t = 0; t < n_tokens; ++t)
        for (int j = 0; j < n_audio_tokens; ++j) {
            double sum = 0.0;
            for (int kk = 0; kk < n_heads; ++kk) sum += (double) med[((size_t) kk * n_tokens + t) * n_audio_tokens + j];
            float v = (float) sum;
            v /= (float) n_heads;
            cost_in[(size_t) t * n_audio_tokens + j] = v * -1.0f;
        }
}

void wa_dtw_host_table(const float * cost_in, int M, int sot_len, int N, std::vector<uint8_t> & trace) {
    // drop the sot sequence and eot (whisper.cpp:8880-8882): rows [sot_len, n_tokens - 1)
    const int n_audio_tokens = M;
    auto X = [&](int i, int j) { return cost_in[(size_t) (i + sot_len) * n_audio_tokens + j]; };

    std::vector<float> cost((size_t) (N + 1) * (M + 1), INFINITY);
    trace.assign((size_t) (N + 1) * (M + 1), 0xff);
    auto C = [&](int i, int j) -> float & { return cost[(size_t) j * (N + 1) + i]; };
    auto TR = [&](int i, int j) -> uint8_t & { return trace[(size_t) j * (N + 1) + i]; };
    C(0, 0) = 0.0f;
    for (int j = 1; j < M + 1; ++j)
        for (int i = 1; i < N + 1; ++i) {
            const float c0 = C(i - 1, j - 1), c1 = C(i - 1, j), c2 = C(i, j - 1);
            float c; uint8_t t;
            if (c0 < c1 && c0 < c2) { c = c0; t = 0; } else if (c1 < c0 && c1 < c2) { c = c1; t = 1; } else { c = c2; t = 2; }
            C(i, j) = X(i - 1, j - 1) + c;
            TR(i, j) = t;
        }
    for (int j = 0; j < M + 1; ++j) TR(0, j) = 2;
    for (int i = 0; i < N + 1; ++i) TR(i, 0) = 1;
}

void wa_dtw_backtrace(const uint8_t * tr11, long long si, long long sj, int N, int M, wa_dtw_path_t & path) {
    path.clear();                           // built backwards
    int i = N, j = M;
    while (i > 0 || j > 0) {
        path.emplace_back(i - 1, j - 1);
        const int t = i == 0 ? 2 : j == 0 ? 1 : tr11[(i - 1) * si + (j - 1) * sj];      // TR(0, j) = 2, TR(i, 0) = 1
        if (t == 0) { --i; --j; } else if (t == 1) { --i; } else if (t == 2) { --j; } else break;
    }
    std::reverse(path.begin(), path.end());
}

int wa_dtw_host_path(const wa_dtw_view & v, int M, int sot_len, int medfilt_width, wa_dtw_path_t & path, std::vector<float> * cost_out) {
    path.clear();
    if (!wa_dtw_args_ok(v.n_heads, v.n_tokens, v.n_ctx, M, sot_len, medfilt_width)) return WA_DTW_REFUSED;
    const int N = v.n_tokens - sot_len - 1;
    std::vector<float> cost_in;
    wa_dtw_host_cost(v, M, medfilt_width, cost_in);
    std::vector<uint8_t> trace;
    wa_dtw_host_table(cost_in.data(), M, sot_len, N, trace);
    wa_dtw_backtrace(trace.data() + N + 2, 1, N + 1, N, M, path);
    if (cost_out) cost_out->swap(cost_in);
    return (int) path.size();
}

// wa_dtw.hip - the post-processing of the DTW token timestamps on the device (wa_dtw.cpp issues it; wa_dtw_host.cpp is the same arithmetic on
// the host and the yardstick): normalise over tokens, 7-wide median over audio, mean over heads, cost / trace table.  The backtrace runs on the
// host from the trace (one byte per cell), the only thing that leaves the device.
//
// The kernels read the alignment heads where the decoder pass left them, through a table of head offsets (wa_dtw_host.h: wa_dtw_view):
// x(k, t, j) = x[head_off[k] + t * tok_stride + j].  No transposed or normalised copy is made.
//
// Rounding points are the host's (ggml_norm / ggml_mean): F64 sums in index order, every F32 step rounded once (-ffp-contract=off, no fma
// written), correctly rounded F32 division and square root, F32 denormals kept (v * v can be one).  The median network is the host's 13
// exchanges with std::min / std::max written as compare-selects: fminf / fmaxf order +0 and -0, std::min / std::max do not.
//
// No kernel of this file exchanges anything with another workgroup: nothing here can wait on a workgroup that is not running.
#include "wa_kernels.h"

// ---- statistics: one thread per (head k, audio index j): mean and 1 / sqrt(variance + eps) over the tokens ----
__global__ __launch_bounds__(256) void k_dtw_stats(const float * __restrict__ x, const long long * __restrict__ head_off, long long tok_stride, int n_tokens,
                                                   int M, float * __restrict__ mean_o, float * __restrict__ scale_o) {
    const int j = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (j >= M) return;
    const float * p = x + head_off[k] + j;
    double sum = 0.0;
    for (int t = 0; t < n_tokens; ++t) sum += (double) p[(long long) t * tok_stride];
    const float mean = (float) (sum / n_tokens);
    double sum2 = 0.0;
    for (int t = 0; t < n_tokens; ++t) { const float v = p[(long long) t * tok_stride] - mean; sum2 += (double) (v * v); }
    const float variance = (float) (sum2 / n_tokens);
    const float scale = 1.0f / sqrtf(variance + 1e-9f);
    mean_o[(size_t) k * M + j] = mean;
    scale_o[(size_t) k * M + j] = scale;
}

// std::min(a, b) = (b < a) ? b : a and std::max(a, b) = (a < b) ? b : a, both from the values before the exchange
#define DTW_CX(a, b) do { const float lo_ = (b < a) ? b : a, hi_ = (a < b) ? b : a; a = lo_; b = hi_; } while (0)

// ---- median and mean: one thread per (table row i = token sot_len + i, audio index j) ----
// The result goes where the table kernel reads it: cost[(i + j) * N + i], one anti-diagonal of the table per row of N floats.
__global__ __launch_bounds__(256) void k_dtw_cost(const float * __restrict__ x, const long long * __restrict__ head_off, long long tok_stride, int n_heads,
                                                  int sot_len, int N, int M, const float * __restrict__ mean, const float * __restrict__ scale,
                                                  float * __restrict__ cost) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= M) return;
    int idx[7];
#pragma unroll
    for (int o = 0; o < 7; ++o) { const int q = j - 3 + o; idx[o] = q < 0 ? -q : (q > M - 1 ? 2 * (M - 1) - q : q); }      // reflect (M > 7)
    double sum = 0.0;
    for (int k = 0; k < n_heads; ++k) {
        const float * p = x + head_off[k] + (long long) (sot_len + i) * tok_stride;
        const float * mk = mean + (size_t) k * M, * sk = scale + (size_t) k * M;
        float v[7];
#pragma unroll
        for (int o = 0; o < 7; ++o) { const float c = p[idx[o]] - mk[idx[o]]; v[o] = c * sk[idx[o]]; }
        float p0 = v[0], p1 = v[1], p2 = v[2], p3 = v[3], p4 = v[4], p5 = v[5], p6 = v[6];
        DTW_CX(p0, p5); DTW_CX(p0, p3); DTW_CX(p1, p6); DTW_CX(p2, p4); DTW_CX(p0, p1); DTW_CX(p3, p5); DTW_CX(p2, p6);
        DTW_CX(p2, p3); DTW_CX(p3, p6); DTW_CX(p4, p5); DTW_CX(p1, p4); DTW_CX(p1, p3); DTW_CX(p3, p4);
        sum += (double) p3;
    }
    float r = (float) sum;
    r /= (float) n_heads;
    cost[(size_t) (i + j) * N + i] = r * -1.0f;
}

// ---- cost / trace table: ONE workgroup, thread i owns table row i + 1 and walks it one cell per anti-diagonal ----
// Cell (i + 1, j + 1) lies on diagonal d = i + j.  Its three neighbours: C(i + 1, j) is the thread's own previous cell, C(i, j + 1) is thread
// i - 1's cell of diagonal d - 1 (read from LDS), C(i, j) is what this thread read there one diagonal earlier.  Two LDS rows alternate: a
// diagonal reads row (d - 1) & 1 and writes row d & 1, so one barrier per diagonal orders both.  The loop's trip count is the same for every
// thread (N + M - 1 diagonals, rounded up to the prefetch ring); threads beyond row N and cells beyond a row's ends only keep the barrier.
// The costs of the next DTW_AHEAD diagonals are in flight in registers (clamped addresses, no branch around a load).
#define DTW_AHEAD 8
__global__ __launch_bounds__(WA_DTW_MAX_N) void k_dtw_table(const float * __restrict__ cost, int N, int M, uint8_t * __restrict__ trace) {
    __shared__ float diag[2][WA_DTW_MAX_N];
    const int i = threadIdx.x, ic = i < N ? i : N - 1;
    const int nd = N + M - 1;
    diag[0][i] = INFINITY; diag[1][i] = INFINITY;
    float xr[DTW_AHEAD];
#pragma unroll
    for (int u = 0; u < DTW_AHEAD; ++u) xr[u] = cost[(size_t) (u < nd ? u : nd - 1) * N + ic];
    float left = INFINITY, up_prev = INFINITY;
    __syncthreads();
    for (int d0 = 0; d0 < nd; d0 += DTW_AHEAD) {
#pragma unroll
        for (int u = 0; u < DTW_AHEAD; ++u) {
            const int d = d0 + u, j = d - i;
            const float xv = xr[u];
            { const int dn = d + DTW_AHEAD; xr[u] = cost[(size_t) (dn < nd ? dn : nd - 1) * N + ic]; }
            const float up = i > 0 ? diag[(d & 1) ^ 1][i - 1] : INFINITY;
            if (i < N && j >= 0 && j < M) {
                const float c0 = j == 0 ? (i == 0 ? 0.0f : INFINITY) : (i == 0 ? INFINITY : up_prev);
                const float c1 = up;
                const float c2 = j == 0 ? INFINITY : left;
                float c; uint8_t t;
                if (c0 < c1 && c0 < c2) { c = c0; t = 0; } else if (c1 < c0 && c1 < c2) { c = c1; t = 1; } else { c = c2; t = 2; }
                left = xv + c;
                diag[d & 1][i] = left;
                trace[(size_t) d * N + i] = t;
            }
            up_prev = up;
            __syncthreads();
        }
    }
}

void wa_launch_dtw(hipStream_t stream, const float * x, const long long * head_off, long long tok_stride, int n_heads, int n_tokens, int sot_len, int M,
                   float * mean, float * scale, float * cost, uint8_t * trace) {
    const int N = n_tokens - sot_len - 1;
    if (n_heads <= 0 || N <= 0 || N > WA_DTW_MAX_N || M <= 7) return;
    const unsigned gx = (unsigned) ((M + 255) / 256);
    hipLaunchKernelGGL(k_dtw_stats, dim3(gx, (unsigned) n_heads), dim3(256), 0, stream, x, head_off, tok_stride, n_tokens, M, mean, scale);
    hipLaunchKernelGGL(k_dtw_cost, dim3(gx, (unsigned) N), dim3(256), 0, stream, x, head_off, tok_stride, n_heads, sot_len, N, M, mean, scale, cost);
    hipLaunchKernelGGL(k_dtw_table, dim3(1), dim3((unsigned) ((N + 63) / 64 * 64)), 0, stream, cost, N, M, trace);
}

// wa_stream.hip - live streaming sessions on the device: the packet push into the 16 kHz ring and the window gather.
//
// The arithmetic is wa_audio.h's and the bookkeeping wa_stream.h's (wa_stream_ref), operation for operation: the conversions round each step
// on its own, one output sample is ONE chain of __builtin_fmaf over its K taps in ascending order from 0.0f (-ffp-contract=off).
//   k_stream_push<FMT, CH>   one packet.  Workgroup b < n_tiles makes WA_STREAM_TILE consecutive new outputs as k_audio_resample makes a tile:
//                            the frames the tile reads go to LDS as mono F32 - from the carry (the K - 1 frames before the packet), from the
//                            packet, zero in front of frame 0 (the carry starts as zeros) and behind the packet (the planner releases no
//                            output that reads there) -, the taps beside them when the table fits, then every thread runs the chains of its
//                            4 outputs and stores them at (r_w + j) mod cap.  At 16 kHz an output is the converted frame.  Workgroup
//                            n_tiles writes the next carry into the OTHER carry buffer: nothing a workgroup reads is written in the launch.
//   k_stream_window          the windows of up to 8 sessions, blockIdx.y the session: a pure copy of up to four ring pieces per session
//                            into its destination.  Threads take groups of 4 consecutive samples that start on a 16-byte boundary of the
//                            DESTINATION; a group inside one piece is one 16-byte store, fed by one 16-byte load where the source
//                            address is 16-byte aligned too and by four 4-byte loads where it is not; the groups at the window's head and
//                            tail and across a piece edge go sample by sample.
// Plain C++, vector stores, no atomics, a fixed order.
#include "wa_stream.h"

#include <hip/hip_runtime.h>

static_assert(WA_STREAM_TILE == WA_AUDIO_TILE, "k_stream_push sizes its LDS span with wa_audio_span");

template <int FMT, int CH>
static __device__ __forceinline__ float sm_frame(const void * __restrict__ data, long long i) {
    if (FMT == WA_AUDIO_I16) {
        const short * s = (const short *) data;
        if (CH == 1) return (float) s[i] / 32768.0f;
        const float sum = (float) s[2 * i] + (float) s[2 * i + 1];
        const float mid = sum / 2.0f;
        return mid / 32768.0f;
    }
    const float * f = (const float *) data;
    if (CH == 1) return f[i];
    const float sum = f[2 * i] + f[2 * i + 1];
    return sum / 2.0f;
}

// C = K - 1 carry frames (0 at 16 kHz); taps [L][K] (K a multiple of 4, rows 16-byte aligned); span = wa_audio_span
template <int FMT, int CH>
__global__ __launch_bounds__(256) void k_stream_push(const void * __restrict__ data, long long n_frames, long long T, const float * __restrict__ carry_in,
                                                     float * __restrict__ carry_out, int C, const float * __restrict__ taps, int L, int M, int K, int span,
                                                     int taps_in_lds, long long n_first, long long n_new, float * __restrict__ ring, long long cap,
                                                     long long r_w, int n_tiles) {
    __shared__ __attribute__((aligned(16))) float lds[WA_AUDIO_LDS];
    const int tid = threadIdx.x;
    if ((int) blockIdx.x == n_tiles) {              // the next carry: the last C of [carry ++ packet]
        for (int j = tid; j < C; j += 256) {
            const long long i = n_frames + j;
            carry_out[j] = i < C ? carry_in[i] : sm_frame<FMT, CH>(data, i - C);
        }
        return;
    }
    const long long j0 = (long long) blockIdx.x * WA_STREAM_TILE;      // the tile's first output, counted from n_first
    if (K == 0) {
        for (int q = 0; q < WA_STREAM_TILE / 256; ++q) {
            const long long j = j0 + q * 256 + tid;
            if (j >= n_new) break;
            ring[(r_w + j) % cap] = sm_frame<FMT, CH>(data, n_first + j - T);
        }
        return;
    }
    const long long n0 = n_first + j0;
    const long long i_first = n0 * M / L;                    // i0 of the tile's first output
    const long long start = i_first - K / 2 + 1 - (T - C);   // lds[0] holds element `start` of [carry ++ packet]
    for (int s = tid; s < span; s += 256) {
        const long long at = start + s;
        lds[s] = at < 0 ? 0.0f : at < C ? carry_in[at] : at < C + n_frames ? sm_frame<FMT, CH>(data, at - C) : 0.0f;
    }
    const int span4 = (span + 3) & ~3;
    if (taps_in_lds) {
        const float4 * src = (const float4 *) taps;
        float4 * dst = (float4 *) (lds + span4);
        for (int s = tid; s < L * K / 4; s += 256) dst[s] = src[s];
    }
    __syncthreads();
    const float * tbase = taps_in_lds ? lds + span4 : taps;
#pragma unroll 1
    for (int q = 0; q < WA_STREAM_TILE / 256; ++q) {
        const long long j = j0 + q * 256 + tid;
        if (j >= n_new) break;
        const long long t = (n_first + j) * M, i0 = t / L;
        const int p = (int) (t - i0 * L);
        const float  * x = lds + (int) (i0 - i_first);
        const float4 * h = (const float4 *) (tbase + (size_t) p * K);
        float acc = 0.0f;
#pragma unroll 4
        for (int k = 0; k < K / 4; ++k) {
            const float4 w = h[k];
            acc = __builtin_fmaf(w.x, x[4 * k + 0], acc);
            acc = __builtin_fmaf(w.y, x[4 * k + 1], acc);
            acc = __builtin_fmaf(w.z, x[4 * k + 2], acc);
            acc = __builtin_fmaf(w.w, x[4 * k + 3], acc);
        }
        ring[(r_w + j) % cap] = acc;
    }
}

__global__ __launch_bounds__(256) void k_stream_window(const wa_stream_windows tab) {
    const wa_stream_window & w = tab.w[blockIdx.y];
    const int lead = (int) (((uintptr_t) w.dst >> 2) & 3);             // floats between the last 16-byte boundary and the destination
    const long long i0 = 4 * ((long long) blockIdx.x * 256 + threadIdx.x) - lead;      // this thread's group: window samples [i0, i0 + 4)
    const long long len = w.len;
    if (i0 >= len) return;
    int p = 0;
    long long base = 0;                             // piece p holds window samples [base, base + plen[p])
    const long long first = i0 < 0 ? 0 : i0;
    while (p + 1 < w.n_pieces && first >= base + w.plen[p]) { base += w.plen[p]; ++p; }
    if (i0 >= 0 && i0 + 4 <= base + w.plen[p]) {
        const float * s = w.ring + (w.slot[p] + (i0 - base));
        float4 v;
        if (((uintptr_t) s & 15) == 0) v = *(const float4 *) s;
        else v = make_float4(s[0], s[1], s[2], s[3]);
        *(float4 *) (w.dst + i0) = v;
    } else {
        for (int k = 0; k < 4; ++k) {
            const long long at = i0 + k;
            if (at < 0 || at >= len) continue;
            while (p + 1 < w.n_pieces && at >= base + w.plen[p]) { base += w.plen[p]; ++p; }
            w.dst[at] = w.ring[w.slot[p] + (at - base)];
        }
    }
}

template <int FMT, int CH>
static bool sm_push(void * stream, const void * d_data, long long n_frames, const wa_audio_plan & p, const float * d_taps, long long T,
                    const float * d_carry_in, float * d_carry_out, long long n_first, long long n_new, float * d_ring, long long cap, long long r_w) {
    const int C = wa_stream_carry_len(p);
    int span = 0, in_lds = 0;
    if (n_first + n_new > wa_stream_final(p, T + n_frames) || (!p.K && n_first != T)) return false;     // an output whose frames have not arrived
    if (p.K) {
        span = wa_audio_span(p);
        const int span4 = (span + 3) & ~3;
        if (span4 > WA_AUDIO_LDS || !d_taps || ((uintptr_t) d_taps & 15) != 0 || p.K % 4 != 0 || !d_carry_in || !d_carry_out) return false;
        in_lds = (long long) span4 + (long long) p.L * p.K <= WA_AUDIO_LDS ? 1 : 0;
    }
    const long long tiles = (n_new + WA_STREAM_TILE - 1) / WA_STREAM_TILE, blocks = tiles + (C > 0 ? 1 : 0);
    if (blocks > 0x7fffffffLL) return false;
    if (blocks == 0) return true;
    hipLaunchKernelGGL((k_stream_push<FMT, CH>), dim3((unsigned) blocks), dim3(256), 0, (hipStream_t) stream, d_data, n_frames, T, d_carry_in, d_carry_out, C,
                       d_taps, p.L, p.M, p.K, span, in_lds, n_first, n_new, d_ring, cap, r_w, (int) tiles);
    return hipGetLastError() == hipSuccess;
}

bool wa_stream_push_launch(void * stream, const void * d_data, long long n_frames, int channels, int format, const wa_audio_plan & p, const float * d_taps,
                           long long T, const float * d_carry_in, float * d_carry_out, long long n_first, long long n_new, float * d_ring, long long cap,
                           long long r_w) {
    if (n_frames <= 0) return true;
    if (!d_data || n_new < 0 || T < 0 || n_first < 0 || r_w < 0 || (n_new > 0 && (!d_ring || cap <= 0 || n_new > cap))) return false;
    if (format == WA_AUDIO_I16) return channels == 1 ? sm_push<WA_AUDIO_I16, 1>(stream, d_data, n_frames, p, d_taps, T, d_carry_in, d_carry_out, n_first, n_new, d_ring, cap, r_w)
                                                     : sm_push<WA_AUDIO_I16, 2>(stream, d_data, n_frames, p, d_taps, T, d_carry_in, d_carry_out, n_first, n_new, d_ring, cap, r_w);
    return channels == 1 ? sm_push<WA_AUDIO_F32, 1>(stream, d_data, n_frames, p, d_taps, T, d_carry_in, d_carry_out, n_first, n_new, d_ring, cap, r_w)
                         : sm_push<WA_AUDIO_F32, 2>(stream, d_data, n_frames, p, d_taps, T, d_carry_in, d_carry_out, n_first, n_new, d_ring, cap, r_w);
}

bool wa_stream_window_launch(void * stream, const wa_stream_windows & tab, int n_sessions) {
    if (n_sessions <= 0 || n_sessions > WA_STREAM_SESSIONS) return false;
    long long groups = 0;
    for (int i = 0; i < n_sessions; ++i) {
        const wa_stream_window & w = tab.w[i];
        if (!w.ring || !w.dst || ((uintptr_t) w.dst & 3) != 0 || w.len <= 0 || w.n_pieces <= 0 || w.n_pieces > WA_STREAM_PIECES) return false;
        long long sum = 0;
        for (int p = 0; p < w.n_pieces; ++p) { if (w.slot[p] < 0 || w.plen[p] <= 0) return false; sum += w.plen[p]; }
        if (sum != w.len) return false;
        groups = std::max(groups, ((long long) w.len + (long long) (((uintptr_t) w.dst >> 2) & 3) + 3) / 4);
    }
    hipLaunchKernelGGL(k_stream_window, dim3((unsigned) ((groups + 255) / 256), (unsigned) n_sessions), dim3(256), 0, (hipStream_t) stream, tab);
    return hipGetLastError() == hipSuccess;
}

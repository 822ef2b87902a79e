// wa_audio_fmt.hip - the audio front end's kernels for the sample formats beyond int16 and F32: unsigned 8-bit, packed signed
// 24-bit, signed 32-bit and F64 PCM, G.711 mu-law and A-law - for whisper_amd_audio_to_pcm (conversion, resampling), for
// whisper_amd_audio_split (both planes in one launch) and for whisper_amd_stream_feed (the packet push into the ring).
//
// The arithmetic is wa_audio.h's: a sample becomes the value v of its table (wa_audio_value: the SAME function the host restatement runs, G.711
// expanded by integer arithmetic in registers), then v / S mono or ((vl + vr) / 2.0f) / S stereo, every operation rounded on its own; one
// output sample is ONE chain of __builtin_fmaf over its K taps in ascending order from 0.0f (-ffp-contract=off: nothing else is fused).  The
// tiles, spans, LDS budgets and chains are those of k_audio_resample, k_audio_split and k_stream_push; what differs is how a frame is read.
// Samples are read one by one, at their own width: a one- or three-byte sample starts at any byte address, a stereo S24 frame is 6 bytes and
// straddles dwords, so there is no 16-byte path here (consecutive lanes still read consecutive bytes: a wave's loads fall into one or a few
// cache lines).  S32 and F64 device input must be naturally aligned; the launchers refuse other addresses (the caller then takes the host path).
//   k_fmt_convert<FMT, CH>      16 kHz input: conversion alone
//   k_fmt_resample<FMT, CH>     k_audio_resample's tile of WA_AUDIO_TILE outputs
//   k_fmt_deinterleave<FMT>     16 kHz stereo input to two planes
//   k_fmt_split<FMT>            k_audio_split's tile of WA_CH_TILE outputs of both planes
//   k_fmt_push<FMT, CH>         k_stream_push's packet: tiles of new outputs into the ring, one more workgroup for the next carry
#include "wa_channels.h"
#include "wa_stream.h"

#include <hip/hip_runtime.h>

static_assert(WA_STREAM_TILE == WA_AUDIO_TILE, "k_fmt_push sizes its LDS span with wa_audio_span");

template <int FMT, int CH>
static __device__ __forceinline__ float fx_frame(const void * __restrict__ data, long long i) { return wa_audio_frame_fmt(data, i, CH, FMT); }
template <int FMT>
static __device__ __forceinline__ float fx_channel(const void * __restrict__ data, long long i, int c) { return wa_audio_channel_fmt(data, i, c, FMT); }

// one output: the chain over K taps (K a multiple of 4, the row 16-byte aligned) against K consecutive frames
static __device__ __forceinline__ float fx_chain(const float4 * __restrict__ h, const float * __restrict__ x, int K) {
    float acc = 0.0f;
#pragma unroll 4
    for (int k = 0; k < K / 4; ++k) {
        const float4 w = h[k];
        acc = __builtin_fmaf(w.x, x[4 * k + 0], acc);
        acc = __builtin_fmaf(w.y, x[4 * k + 1], acc);
        acc = __builtin_fmaf(w.z, x[4 * k + 2], acc);
        acc = __builtin_fmaf(w.w, x[4 * k + 3], acc);
    }
    return acc;
}

// the table into LDS behind `at` floats, where it fits; returns where the chains read it
static __device__ __forceinline__ const float * fx_taps(float * lds, int at, const float * __restrict__ taps, int L, int K, int taps_in_lds) {
    if (!taps_in_lds) return taps;
    const float4 * src = (const float4 *) taps;
    float4 * dst = (float4 *) (lds + at);
    for (int s = threadIdx.x; s < L * K / 4; s += 256) dst[s] = src[s];
    return lds + at;
}

template <int FMT, int CH>
__global__ __launch_bounds__(256) void k_fmt_convert(const void * __restrict__ data, long long n_frames, float * __restrict__ out) {
    const long long tid = (long long) blockIdx.x * 256 + threadIdx.x, stride = (long long) gridDim.x * 256;
    for (long long i = tid; i < n_frames; i += stride) out[i] = fx_frame<FMT, CH>(data, i);
}

// taps [L][K] (K a multiple of 4, rows 16-byte aligned); span = wa_audio_span; taps_in_lds: the table follows the span in LDS
template <int FMT, int CH>
__global__ __launch_bounds__(256) void k_fmt_resample(const void * __restrict__ data, long long n_frames, const float * __restrict__ taps, int L, int M,
                                                      int K, int span, int taps_in_lds, long long n_out, float * __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[WA_AUDIO_LDS];
    const int tid = threadIdx.x;
    const long long n0 = (long long) blockIdx.x * WA_AUDIO_TILE;
    const long long i_first = n0 * M / L;                    // i0 of the tile's first output
    const long long start = i_first - K / 2 + 1;             // input frame held by lds[0]
    for (int s = tid; s < span; s += 256) {
        const long long i = start + s;
        lds[s] = i >= 0 && i < n_frames ? fx_frame<FMT, CH>(data, i) : 0.0f;
    }
    const float * tbase = fx_taps(lds, (span + 3) & ~3, taps, L, K, taps_in_lds);
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < WA_AUDIO_TILE / 256; ++q) {
        const long long n = n0 + q * 256 + tid;
        if (n >= n_out) break;
        const long long t = n * M, i0 = t / L;
        const int p = (int) (t - i0 * L);
        out[n] = fx_chain((const float4 *) (tbase + (size_t) p * K), lds + (int) (i0 - i_first), K);
    }
}

// plane c at out + c * stride
template <int FMT>
__global__ __launch_bounds__(256) void k_fmt_deinterleave(const void * __restrict__ data, long long n_frames, long long stride, float * __restrict__ out) {
    const long long tid = (long long) blockIdx.x * 256 + threadIdx.x, step = (long long) gridDim.x * 256;
    for (long long i = tid; i < n_frames; i += step) {
        out[i] = fx_channel<FMT>(data, i, 0);
        out[stride + i] = fx_channel<FMT>(data, i, 1);
    }
}

// span = wa_ch_span; taps_in_lds: the table follows the two planes in LDS
template <int FMT>
__global__ __launch_bounds__(256) void k_fmt_split(const void * __restrict__ data, long long n_frames, const float * __restrict__ taps, int L, int M, int K,
                                                   int span, int taps_in_lds, long long n_out, long long stride, float * __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[WA_CH_LDS];
    const int tid = threadIdx.x;
    const int span4 = (span + 3) & ~3;
    const long long n0 = (long long) blockIdx.x * WA_CH_TILE;
    const long long i_first = n0 * M / L;                      // i0 of the tile's first output
    const long long start = i_first - K / 2 + 1;               // input frame held by lds[0] and lds[span4]
    for (int s = tid; s < span; s += 256) {
        const long long i = start + s;
        const bool in = i >= 0 && i < n_frames;
        lds[s] = in ? fx_channel<FMT>(data, i, 0) : 0.0f;
        lds[span4 + s] = in ? fx_channel<FMT>(data, i, 1) : 0.0f;
    }
    const float * tbase = fx_taps(lds, 2 * span4, taps, L, K, taps_in_lds);
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < WA_CH_TILE / 256; ++q) {
        const long long n = n0 + q * 256 + tid;
        if (n >= n_out) break;
        const long long t = n * M, i0 = t / L;
        const int p = (int) (t - i0 * L);
        const float  * x = lds + (int) (i0 - i_first);
        const float4 * h = (const float4 *) (tbase + (size_t) p * K);
        out[n] = fx_chain(h, x, K);
        out[stride + n] = fx_chain(h, x + span4, K);
    }
}

// C = K - 1 carry frames (0 at 16 kHz); span = wa_audio_span; the arguments are k_stream_push's
template <int FMT, int CH>
__global__ __launch_bounds__(256) void k_fmt_push(const void * __restrict__ data, long long n_frames, long long T, const float * __restrict__ carry_in,
                                                  float * __restrict__ carry_out, int C, const float * __restrict__ taps, int L, int M, int K, int span,
                                                  int taps_in_lds, long long n_first, long long n_new, float * __restrict__ ring, long long cap, long long r_w,
                                                  int n_tiles) {
    __shared__ __attribute__((aligned(16))) float lds[WA_AUDIO_LDS];
    const int tid = threadIdx.x;
    if ((int) blockIdx.x == n_tiles) {              // the next carry: the last C of [carry ++ packet]
        for (int j = tid; j < C; j += 256) {
            const long long i = n_frames + j;
            carry_out[j] = i < C ? carry_in[i] : fx_frame<FMT, CH>(data, i - C);
        }
        return;
    }
    const long long j0 = (long long) blockIdx.x * WA_STREAM_TILE;      // the tile's first output, counted from n_first
    if (K == 0) {
        for (int q = 0; q < WA_STREAM_TILE / 256; ++q) {
            const long long j = j0 + q * 256 + tid;
            if (j >= n_new) break;
            ring[(r_w + j) % cap] = fx_frame<FMT, CH>(data, n_first + j - T);
        }
        return;
    }
    const long long n0 = n_first + j0;
    const long long i_first = n0 * M / L;                    // i0 of the tile's first output
    const long long start = i_first - K / 2 + 1 - (T - C);   // lds[0] holds element `start` of [carry ++ packet]
    for (int s = tid; s < span; s += 256) {
        const long long at = start + s;
        lds[s] = at < 0 ? 0.0f : at < C ? carry_in[at] : at < C + n_frames ? fx_frame<FMT, CH>(data, at - C) : 0.0f;
    }
    const float * tbase = fx_taps(lds, (span + 3) & ~3, taps, L, K, taps_in_lds);
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < WA_STREAM_TILE / 256; ++q) {
        const long long j = j0 + q * 256 + tid;
        if (j >= n_new) break;
        const long long t = (n_first + j) * M, i0 = t / L;
        const int p = (int) (t - i0 * L);
        ring[(r_w + j) % cap] = fx_chain((const float4 *) (tbase + (size_t) p * K), lds + (int) (i0 - i_first), K);
    }
}

// S32 and F64 are read with aligned loads
static bool fx_aligned(const void * d_data, int format) {
    const uintptr_t a = (uintptr_t) d_data;
    return format == WA_AUDIO_S32 ? (a & 3) == 0 : format == WA_AUDIO_F64 ? (a & 7) == 0 : true;
}

// `CALL(F)` with F the compile-time format of `format`; false for a code that is none of these
#define FX_BY_FORMAT(format, CALL)                      \
    switch (format) {                                   \
        case WA_AUDIO_U8:   return CALL(WA_AUDIO_U8);   \
        case WA_AUDIO_S24:  return CALL(WA_AUDIO_S24);  \
        case WA_AUDIO_S32:  return CALL(WA_AUDIO_S32);  \
        case WA_AUDIO_F64:  return CALL(WA_AUDIO_F64);  \
        case WA_AUDIO_ULAW: return CALL(WA_AUDIO_ULAW); \
        case WA_AUDIO_ALAW: return CALL(WA_AUDIO_ALAW); \
        default:            return false;               \
    }

template <int FMT, int CH>
static bool fx_launch(void * stream, const void * d_data, long long n_frames, const wa_audio_plan & p, const float * d_taps, long long n_out, float * d_out) {
    hipStream_t s = (hipStream_t) stream;
    if (!p.K) {
        long long blocks = (n_frames + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL((k_fmt_convert<FMT, CH>), dim3((unsigned) blocks), dim3(256), 0, s, d_data, n_frames, d_out);
    } else {
        const int span = wa_audio_span(p), span4 = (span + 3) & ~3;
        if (span4 > WA_AUDIO_LDS || !d_taps || ((uintptr_t) d_taps & 15) != 0 || p.K % 4 != 0) return false;
        const int in_lds = (long long) span4 + (long long) p.L * p.K <= WA_AUDIO_LDS ? 1 : 0;
        const long long blocks = (n_out + WA_AUDIO_TILE - 1) / WA_AUDIO_TILE;
        if (blocks > 0x7fffffffLL) return false;
        hipLaunchKernelGGL((k_fmt_resample<FMT, CH>), dim3((unsigned) blocks), dim3(256), 0, s, d_data, n_frames, d_taps, p.L, p.M, p.K, span, in_lds,
                           n_out, d_out);
    }
    return hipGetLastError() == hipSuccess;
}

// d_out[0 .. n_out) from d_data (device pointers), on `stream`, as wa_audio_launch.  false: a launch failed or the shape, format or alignment
// is not served (nothing was launched); the other arguments are the caller's to check (wa_audio_args_ok).
bool wa_audio_fmt_launch(void * stream, const void * d_data, long long n_frames, int channels, int format, const wa_audio_plan & p, const float * d_taps,
                         long long n_out, float * d_out) {
    if (n_out <= 0) return true;
    if (!d_data || !d_out || n_frames <= 0 || (channels != 1 && channels != 2) || !fx_aligned(d_data, format)) return false;
#define FX_CALL(F) (channels == 1 ? fx_launch<F, 1>(stream, d_data, n_frames, p, d_taps, n_out, d_out) : fx_launch<F, 2>(stream, d_data, n_frames, p, d_taps, n_out, d_out))
    FX_BY_FORMAT(format, FX_CALL)
#undef FX_CALL
}

template <int FMT>
static bool fx_split(void * stream, const void * d_data, long long n_frames, const wa_audio_plan & p, const float * d_taps, long long n_out, long long stride,
                     float * d_out) {
    hipStream_t s = (hipStream_t) stream;
    if (!p.K) {
        long long blocks = (n_frames + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL((k_fmt_deinterleave<FMT>), dim3((unsigned) blocks), dim3(256), 0, s, d_data, n_frames, stride, d_out);
    } else {
        const int span = wa_ch_span(p), span4 = (span + 3) & ~3;
        if (2 * span4 > WA_CH_LDS || !d_taps || ((uintptr_t) d_taps & 15) != 0 || p.K % 4 != 0) return false;
        const int in_lds = 2LL * span4 + (long long) p.L * p.K <= WA_CH_LDS ? 1 : 0;
        const long long blocks = (n_out + WA_CH_TILE - 1) / WA_CH_TILE;
        if (blocks > 0x7fffffffLL) return false;
        hipLaunchKernelGGL((k_fmt_split<FMT>), dim3((unsigned) blocks), dim3(256), 0, s, d_data, n_frames, d_taps, p.L, p.M, p.K, span, in_lds, n_out, stride,
                           d_out);
    }
    return hipGetLastError() == hipSuccess;
}

bool wa_ch_split_fmt_launch(void * stream, const void * d_data, long long n_frames, int format, const wa_audio_plan & p, const float * d_taps, long long n_out,
                            long long stride, float * d_out) {
    if (n_out <= 0) return true;
    if (!d_data || !d_out || n_frames <= 0 || stride < n_out || !fx_aligned(d_data, format)) return false;
#define FX_CALL(F) fx_split<F>(stream, d_data, n_frames, p, d_taps, n_out, stride, d_out)
    FX_BY_FORMAT(format, FX_CALL)
#undef FX_CALL
}

template <int FMT, int CH>
static bool fx_push(void * stream, const void * d_data, long long n_frames, const wa_audio_plan & p, const float * d_taps, long long T, const float * d_carry_in,
                    float * d_carry_out, long long n_first, long long n_new, float * d_ring, long long cap, long long r_w) {
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
    hipLaunchKernelGGL((k_fmt_push<FMT, CH>), dim3((unsigned) blocks), dim3(256), 0, (hipStream_t) stream, d_data, n_frames, T, d_carry_in, d_carry_out, C,
                       d_taps, p.L, p.M, p.K, span, in_lds, n_first, n_new, d_ring, cap, r_w, (int) tiles);
    return hipGetLastError() == hipSuccess;
}

bool wa_stream_push_fmt_launch(void * stream, const void * d_data, long long n_frames, int channels, int format, const wa_audio_plan & p, const float * d_taps,
                               long long T, const float * d_carry_in, float * d_carry_out, long long n_first, long long n_new, float * d_ring, long long cap,
                               long long r_w) {
    if (n_frames <= 0) return true;
    if (!d_data || n_new < 0 || T < 0 || n_first < 0 || r_w < 0 || (n_new > 0 && (!d_ring || cap <= 0 || n_new > cap))) return false;
    if ((channels != 1 && channels != 2) || !fx_aligned(d_data, format)) return false;
#define FX_CALL(F) (channels == 1 ? fx_push<F, 1>(stream, d_data, n_frames, p, d_taps, T, d_carry_in, d_carry_out, n_first, n_new, d_ring, cap, r_w) \
                                  : fx_push<F, 2>(stream, d_data, n_frames, p, d_taps, T, d_carry_in, d_carry_out, n_first, n_new, d_ring, cap, r_w))
    FX_BY_FORMAT(format, FX_CALL)
#undef FX_CALL
}

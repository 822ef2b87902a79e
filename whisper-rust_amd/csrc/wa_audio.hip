// wa_audio.hip - audio front end on the device: int16 / F32, mono / stereo, 8 .. 192 kHz -> 16 kHz mono F32.
//
// The arithmetic is wa_audio.h's (wa_audio_ref), operation for operation: the conversions round each step on its own, one output sample
// is ONE chain of __builtin_fmaf over its K taps in ascending order from 0.0f (-ffp-contract=off: nothing else is fused).
//   k_audio_convert<FMT, CH>   16 kHz input: conversion alone, 16-byte loads and stores; frames past the last whole vector, and every
//                              frame of an input whose base is not 16-byte aligned, go through the scalar tail.
//   k_audio_resample<FMT, CH>  256 threads make WA_AUDIO_TILE consecutive outputs: the input span the tile reads is converted to mono F32
//                              into LDS (zero outside the input), the taps beside it when the table fits (else they are read from global
//                              memory, 160 KB at most: it stays in L2), then every thread runs the chains of its 4 outputs.
#include "wa_audio.h"

#include <hip/hip_runtime.h>

template <int FMT, int CH>
static __device__ __forceinline__ float au_frame(const void * __restrict__ data, long long i) {
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

static __device__ __forceinline__ float au_lo(unsigned w) { return (float) (short) (w & 0xffffu); }
static __device__ __forceinline__ float au_hi(unsigned w) { return (float) (short) (w >> 16); }
static __device__ __forceinline__ float au_i16_stereo(unsigned w) {
    const float sum = au_lo(w) + au_hi(w);
    const float mid = sum / 2.0f;
    return mid / 32768.0f;
}

// n_vec vectors of V frames (V = 8 for int16 mono, else 4) through 16-byte accesses, frames [n_vec V, n_frames) one by one
template <int FMT, int CH>
__global__ __launch_bounds__(256) void k_audio_convert(const void * __restrict__ data, long long n_frames, long long n_vec, float * __restrict__ out) {
    constexpr int V = (FMT == WA_AUDIO_I16 && CH == 1) ? 8 : 4;
    const long long tid = (long long) blockIdx.x * 256 + threadIdx.x, stride = (long long) gridDim.x * 256;
    for (long long v = tid; v < n_vec; v += stride) {
        float4 * o = (float4 *) out + v * (V / 4);
        if (FMT == WA_AUDIO_I16 && CH == 1) {
            const uint4 w = ((const uint4 *) data)[v];
            o[0] = make_float4(au_lo(w.x) / 32768.0f, au_hi(w.x) / 32768.0f, au_lo(w.y) / 32768.0f, au_hi(w.y) / 32768.0f);
            o[1] = make_float4(au_lo(w.z) / 32768.0f, au_hi(w.z) / 32768.0f, au_lo(w.w) / 32768.0f, au_hi(w.w) / 32768.0f);
        } else if (FMT == WA_AUDIO_I16) {
            const uint4 w = ((const uint4 *) data)[v];
            o[0] = make_float4(au_i16_stereo(w.x), au_i16_stereo(w.y), au_i16_stereo(w.z), au_i16_stereo(w.w));
        } else if (CH == 1) {
            o[0] = ((const float4 *) data)[v];
        } else {
            const float4 a = ((const float4 *) data)[2 * v], b = ((const float4 *) data)[2 * v + 1];
            const float s0 = a.x + a.y, s1 = a.z + a.w, s2 = b.x + b.y, s3 = b.z + b.w;
            o[0] = make_float4(s0 / 2.0f, s1 / 2.0f, s2 / 2.0f, s3 / 2.0f);
        }
    }
    for (long long i = n_vec * V + tid; i < n_frames; i += stride) out[i] = au_frame<FMT, CH>(data, i);
}

// taps [L][K] (K a multiple of 64, rows 16-byte aligned); span = wa_audio_span; taps_in_lds: the table follows the span in LDS
template <int FMT, int CH>
__global__ __launch_bounds__(256) void k_audio_resample(const void * __restrict__ data, long long n_frames, const float * __restrict__ taps, int L, int M,
                                                        int K, int span, int taps_in_lds, long long n_out, float * __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[WA_AUDIO_LDS];
    const int tid = threadIdx.x;
    const long long n0 = (long long) blockIdx.x * WA_AUDIO_TILE;
    const long long i_first = n0 * M / L;                    // i0 of the tile's first output
    const long long start = i_first - K / 2 + 1;             // input frame held by lds[0]
    for (int s = tid; s < span; s += 256) {
        const long long i = start + s;
        lds[s] = i >= 0 && i < n_frames ? au_frame<FMT, CH>(data, i) : 0.0f;
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
    for (int q = 0; q < WA_AUDIO_TILE / 256; ++q) {
        const long long n = n0 + q * 256 + tid;
        if (n >= n_out) break;
        const long long t = n * M, i0 = t / L;
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
        out[n] = acc;
    }
}

template <int FMT, int CH>
static bool au_launch(void * stream, const void * d_data, long long n_frames, const wa_audio_plan & p, const float * d_taps, long long n_out, float * d_out) {
    hipStream_t s = (hipStream_t) stream;
    if (!p.K) {
        constexpr int V = (FMT == WA_AUDIO_I16 && CH == 1) ? 8 : 4;
        const long long n_vec = ((uintptr_t) d_data & 15) == 0 && ((uintptr_t) d_out & 15) == 0 ? n_frames / V : 0;
        const long long work = n_vec > n_frames - n_vec * V ? n_vec : n_frames - n_vec * V;
        long long blocks = (work + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL((k_audio_convert<FMT, CH>), dim3((unsigned) blocks), dim3(256), 0, s, d_data, n_frames, n_vec, d_out);
    } else {
        const int span = wa_audio_span(p), span4 = (span + 3) & ~3;
        if (span4 > WA_AUDIO_LDS || !d_taps || ((uintptr_t) d_taps & 15) != 0 || p.K % 4 != 0) return false;
        const int in_lds = (long long) span4 + (long long) p.L * p.K <= WA_AUDIO_LDS ? 1 : 0;
        const long long blocks = (n_out + WA_AUDIO_TILE - 1) / WA_AUDIO_TILE;
        if (blocks > 0x7fffffffLL) return false;
        hipLaunchKernelGGL((k_audio_resample<FMT, CH>), dim3((unsigned) blocks), dim3(256), 0, s, d_data, n_frames, d_taps, p.L, p.M, p.K, span, in_lds,
                           n_out, d_out);
    }
    return hipGetLastError() == hipSuccess;
}

// d_out[0 .. n_out) from d_data (device pointers; d_taps: the device copy of wa_audio_taps' table, unused at 16 kHz), on `stream`.
// false: a launch failed or the shape is not served (nothing was launched); the arguments are the caller's to check (wa_audio_args_ok).
bool wa_audio_launch(void * stream, const void * d_data, long long n_frames, int channels, int format, const wa_audio_plan & p, const float * d_taps,
                     long long n_out, float * d_out) {
    if (n_out <= 0) return true;
    if (format == WA_AUDIO_I16) return channels == 1 ? au_launch<WA_AUDIO_I16, 1>(stream, d_data, n_frames, p, d_taps, n_out, d_out)
                                                     : au_launch<WA_AUDIO_I16, 2>(stream, d_data, n_frames, p, d_taps, n_out, d_out);
    return channels == 1 ? au_launch<WA_AUDIO_F32, 1>(stream, d_data, n_frames, p, d_taps, n_out, d_out)
                         : au_launch<WA_AUDIO_F32, 2>(stream, d_data, n_frames, p, d_taps, n_out, d_out);
}

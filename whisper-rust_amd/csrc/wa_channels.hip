// wa_channels.hip - two-channel recordings on the device: both channels of an interleaved stereo recording as two planes of
// 16 kHz F32 in ONE launch, and the energy of spans of both planes in ONE launch.
//
// The arithmetic is wa_channels.h's (wa_ch_split_ref, wa_ch_energy_ref), operation for operation; -ffp-contract=off: a chain is the
// __builtin_fmaf calls written here, nothing else is fused.
//   k_audio_deinterleave<FMT>  16 kHz input: conversion alone.  One 16-byte load brings 4 int16 frames (two bring 4 F32 frames) of both
//                              channels, one 16-byte store goes to each plane; frames past the last whole vector, and every frame of an
//                              input whose base is not 16-byte aligned, go through the scalar tail.
//   k_audio_split<FMT>         256 threads make WA_CH_TILE consecutive outputs of BOTH planes.  The interleaved input span of the tile is
//                              read once - 16-byte loads where a whole vector lies inside the input and the base is aligned - and converted
//                              into two LDS planes (zero outside the input); the taps follow them in LDS where they fit (else they are read
//                              from global memory, where the table stays in L2).  A thread then runs the two chains of an output index
//                              against ONE read of each tap.
//   k_channel_energy           one workgroup per (span, channel): thread l is lane l of the stated order, the tree runs in LDS.  No atomics.
#include "wa_channels.h"

#include <hip/hip_runtime.h>

static __device__ __forceinline__ float ch_lo(unsigned w) { return (float) (short) (w & 0xffffu); }
static __device__ __forceinline__ float ch_hi(unsigned w) { return (float) (short) (w >> 16); }

template <int FMT>
static __device__ __forceinline__ float ch_frame(const void * __restrict__ data, long long i, int c) {
    if (FMT == WA_AUDIO_I16) return (float) ((const short *) data)[2 * i + c] / 32768.0f;
    return ((const float *) data)[2 * i + c];
}

// n_vec vectors of 4 frames through 16-byte accesses, frames [4 n_vec, n_frames) one by one; plane c at out + c * stride
template <int FMT>
__global__ __launch_bounds__(256) void k_audio_deinterleave(const void * __restrict__ data, long long n_frames, long long n_vec, long long stride,
                                                            float * __restrict__ out) {
    const long long tid = (long long) blockIdx.x * 256 + threadIdx.x, step = (long long) gridDim.x * 256;
    for (long long v = tid; v < n_vec; v += step) {
        float4 a, b;
        if (FMT == WA_AUDIO_I16) {
            const uint4 w = ((const uint4 *) data)[v];
            a = make_float4(ch_lo(w.x) / 32768.0f, ch_lo(w.y) / 32768.0f, ch_lo(w.z) / 32768.0f, ch_lo(w.w) / 32768.0f);
            b = make_float4(ch_hi(w.x) / 32768.0f, ch_hi(w.y) / 32768.0f, ch_hi(w.z) / 32768.0f, ch_hi(w.w) / 32768.0f);
        } else {
            const float4 p = ((const float4 *) data)[2 * v], q = ((const float4 *) data)[2 * v + 1];
            a = make_float4(p.x, p.z, q.x, q.z);
            b = make_float4(p.y, p.w, q.y, q.w);
        }
        *(float4 *) (out + 4 * v) = a;
        *(float4 *) (out + stride + 4 * v) = b;
    }
    for (long long i = n_vec * 4 + tid; i < n_frames; i += step) {
        out[i] = ch_frame<FMT>(data, i, 0);
        out[stride + i] = ch_frame<FMT>(data, i, 1);
    }
}

// taps [L][K] (K a multiple of 4, rows 16-byte aligned); span = wa_ch_span; taps_in_lds: the table follows the two planes in LDS;
// vec_ok: the input's base is 16-byte aligned
template <int FMT>
__global__ __launch_bounds__(256) void k_audio_split(const void * __restrict__ data, long long n_frames, const float * __restrict__ taps, int L, int M, int K,
                                                     int span, int taps_in_lds, int vec_ok, long long n_out, long long stride, float * __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[WA_CH_LDS];
    constexpr int V = FMT == WA_AUDIO_I16 ? 4 : 2;             // frames of both channels in 16 bytes
    const int tid = threadIdx.x;
    const int span4 = (span + 3) & ~3;
    const long long n0 = (long long) blockIdx.x * WA_CH_TILE;
    const long long i_first = n0 * M / L;                      // i0 of the tile's first output
    const long long start = i_first - K / 2 + 1;               // input frame held by lds[0] and lds[span4]
    const long long g0 = (start >= 0 ? start / V : -((-start + V - 1) / V)) * V;      // start rounded down to a whole vector
    const int n_vec = (int) ((start + span - g0 + V - 1) / V);
    for (int v = tid; v < n_vec; v += 256) {
        const long long i = g0 + (long long) v * V;            // frames i .. i + V - 1 go to lds[i - start ..]
        float x0[V], x1[V];
        if (vec_ok && i >= 0 && i + V <= n_frames) {
            if (FMT == WA_AUDIO_I16) {
                const uint4 w = *(const uint4 *) ((const short *) data + 2 * i);
                x0[0] = ch_lo(w.x) / 32768.0f; x1[0] = ch_hi(w.x) / 32768.0f;
                x0[1] = ch_lo(w.y) / 32768.0f; x1[1] = ch_hi(w.y) / 32768.0f;
                x0[V - 2] = ch_lo(w.z) / 32768.0f; x1[V - 2] = ch_hi(w.z) / 32768.0f;
                x0[V - 1] = ch_lo(w.w) / 32768.0f; x1[V - 1] = ch_hi(w.w) / 32768.0f;
            } else {
                const float4 w = *(const float4 *) ((const float *) data + 2 * i);
                x0[0] = w.x; x1[0] = w.y; x0[V - 1] = w.z; x1[V - 1] = w.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool in = i + j >= 0 && i + j < n_frames;
                x0[j] = in ? ch_frame<FMT>(data, i + j, 0) : 0.0f;
                x1[j] = in ? ch_frame<FMT>(data, i + j, 1) : 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const long long s = i + j - start;
            if (s >= 0 && s < span) { lds[s] = x0[j]; lds[span4 + s] = x1[j]; }
        }
    }
    if (taps_in_lds) {
        const float4 * src = (const float4 *) taps;
        float4 * dst = (float4 *) (lds + 2 * span4);
        for (int s = tid; s < L * K / 4; s += 256) dst[s] = src[s];
    }
    __syncthreads();
    const float * tbase = taps_in_lds ? lds + 2 * span4 : taps;
#pragma unroll 1
    for (int q = 0; q < WA_CH_TILE / 256; ++q) {
        const long long n = n0 + q * 256 + tid;
        if (n >= n_out) break;
        const long long t = n * M, i0 = t / L;
        const int p = (int) (t - i0 * L);
        const float  * x = lds + (int) (i0 - i_first), * y = x + span4;
        const float4 * h = (const float4 *) (tbase + (size_t) p * K);
        float acc0 = 0.0f, acc1 = 0.0f;
#pragma unroll 4
        for (int k = 0; k < K / 4; ++k) {
            const float4 w = h[k];
            acc0 = __builtin_fmaf(w.x, x[4 * k + 0], acc0); acc1 = __builtin_fmaf(w.x, y[4 * k + 0], acc1);
            acc0 = __builtin_fmaf(w.y, x[4 * k + 1], acc0); acc1 = __builtin_fmaf(w.y, y[4 * k + 1], acc1);
            acc0 = __builtin_fmaf(w.z, x[4 * k + 2], acc0); acc1 = __builtin_fmaf(w.z, y[4 * k + 2], acc1);
            acc0 = __builtin_fmaf(w.w, x[4 * k + 3], acc0); acc1 = __builtin_fmaf(w.w, y[4 * k + 3], acc1);
        }
        out[n] = acc0;
        out[stride + n] = acc1;
    }
}

// block (i, c): E_c of span i.  Thread l sums the samples of its lane in ascending order; the tree is wa_ch_energy_ref's.
__global__ __launch_bounds__(WA_CH_LANES) void k_channel_energy(const float * __restrict__ planes, long long n, long long stride,
                                                                const long long * __restrict__ spans, double * __restrict__ energy) {
    __shared__ double v[WA_CH_LANES];
    const int l = threadIdx.x, c = blockIdx.y;
    long long a = spans[2 * (long long) blockIdx.x], b = spans[2 * (long long) blockIdx.x + 1];
    if (a < 0) a = 0;
    if (b > n) b = n;
    const float * x = planes + c * stride;
    double s = 0.0;
    if (a < b)
        for (long long j = a + ((l - (int) (a % WA_CH_LANES)) + WA_CH_LANES) % WA_CH_LANES; j < b; j += WA_CH_LANES) s += (double) __builtin_fabsf(x[j]);
    v[l] = s;
    __syncthreads();
    for (int w = WA_CH_LANES / 2; w >= 1; w >>= 1) {
        if (l < w) v[l] += v[l + w];
        __syncthreads();
    }
    if (l == 0) energy[2 * (long long) blockIdx.x + c] = v[0];
}

template <int FMT>
static bool ch_launch(void * stream, const void * d_data, long long n_frames, const wa_audio_plan & p, const float * d_taps, long long n_out, long long stride,
                      float * d_out) {
    hipStream_t s = (hipStream_t) stream;
    const bool aligned = ((uintptr_t) d_data & 15) == 0;
    if (!p.K) {
        const long long n_vec = aligned ? n_frames / 4 : 0;
        const long long work = n_vec > n_frames - n_vec * 4 ? n_vec : n_frames - n_vec * 4;
        long long blocks = (work + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL((k_audio_deinterleave<FMT>), dim3((unsigned) blocks), dim3(256), 0, s, d_data, n_frames, n_vec, stride, d_out);
    } else {
        const int span = wa_ch_span(p), span4 = (span + 3) & ~3;
        if (2 * span4 > WA_CH_LDS || !d_taps || ((uintptr_t) d_taps & 15) != 0 || p.K % 4 != 0) return false;
        const int in_lds = 2LL * span4 + (long long) p.L * p.K <= WA_CH_LDS ? 1 : 0;
        const long long blocks = (n_out + WA_CH_TILE - 1) / WA_CH_TILE;
        if (blocks > 0x7fffffffLL) return false;
        hipLaunchKernelGGL((k_audio_split<FMT>), dim3((unsigned) blocks), dim3(256), 0, s, d_data, n_frames, d_taps, p.L, p.M, p.K, span, in_lds,
                           aligned ? 1 : 0, n_out, stride, d_out);
    }
    return hipGetLastError() == hipSuccess;
}

bool wa_ch_split_launch(void * stream, const void * d_data, long long n_frames, int format, const wa_audio_plan & p, const float * d_taps, long long n_out,
                        long long stride, float * d_out) {
    if (n_out <= 0) return true;
    if (!d_data || !d_out || ((uintptr_t) d_out & 15) != 0 || stride < n_out || stride % 4 != 0) return false;
    return format == WA_AUDIO_I16 ? ch_launch<WA_AUDIO_I16>(stream, d_data, n_frames, p, d_taps, n_out, stride, d_out)
                                  : ch_launch<WA_AUDIO_F32>(stream, d_data, n_frames, p, d_taps, n_out, stride, d_out);
}

bool wa_ch_energy_launch(void * stream, const float * d_planes, long long n, long long stride, const long long * d_spans, int n_spans, double * d_energy) {
    if (n_spans <= 0) return true;
    if (!d_planes || !d_spans || !d_energy || n < 0 || stride < n) return false;
    hipLaunchKernelGGL(k_channel_energy, dim3((unsigned) n_spans, 2), dim3(WA_CH_LANES), 0, (hipStream_t) stream, d_planes, n, stride, d_spans, d_energy);
    return hipGetLastError() == hipSuccess;
}

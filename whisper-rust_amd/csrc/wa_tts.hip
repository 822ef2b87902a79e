// wa_tts.hip - heuristic token timestamps on the device: the windowed |PCM| energy of a call's audio and the boundary
// scans of a finished segment's text tokens, on the state's stream (wa_tts.cpp issues them).
//
// The arithmetic is wa_tts.h's (wa_signal_energy, wa_tts_record_host), operation for operation: F32 additions in ascending index order,
// nothing fused (-ffp-contract=off, and there is no product to fuse with), F32 subnormals kept, the divisions correctly rounded.
//   k_tts_energy   256 threads own WA_TTS_TILE consecutive outputs.  The tile's TILE + 64 samples are read once, coalesced, and staged in
//                  LDS as |x|, +0.0f where the 32-sample halo leaves the recording.  Every output then runs the full 65-term chain out of
//                  LDS: thread t owns outputs t, t + 256, t + 512, t + 768 (four independent chains in flight), so the lanes of a wave
//                  read consecutive words in every step and no bank is hit twice.  The zeros make the clipped windows exact: the staged
//                  values are >= +0.0f or NaN, so a chain never holds -0.0f, and 0.0f + 0.0f in front of the window's first sample or
//                  acc + 0.0f behind its last one leaves the chain's value as it is - the clipped chain of wa_signal_energy bit for bit.
//   k_tts_snap     one wave per text token.  The total of the token's window is ONE F32 chain, so it cannot be reduced as a tree: the wave
//                  loads 64 energies per step, coalesced, one per lane - the next step's load is issued before this step's chain - and
//                  every lane carries the same chain over v_readlane of lane 0 .. 63 (uniform, no LDS round trip).  The four scans have
//                  independent comparisons and are wave-wide: 64 energies per step, a ballot of "the scan stops here", its first set bit.
//                  Every index a lane reads is inside [0, n).
#include "wa_tts.h"

#include <hip/hip_runtime.h>

#define TTS_SPAN (WA_TTS_TILE + 2 * WA_TTS_HALF)

__global__ __launch_bounds__(256) void k_tts_energy(const float * __restrict__ x, int n, float * __restrict__ e) {
    __shared__ float a[TTS_SPAN];
    const int tid = threadIdx.x;
    const long long i0 = (long long) blockIdx.x * WA_TTS_TILE;
    for (int s = tid; s < TTS_SPAN; s += 256) {
        const long long g = i0 - WA_TTS_HALF + s;
        a[s] = g >= 0 && g < n ? __builtin_fabsf(x[g]) : 0.0f;
    }
    __syncthreads();
    float acc[WA_TTS_TILE / 256];
#pragma unroll
    for (int q = 0; q < WA_TTS_TILE / 256; ++q) acc[q] = 0.0f;
#pragma unroll
    for (int k = 0; k <= 2 * WA_TTS_HALF; ++k) {
#pragma unroll
        for (int q = 0; q < WA_TTS_TILE / 256; ++q) acc[q] += a[q * 256 + tid + k];
    }
#pragma unroll
    for (int q = 0; q < WA_TTS_TILE / 256; ++q) {
        const long long i = i0 + q * 256 + tid;
        if (i < n) e[i] = acc[q] / (float) (2 * WA_TTS_HALF + 1);
    }
}

template <bool LOUD> static __device__ __forceinline__ bool tts_holds(float x, float level) { return LOUD ? x > level : x < level; }

// k = from; while (k < end && holds(k)) ++k;  from <= n - 1, end <= n
template <bool LOUD> static __device__ __forceinline__ int tts_scan_up(const float * __restrict__ e, int from, int end, float level, int lane) {
    for (int base = from; base < end; base += 64) {
        const int k = base + lane;
        const bool stop = k < end && !tts_holds<LOUD>(e[k < end ? k : from], level);
        const unsigned long long m = __ballot(stop);
        if (m) return base + __builtin_ctzll(m);
    }
    return end > from ? end : from;
}

// k = from; while (k > 0 && holds(k)) --k;  0 <= from <= n - 1
template <bool LOUD> static __device__ __forceinline__ int tts_scan_down(const float * __restrict__ e, int from, float level, int lane) {
    for (int base = from; base >= 1; base -= 64) {
        const int k = base - lane;
        const bool stop = k >= 1 && !tts_holds<LOUD>(e[k >= 1 ? k : from], level);
        const unsigned long long m = __ballot(stop);
        if (m) return base - __builtin_ctzll(m);
    }
    return 0;
}

__global__ __launch_bounds__(64) void k_tts_snap(const float * __restrict__ e, int n, const int32_t * __restrict__ tok, int n_tokens,
                                                 wa_tts_record * __restrict__ rec) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int s_lo = tok[j], s_hi = tok[n_tokens + j], has_prev = tok[2 * n_tokens + j];
    const int w_lo = s_lo - WA_TTS_REACH > 0 ? s_lo - WA_TTS_REACH : 0, w_hi = s_hi + WA_TTS_REACH < n ? s_hi + WA_TTS_REACH : n;

    float total = 0.0f;
    float v = lane < w_hi - w_lo ? e[w_lo + lane] : 0.0f;
    for (int base = w_lo; base < w_hi; base += 64) {
        const int left = w_hi - base;                       // energies of this step and behind it
        const float next = lane < left - 64 ? e[base + 64 + lane] : 0.0f;
        if (left >= 64) {
#pragma unroll
            for (int t = 0; t < 64; ++t) total += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t));
        } else {
            for (int t = 0; t < left; ++t) total += __shfl(v, t);
        }
        v = next;
    }
    const float level = (float) (0.5 * (double) total / (double) (w_hi - w_lo));

    const float e_lo = e[s_lo], e_hi = e[s_hi];
    const int back_lo = has_prev ? tts_scan_down<true>(e, s_lo, level, lane) : s_lo;
    const int fwd_lo  = tts_scan_up<false>(e, s_lo, s_hi, level, lane);
    const int fwd_hi  = tts_scan_up<true>(e, s_hi, n - 1, level, lane);
    const int back_hi = tts_scan_down<false>(e, s_hi, level, lane);
    if (lane == 0) {
        wa_tts_record r;
        r.back_lo = back_lo; r.fwd_lo = fwd_lo; r.fwd_hi = fwd_hi; r.back_hi = back_hi;
        r.flags = (e_lo > level ? WA_TTS_LOUD_LO : 0u) | (e_hi > level ? WA_TTS_LOUD_HI : 0u) | (has_prev ? WA_TTS_HAS_PREV : 0u);
        r.level = level == level ? level : __int_as_float(0x7fc00000);
        rec[j] = r;
    }
}

bool wa_tts_energy_launch(void * stream, const float * d_pcm, int n, float * d_energy) {
    if (!d_pcm || !d_energy || n <= 0 || n > WA_TTS_MAX_N) return false;
    hipLaunchKernelGGL(k_tts_energy, dim3((unsigned) ((n + WA_TTS_TILE - 1) / WA_TTS_TILE)), dim3(256), 0, (hipStream_t) stream, d_pcm, n, d_energy);
    return hipGetLastError() == hipSuccess;
}

bool wa_tts_snap_launch(void * stream, const float * d_energy, int n, const int32_t * d_tok, int n_tokens, wa_tts_record * d_rec) {
    if (n_tokens <= 0) return true;
    if (!d_energy || !d_tok || !d_rec || n <= 0 || n > WA_TTS_MAX_N) return false;
    hipLaunchKernelGGL(k_tts_snap, dim3((unsigned) n_tokens), dim3(64), 0, (hipStream_t) stream, d_energy, n, d_tok, n_tokens, d_rec);
    return hipGetLastError() == hipSuccess;
}

// wa_vad.hip - k_vad_front: the part of the Silero VAD graph (whisper.cpp:4534-4598) that depends on one 512-sample window alone,
// for all windows of a slab at once: reflect pad, STFT as a conv_1d, magnitude, four Conv1d + bias + ReLU, and W_ih x + b_ih.
// The LSTM recurrence that consumes the result runs on the host (wa_vad_host.cpp).
//
// Every sum is formed in the reference's order (as wa_exact.hip): a convolution is an im2col ROUNDED TO F16 followed by
// ggml_vec_dot_f16 - 32 F32 partial sums s[k mod 32], each an FMA chain in k order, the fixed tree (wa_tree32), the K % 32 leftovers
// in F64; W_ih x is ggml_vec_dot_f32, the same chains and tree on F32 operands.  Products, adds and the square root of the magnitude
// are rounded one by one (-ffp-contract=off).  VALU, not MFMA: the MFMA's internal order is not the reference's.
//
// A workgroup (256 threads) takes WA_VAD_TILE windows and keeps everything between the samples and the result in LDS, each layer's
// output written straight into the NEXT layer's im2col rows (F16, zero where the convolution pads), so that every layer is a plain
// "rows x weight rows" product over contiguous K.  A lane owns a 2 x 2 patch of outputs - rows (2i, 2i+1), columns (j, j + N/2) - with
// all 32 partial sums of each in registers (128 accumulators); for the STFT the two columns are the real and imaginary part of one
// bin, so the magnitude is lane-local.  Activation rows come from LDS (the lanes of a wave share them: broadcast reads), weight rows
// from global memory: 354 KB of F16 + 256 KB of F32 that every workgroup reads and that stay in L2.
// LDS: 57 KB per workgroup, two workgroups per CU; ~200 VGPRs.
#include "wa_device.h"
#include "wa_vad.h"

#define VT     WA_VAD_TILE
#define V_PS   648                 // halfs per padded window (640 + 8: 16-byte rows, successive windows on different banks)
#define V_LD01 WA_VAD_LD0          // im2col row stride of layers 0 (K = 387) and 1 (K = 384)
#define V_LD23 200                 // ... of layers 2 and 3 (K = 192)
#define V_LDX  132                 // floats per LSTM input row (K = 128)

typedef float f32x4v __attribute__((ext_vector_type(4)));

// r[p][q] = dot(a_p, w_q) over K halfs in ggml_vec_dot_f16 order; a in LDS, w in global memory (the next 32 k are loaded ahead)
template <int K>
__device__ __forceinline__ void vad_patch_f16(const h16 * a0, const h16 * a1, const h16 * __restrict__ w0, const h16 * __restrict__ w1, float (&r)[2][2]) {
    float acc[2][2][32];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int i = 0; i < 32; ++i) acc[p][q][i] = 0.0f;
    constexpr int NS = K / 32;
    half8 w[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { w[0][c] = *(const half8 *) (w0 + c * 8); w[1][c] = *(const half8 *) (w1 + c * 8); }
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {
        const int sn = (s + 1 < NS ? s + 1 : s) * 32;
        half8 wn[2][4], a[2][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { wn[0][c] = *(const half8 *) (w0 + sn + c * 8); wn[1][c] = *(const half8 *) (w1 + sn + c * 8); }
#pragma unroll
        for (int c = 0; c < 4; ++c) { a[0][c] = *(const half8 *) (a0 + s * 32 + c * 8); a[1][c] = *(const half8 *) (a1 + s * 32 + c * 8); }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        acc[p][q][c * 8 + i] = fmaf((float) w[q][c][i], (float) a[p][c][i], acc[p][q][c * 8 + i]);
#pragma unroll
        for (int c = 0; c < 4; ++c) { w[0][c] = wn[0][c]; w[1][c] = wn[1][c]; }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float res = wa_tree32(acc[p][q]);
            if (K % 32 != 0) {          // leftovers in F64, index order (vec.cpp:221-223)
                double sumf = (double) res;
                const h16 * ar = p ? a1 : a0, * wr = q ? w1 : w0;
                for (int i = NS * 32; i < K; ++i) sumf += (double) ((float) ar[i] * (float) wr[i]);
                res = (float) sumf;
            }
            r[p][q] = res;
        }
}

// the same on F32 operands (ggml_vec_dot_f32 of the AVX2 build), K % 32 == 0
template <int K>
__device__ __forceinline__ void vad_patch_f32(const float * a0, const float * a1, const float * __restrict__ w0, const float * __restrict__ w1, float (&r)[2][2]) {
    float acc[2][2][32];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int i = 0; i < 32; ++i) acc[p][q][i] = 0.0f;
#pragma unroll 1
    for (int s = 0; s < K / 32; ++s) {
        f32x4v w[2][8], a[2][8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { w[0][c] = *(const f32x4v *) (w0 + s * 32 + c * 4); w[1][c] = *(const f32x4v *) (w1 + s * 32 + c * 4); }
#pragma unroll
        for (int c = 0; c < 8; ++c) { a[0][c] = *(const f32x4v *) (a0 + s * 32 + c * 4); a[1][c] = *(const f32x4v *) (a1 + s * 32 + c * 4); }
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        acc[p][q][c * 4 + i] = fmaf(w[q][c][i], a[p][c][i], acc[p][q][c * 4 + i]);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) r[p][q] = wa_tree32(acc[p][q]);
}

// One layer: M rows (even) x N weight rows (even).  rowa(r) = LDS address of activation row r; epi(r, j, lo, hi) receives row r's
// outputs for the weight rows j and j + N/2.
template <int K, class RowA, class Epi>
__device__ __forceinline__ void vad_layer_f16(int M, int N, RowA rowa, const wa_f16 * __restrict__ W, int ldw, Epi epi) {
    const int np = N >> 1, total = (M >> 1) * np;
    for (int p = threadIdx.x; p < total; p += 256) {
        const int rp = p / np, j = p - rp * np;
        float r[2][2];
        vad_patch_f16<K>((const h16 *) rowa(2 * rp), (const h16 *) rowa(2 * rp + 1), (const h16 *) W + (size_t) j * ldw, (const h16 *) W + (size_t) (j + np) * ldw, r);
        epi(2 * rp, j, r[0][0], r[0][1]);
        epi(2 * rp + 1, j, r[1][0], r[1][1]);
    }
}

// value v of (window c, time t, channel oc) of a layer's output -> the im2col rows of the next layer (k = 3, padding 1, `stride`,
// lout output steps): row (c, t') holds it at column oc * 3 + k where t' * stride + k - 1 == t
__device__ __forceinline__ void vad_scatter(wa_f16 * I, int ld, int c, int lout, int stride, int t, int oc, wa_f16 v) {
    for (int tp = 0; tp < lout; ++tp) {
        const int k = t + 1 - stride * tp;
        if (k >= 0 && k < 3) I[(c * lout + tp) * ld + oc * 3 + k] = v;
    }
}
__device__ __forceinline__ float vad_bias_relu(float v, float b) { const float y = v + b; return y > 0.f ? y : 0.f; }

// The front end of one workgroup: VT windows from load(c, s) - sample s (0 .. 511) of the workgroup's window c, 0.0f where there is none -
// through every layer; store(c, j, lo, hi) receives gate inputs j and j + 256 of window c (b_ih added).  k_vad_front and k_stream_vad_front
// are this body with their own load and store: the layers, their order of operations and the LDS layout are stated once.
template <class Load, class Store>
__device__ __forceinline__ void vad_front_body(const wa_vad_dev & W, Load load, Store store) {
    __shared__ __attribute__((aligned(16))) wa_f16 P[VT * V_PS];              // padded windows, F16 (the STFT's im2col rounds them)
    __shared__ __attribute__((aligned(16))) wa_f16 I0[VT * 4 * V_LD01];       // im2col rows of layer 0: (window, t) x 129 * 3
    __shared__ __attribute__((aligned(16))) wa_f16 I1[VT * 2 * V_LD01];       // layer 1: (window, t) x 128 * 3
    __shared__ __attribute__((aligned(16))) wa_f16 I2[VT * V_LD23];           // layer 2: window x 64 * 3
    __shared__ __attribute__((aligned(16))) wa_f16 I3[VT * V_LD23];           // layer 3: window x 64 * 3
    __shared__ __attribute__((aligned(16))) float  X[VT * V_LDX];             // LSTM input: window x 128
    const int tid = threadIdx.x;

    // windows: zero-filled past the end of the audio, then reflect-padded by 64 (ops.cpp:6784-6790: left[-i] = left[i], right[i] = right[-i])
    for (int idx = tid; idx < VT * (WA_VAD_WINDOW + 2 * WA_VAD_PAD); idx += 256) {
        const int c = idx / (WA_VAD_WINDOW + 2 * WA_VAD_PAD), j = idx - c * (WA_VAD_WINDOW + 2 * WA_VAD_PAD);
        const int s = j < WA_VAD_PAD ? WA_VAD_PAD - j : j < WA_VAD_PAD + WA_VAD_WINDOW ? j - WA_VAD_PAD : 2 * WA_VAD_WINDOW + WA_VAD_PAD - 2 - j;
        P[c * V_PS + j] = f2h(load(c, s));
    }
    for (int i = tid; i < VT * 4 * V_LD01; i += 256) I0[i] = 0;
    for (int i = tid; i < VT * 2 * V_LD01; i += 256) I1[i] = 0;
    for (int i = tid; i < VT * V_LD23; i += 256) { I2[i] = 0; I3[i] = 0; }
    __syncthreads();

    // STFT (K = 256, stride 128: 4 frames per window) + magnitude sqrtf(re re + im im) -> layer 0's rows (stride 1, 4 steps)
    vad_layer_f16<WA_VAD_NFFT>(VT * 4, 2 * WA_VAD_BINS, [&](int r) { return &P[(r >> 2) * V_PS + (r & 3) * WA_VAD_HOP]; }, W.stft, WA_VAD_NFFT,
        [&](int r, int j, float re, float im) {
            const float r2 = re * re, i2 = im * im;
            vad_scatter(I0, V_LD01, r >> 2, 4, 1, r & 3, j, f2h(sqrtf(r2 + i2)));
        });
    __syncthreads();
    // layer 0: 129 -> 128, stride 1, 4 steps -> layer 1's rows (stride 2, 2 steps)
    vad_layer_f16<387>(VT * 4, 128, [&](int r) { return &I0[r * V_LD01]; }, W.enc_w[0], WA_VAD_LD0,
        [&](int r, int j, float lo, float hi) {
            vad_scatter(I1, V_LD01, r >> 2, 2, 2, r & 3, j,      f2h(vad_bias_relu(lo, W.enc_b[0][j])));
            vad_scatter(I1, V_LD01, r >> 2, 2, 2, r & 3, j + 64, f2h(vad_bias_relu(hi, W.enc_b[0][j + 64])));
        });
    __syncthreads();
    // layer 1: 128 -> 64, stride 2, 2 steps -> layer 2's rows (stride 2, 1 step)
    vad_layer_f16<384>(VT * 2, 64, [&](int r) { return &I1[r * V_LD01]; }, W.enc_w[1], 384,
        [&](int r, int j, float lo, float hi) {
            vad_scatter(I2, V_LD23, r >> 1, 1, 2, r & 1, j,      f2h(vad_bias_relu(lo, W.enc_b[1][j])));
            vad_scatter(I2, V_LD23, r >> 1, 1, 2, r & 1, j + 32, f2h(vad_bias_relu(hi, W.enc_b[1][j + 32])));
        });
    __syncthreads();
    // layer 2: 64 -> 64, stride 2, 1 step -> layer 3's rows (stride 1, 1 step)
    vad_layer_f16<192>(VT, 64, [&](int r) { return &I2[r * V_LD23]; }, W.enc_w[2], 192,
        [&](int r, int j, float lo, float hi) {
            vad_scatter(I3, V_LD23, r, 1, 1, 0, j,      f2h(vad_bias_relu(lo, W.enc_b[2][j])));
            vad_scatter(I3, V_LD23, r, 1, 1, 0, j + 32, f2h(vad_bias_relu(hi, W.enc_b[2][j + 32])));
        });
    __syncthreads();
    // layer 3: 64 -> 128, stride 1, 1 step: its time step 0 is the LSTM's input, in F32
    vad_layer_f16<192>(VT, 128, [&](int r) { return &I3[r * V_LD23]; }, W.enc_w[3], 192,
        [&](int r, int j, float lo, float hi) {
            X[r * V_LDX + j]      = vad_bias_relu(lo, W.enc_b[3][j]);
            X[r * V_LDX + j + 64] = vad_bias_relu(hi, W.enc_b[3][j + 64]);
        });
    __syncthreads();
    // W_ih x + b_ih (F32 weights, K = 128)
    {
        const int np = WA_VAD_GATES / 2, total = (VT / 2) * np;
        for (int p = tid; p < total; p += 256) {
            const int rp = p / np, j = p - rp * np;
            float r[2][2];
            vad_patch_f32<WA_VAD_HID>(&X[(2 * rp) * V_LDX], &X[(2 * rp + 1) * V_LDX], W.w_ih + (size_t) j * WA_VAD_HID, W.w_ih + (size_t) (j + np) * WA_VAD_HID, r);
            store(2 * rp,     j, r[0][0] + W.b_ih[j], r[0][1] + W.b_ih[j + np]);
            store(2 * rp + 1, j, r[1][0] + W.b_ih[j], r[1][1] + W.b_ih[j + np]);
        }
    }
}

struct vad_front_args {
    wa_vad_dev w;
    const float * samples;
    int n_valid, n_chunks;
    float * out;
};

__global__ __launch_bounds__(256, 2) void k_vad_front(vad_front_args A) {
    const int chunk0 = blockIdx.x * VT;
    vad_front_body(A.w,
        [&](int c, int s) {
            const long long g = (long long) (chunk0 + c) * WA_VAD_WINDOW + s;
            return (chunk0 + c < A.n_chunks && g < (long long) A.n_valid) ? A.samples[g] : 0.0f;
        },
        [&](int c, int j, float lo, float hi) {
            if (chunk0 + c < A.n_chunks) {
                A.out[(size_t) (chunk0 + c) * WA_VAD_GATES + j]                    = lo;
                A.out[(size_t) (chunk0 + c) * WA_VAD_GATES + j + WA_VAD_GATES / 2] = hi;
            }
        });
}

bool wa_vad_front_launch(const wa_vad_dev & w, const float * d_samples, int n_valid, int n_chunks, float * d_out, void * stream) {
    if (n_chunks <= 0) return true;
    vad_front_args a;
    a.w = w; a.samples = d_samples; a.n_valid = n_valid; a.n_chunks = n_chunks; a.out = d_out;
    hipLaunchKernelGGL(k_vad_front, dim3((n_chunks + VT - 1) / VT), dim3(256), 0, (hipStream_t) stream, a);
    return hipGetLastError() == hipSuccess;
}

// k_stream_vad_front: the same front end on the ring windows of up to WA_SVAD_SESSIONS live sessions (wa_stream_vad.cpp).
// The (session, window) pairs of a launch form one flat list - session 0's new windows, then session 1's, ... - that travels as its prefix
// counts; workgroup b takes flat rows 8 b .. 8 b + 7 whatever sessions they belong to.  Sample s of a session's window k is ring slot
// (slot + 512 k + s) mod cap, zero at and past n_valid (a flush's partial window): the loads go straight into the LDS tile above, so a window
// may wrap inside the ring and start at any slot.  Row k's 512 gate inputs go to out + 512 k, the session's pinned host buffer.
struct svad_front_args {
    wa_vad_dev w;
    wa_svad_table t;
};

__global__ __launch_bounds__(256, 2) void k_stream_vad_front(svad_front_args A) {
    __shared__ int row_s[VT], row_k[VT];            // the session and the window of each tile row; session -1: no row
    if (threadIdx.x < VT) {
        const int f = blockIdx.x * VT + threadIdx.x;
        int s = -1, k = 0;
        if (f < A.t.first[A.t.n_sessions]) {
            s = 0;
            while (s + 1 < A.t.n_sessions && f >= A.t.first[s + 1]) ++s;
            k = f - A.t.first[s];
        }
        row_s[threadIdx.x] = s; row_k[threadIdx.x] = k;
    }
    __syncthreads();
    vad_front_body(A.w,
        [&](int c, int s) {
            const int i = row_s[c];
            if (i < 0) return 0.0f;
            const wa_svad_session & z = A.t.s[i];
            const int off = row_k[c] * WA_VAD_WINDOW + s;
            return off < z.n_valid ? z.ring[(int) (((long long) z.slot + off) % z.cap)] : 0.0f;
        },
        [&](int c, int j, float lo, float hi) {
            const int i = row_s[c];
            if (i >= 0) {
                float * o = A.t.s[i].out + (size_t) row_k[c] * WA_VAD_GATES;
                o[j] = lo; o[j + WA_VAD_GATES / 2] = hi;
            }
        });
}

bool wa_svad_front_launch(const wa_vad_dev & w, const wa_svad_table & t, void * stream) {
    if (t.n_sessions <= 0 || t.n_sessions > WA_SVAD_SESSIONS || t.first[0] != 0) return false;
    for (int i = 0; i < t.n_sessions; ++i) {
        const wa_svad_session & z = t.s[i];
        const int n = t.first[i + 1] - t.first[i];
        if (n < 0 || n > WA_SVAD_MAX_WINDOWS) return false;
        if (n > 0 && (!z.ring || !z.out || z.cap <= 0 || z.slot < 0 || z.slot >= z.cap || z.n_valid <= (n - 1) * WA_VAD_WINDOW || z.n_valid > n * WA_VAD_WINDOW ||
                      z.n_valid > z.cap)) return false;
    }
    const int total = t.first[t.n_sessions];
    if (total == 0) return true;
    svad_front_args a;
    a.w = w; a.t = t;
    hipLaunchKernelGGL(k_stream_vad_front, dim3((total + VT - 1) / VT), dim3(256), 0, (hipStream_t) stream, a);
    return hipGetLastError() == hipSuccess;
}

// wa_vad_lstm.hip - k_vad_lstm: the Silero VAD's LSTM recurrence on the device, bit for bit what wa_vad_step (wa_vad_host.cpp) computes.
//
// The recurrence is serial in time and tiny per step (a 512 x 128 product, 640 transcendental calls, a 128-wide dot), so the kernel is built
// around latency, not throughput: ONE persistent workgroup per sequence walks all its windows, and a launch carries up to WA_VLSTM_SEQS
// independent sequences (grid.x), which never talk to one another - no global atomics, no flags, nothing spins.
//
// Work split, 512 threads = 8 waves, two per SIMD:
//   * thread j owns gate row j (order i, f, g, o as in the file).  Its 128 F32 weights of W_hh are loaded ONCE into registers (128 VGPRs) and
//     stay there for the whole launch; b_hh[j] beside them.  h [128] lives in LDS and every lane reads the same address (32 broadcast
//     ds_read_b128 per window).  The dot is ggml_vec_dot_f32's AVX2 order: 32 chains s[k mod 32] in k order, wa_vad_host.cpp's tree.
//   * gate sum: gate_in[j] + (hid + b_hh[j]), the host function's bracketing; then sigmoid (i, f, o) or tanh (g) through wa_libm.h, the
//     activation to LDS.                                                                                          -- barrier 1 --
//   * threads 0..127 own state element j: c stays in a register across windows; f c, i g, their sum, o tanh(c) each round on their own
//     (-ffp-contract=off).  h goes to LDS, into the buffer of this window's parity.                              -- barrier 2 --
//   * the output (relu, one rounding to F16, the 128-wide dot with the F16 weight in 32 chains, the tree, + bias, sigmoid) of window t is
//     wave 7's job DURING the state phase of window t + 1, in which it would idle: it reads h of window t from the other parity's buffer, 32
//     lanes hold one chain each and the tree is five shuffles in the host tree's pairing.  So the serial path per window is dot -> activation
//     -> barrier -> state -> barrier and nothing else; two barriers is what gates -> state -> next dot allows.
//   * the gate input of window t + 1 is loaded at the top of window t (one coalesced 2 KB row per workgroup) and used a window later.
// wa_expf_full's table (256 bytes; its index depends on the argument, so the read is in series with the result) is copied to LDS once.
//
// Built with -fno-gpu-flush-denormals-to-zero (Makefile): a subnormal state entry, gate product or exp result must stay one.  F32 division is
// the correctly rounded one (hipcc's default).  Code object: 512 threads, no scratch, no spills (DESIGN.md 4.7 records the register count).
#include <hip/hip_runtime.h>

#include "wa_vad.h"
#include "wa_libm.h"

static __device__ const unsigned long long VLSTM_EXP2F_T[32] = WA_LIBM_EXP2F_TABLE;

struct vlstm_args {
    const float * w_hh, * b_hh;
    const uint16_t * w_f;
    float b_f;
    wa_vlstm_table t;
};

__device__ __forceinline__ float vlstm_tree32(const float (&s)[32]) {
    float a[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) a[l] = (s[l] + s[16 + l]) + (s[8 + l] + s[24 + l]);
    const float t0 = a[0] + a[4], t1 = a[1] + a[5], t2 = a[2] + a[6], t3 = a[3] + a[7];
    return (t0 + t1) + (t2 + t3);
}

__device__ __forceinline__ float vlstm_f16_bits_to_f32(uint16_t u) { _Float16 h; __builtin_memcpy(&h, &u, 2); return (float) h; }

// wave 7: the probability of the window whose h lies in `h`; lane l and lane l + 32 both hold chain l, lane 0's result is the full tree
__device__ __forceinline__ float vlstm_output(const float * h, const float (&wf)[4], float b_f, int l, const unsigned long long * tab) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float v = h[l + 32 * i];
        const float x = (float) (_Float16) (v > 0.f ? v : 0.f);          // relu, then the final conv's im2col rounds to F16 once
        s = __builtin_fmaf(x, wf[i], s);
    }
    s = s + __shfl_down(s, 16);        // l < 16: s[l] + s[16 + l]
    s = s + __shfl_down(s, 8);         // l < 8:  (s[l] + s[16 + l]) + (s[8 + l] + s[24 + l])
    s = s + __shfl_down(s, 4);         // l < 4:  a[l] + a[l + 4]
    s = s + __shfl_down(s, 1);         // l = 0, 2: t0 + t1, t2 + t3
    s = s + __shfl_down(s, 2);         // l = 0
    return wa_sigmoidf_libm(s + b_f, tab);
}

__global__ __launch_bounds__(512) void k_vad_lstm(vlstm_args A) {
    __shared__ __attribute__((aligned(16))) float h_s[2][WA_VAD_HID];
    __shared__ float act_s[WA_VAD_GATES];
    __shared__ unsigned long long tab_s[32];
    const wa_vlstm_seq q = A.t.s[blockIdx.x];
    const int j = threadIdx.x, n = q.n;
    if (n <= 0) return;                                  // the whole workgroup: nothing of this sequence is touched

    float w[WA_VAD_HID];
    {
        const float4 * wr = (const float4 *) (A.w_hh + (size_t) j * WA_VAD_HID);
#pragma unroll
        for (int i = 0; i < WA_VAD_HID / 4; ++i) { const float4 v = wr[i]; w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
    }
    const float bh = A.b_hh[j];
    const bool is_g = (j >> 7) == 2, state = j < WA_VAD_HID, outw = j >= 448;
    const int l = j & 31;
    float wf[4] = { 0.f, 0.f, 0.f, 0.f };
    if (outw) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wf[i] = vlstm_f16_bits_to_f32(A.w_f[l + 32 * i]);
    }
    float c = 0.0f;
    if (state) { h_s[1][j] = q.h[j]; c = q.c[j]; }       // window -1's parity
    if (j < 32) tab_s[j] = VLSTM_EXP2F_T[j];
    float g_cur = q.gates[j];
    __syncthreads();

    for (int t = 0; t < n; ++t) {
        const float * h_prev = h_s[(t & 1) ^ 1];
        float * h_now = h_s[t & 1];
        float g_next = 0.0f;
        if (t + 1 < n) g_next = q.gates[(size_t) (t + 1) * WA_VAD_GATES + j];
        float s[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) s[k] = 0.0f;
#pragma unroll
        for (int k4 = 0; k4 < WA_VAD_HID / 4; ++k4) {
            const float4 hv = ((const float4 *) h_prev)[k4];
            const int k = 4 * k4;
            s[k & 31]       = __builtin_fmaf(w[k],     hv.x, s[k & 31]);
            s[(k + 1) & 31] = __builtin_fmaf(w[k + 1], hv.y, s[(k + 1) & 31]);
            s[(k + 2) & 31] = __builtin_fmaf(w[k + 2], hv.z, s[(k + 2) & 31]);
            s[(k + 3) & 31] = __builtin_fmaf(w[k + 3], hv.w, s[(k + 3) & 31]);
        }
        const float g = g_cur + (vlstm_tree32(s) + bh);
        act_s[j] = is_g ? wa_tanhf_libm(g) : wa_sigmoidf_libm(g, tab_s);
        __syncthreads();
        if (state) {
            const float i_t = act_s[j], f_t = act_s[WA_VAD_HID + j], g_t = act_s[2 * WA_VAD_HID + j], o_t = act_s[3 * WA_VAD_HID + j];
            const float fc = f_t * c, ig = i_t * g_t;
            c = fc + ig;
            h_now[j] = o_t * wa_tanhf_libm(c);
        } else if (outw && t > 0) {
            const float p = vlstm_output(h_prev, wf, A.b_f, l, tab_s);
            if (j == 448) q.probs[t - 1] = p;
        }
        __syncthreads();
        g_cur = g_next;
    }
    const float * h_last = h_s[(n - 1) & 1];
    if (outw) {
        const float p = vlstm_output(h_last, wf, A.b_f, l, tab_s);
        if (j == 448) q.probs[n - 1] = p;
    }
    if (state) { q.h[j] = h_last[j]; q.c[j] = c; }
}

bool wa_vlstm_launch(const wa_vad_dev & w, const wa_vlstm_table & t, void * stream) {
    if (!w.w_hh || !w.b_hh || !w.w_f || t.n_seqs <= 0 || t.n_seqs > WA_VLSTM_SEQS) return false;
    bool any = false;
    for (int i = 0; i < t.n_seqs; ++i) {
        const wa_vlstm_seq & q = t.s[i];
        if (q.n < 0 || (q.n > 0 && (!q.gates || !q.h || !q.c || !q.probs))) return false;
        any = any || q.n > 0;
    }
    if (!any) return true;
    vlstm_args a;
    a.w_hh = w.w_hh; a.b_hh = w.b_hh; a.w_f = w.w_f; a.b_f = w.b_f; a.t = t;
    hipLaunchKernelGGL(k_vad_lstm, dim3(t.n_seqs), dim3(512), 0, (hipStream_t) stream, a);
    return hipGetLastError() == hipSuccess;
}

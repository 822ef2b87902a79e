// wa_quantk_rows.hip - the K-format products (Q2_K / Q3_K / Q5_K / Q6_K weights, wa_quantk.hip) of M = R = 2..8 activation rows: a beam / best_of step,
// a small whisper_decode batch.  The one-row kernel's shape (k_kgemv_exact), as k_qgemv_rows of wa_quant.hip has it for the 32-value formats:
// grid = ceil(N / 8) single-wave workgroups, 8 output rows x 8 lanes, no LDS, nothing waits for another workgroup; lane l of a group owns elements
// 4 l .. 4 l + 3 of every 32-element group of a block.  A lane's loads for a weight block - two 16-byte quant loads, its 8 scale bytes (Q5_K: the 8
// scales and the 8 minimums; Q2_K: and its two minimum bytes), d (and dmin) - are issued ONCE, WKR_DEPTH blocks ahead of the arithmetic, and meet
// all R activation rows, which every wave reads from L2 in the same 16-byte pattern (the Q8_K layout of wa_launch_quantize_q8_K).
// Per (activation row, output) the arithmetic is k_kgemm_exact's - wk_block integer sums, acc[r] = fma(dx * dw, (float) t, acc[r]) block after
// block, wk_hsum8 - so the results are the same bits.  Q2_K: the minimum term goes into acc[r] first, by an fma of its own, lane-local for every
// row.  Q5_K: lane l runs the scalar chain of activation row min(l, R - 1) from that row's sixteen block sums and lane 0 fetches row r's chain by
// one DPP move after hsum.  Against k_kgemm_exact (32 output rows per workgroup, activation rows through LDS, one load group in flight) a narrow
// matrix gets 4 x the workgroups: N = 768 -> 96, not 24.
// A code object of its own (build/wa_quantk_rows.o): wa_quantk.o, wa_quantk_q2.o and wa_quantk_mfma.o reference nothing here.
#include <cstdlib>
#include "wa_quantk_dev.h"

#define WKR_DEPTH 4        // weight blocks in flight ahead of the arithmetic; nb = K / 256 = 1 .. 20 may be shorter: the loads are clamped to the last block

// what a lane holds of one weight block
template <int F> struct wkr_wblock {
    wk_i4 w0, w1;      // the lane's 32 quants
    wk_i2 s;           // Q6_K, Q2_K: the lane's half of the 16 scales; Q5_K: the 8 scales
    wk_i2 mm;          // Q5_K: the 8 minimums
    int ma, mb;        // Q2_K: the minimums of the lane's sub-blocks 2 l and 2 l + 1
    float dw, dwm;     // d; dmin (Q5_K, Q2_K)
};
template <int F>
__device__ __forceinline__ wkr_wblock<F> wkr_load(const wk_i4 * __restrict__ wl, const int8_t * __restrict__ sl, const float * __restrict__ dl,
                                                  const float * __restrict__ ml, int b, int l) {
    wkr_wblock<F> w;
    w.mm = wk_i2{0, 0}; w.ma = w.mb = 0; w.dwm = 0.0f;          // (the members a format does not use)
    w.w0 = wl[2 * b]; w.w1 = wl[2 * b + 1];
    w.s = *(const wk_i2 *) (sl + 16 * b + (F == WK_Q5 ? 0 : 8 * (l >> 2)));
    w.dw = dl[b];
    if (F == WK_Q5) { w.mm = *(const wk_i2 *) (sl + 16 * b + 8); w.dwm = ml[b]; }
    if (F == WK_Q2) {          // bytes l and 8 + l of the block's 16, the minimum in the high nibble
        const uint8_t * sb = (const uint8_t *) sl + 16 * b;
        w.ma = sb[l] >> 4; w.mb = sb[8 + l] >> 4; w.dwm = ml[b];
    }
    return w;
}

template <int EPI, int F, int R>
__global__ __launch_bounds__(64) void k_kgemv_rows(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int16_t * __restrict__ xbs,
                                                   const int8_t * __restrict__ wq, const int8_t * __restrict__ wsc, const float * __restrict__ wd,
                                                   const float * __restrict__ wdm, int N, int K, wa_epi e) {
    constexpr bool Q5 = F == WK_Q5, Q2 = F == WK_Q2;
    const int tid = threadIdx.x, l = tid & 7, nb = K >> 8;
    const int n = blockIdx.x * 8 + (tid >> 3);
    const int nn = n < N ? n : N - 1;
    wa_epi_pre pre[R];
#pragma unroll
    for (int r = 0; r < R; ++r) if (l == 0) pre[r] = epi_preload<EPI>(e, r, nn);
    const wk_i4 * wl = (const wk_i4 *) (wq + ((size_t) nn * 8 + l) * nb * 32);
    const int8_t * sl = wsc + (size_t) nn * nb * 16;
    const float * dl = wd + (size_t) nn * nb;
    const float * ml = (Q5 || Q2) ? wdm + (size_t) nn * nb : dl;
    const wk_i4 * xl = (const wk_i4 *) (xq + (size_t) l * nb * 32);            // row r: + r * (K >> 4)
    const int rc = l < R ? l : R - 1;                                           // Q5_K: the activation row whose minimum chain this lane runs
    const float * xdc = xd + (size_t) rc * nb;
    const wk_i4 * xbc = (const wk_i4 *) (xbs + (size_t) rc * nb * 16);           // its sixteen 16-element sums of a block: two 16-byte loads
    // Q2_K: the rows' d through the vector path (a lane offset of zero that the compiler cannot see through).  As uniform loads they and the rows'
    // addresses, which Q2_K has most of, ran out of scalar registers at 7 and 8 rows.
    int zl = 0;
    if (Q2) asm volatile("" : "+v"(zl));
    float acc[R];
    float summs = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
    wkr_wblock<F> wn[WKR_DEPTH];
#pragma unroll
    for (int j = 0; j < WKR_DEPTH; ++j) wn[j] = wkr_load<F>(wl, sl, dl, ml, min(j, nb - 1), l);
    for (int b0 = 0; b0 < nb; b0 += WKR_DEPTH) {
#pragma unroll
        for (int j = 0; j < WKR_DEPTH; ++j) {
            const wkr_wblock<F> w = wn[j];
            wn[j] = wkr_load<F>(wl, sl, dl, ml, min(b0 + WKR_DEPTH + j, nb - 1), l);
            // (clamped: the loads of a round's blocks go out together; a block beyond the row is computed on the last block's data and not added)
            const int b = min(b0 + j, nb - 1);
            const bool live = b0 + j < nb;
            wk_i4 x0[R], x1[R]; float dx[R]; int bs2[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                x0[r] = xl[(size_t) r * (K >> 4) + 2 * b]; x1[r] = xl[(size_t) r * (K >> 4) + 2 * b + 1];
                dx[r] = xd[(size_t) r * nb + b + zl];
                if (Q2) bs2[r] = *(const int *) (xbs + ((size_t) r * nb + b) * 16 + 2 * l);        // bsums[2 l] | bsums[2 l + 1] << 16
            }
            wk_i4 g0, g1; float dxc = 0.0f;
            if (Q5) { g0 = xbc[2 * b]; g1 = xbc[2 * b + 1]; dxc = xdc[b]; }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float a = acc[r];
                if (Q2) {                         // the minimum term first, then the product term
                    const float dn = -dx[r] * w.dwm;
                    a = fmaf(dn, (float) (w.ma * ((bs2[r] << 16) >> 16) + w.mb * (bs2[r] >> 16)), a);
                }
                const float dd = dx[r] * w.dw;
                a = fmaf(dd, (float) wk_block<F>(w.w0, w.w1, x0[r], x1[r], w.s), a);
                acc[r] = live ? a : acc[r];
            }
            if (Q5) {                             // the sums of the 32-element groups, bsums[2 g] + bsums[2 g + 1], against the 8 minimums
#define WKR_G(v) ((((v) << 16) >> 16) + ((v) >> 16))
                const int tot = wk_byte<WK_Q5>(w.mm, 0) * WKR_G(g0.x) + wk_byte<WK_Q5>(w.mm, 1) * WKR_G(g0.y) + wk_byte<WK_Q5>(w.mm, 2) * WKR_G(g0.z) +
                                wk_byte<WK_Q5>(w.mm, 3) * WKR_G(g0.w) + wk_byte<WK_Q5>(w.mm, 4) * WKR_G(g1.x) + wk_byte<WK_Q5>(w.mm, 5) * WKR_G(g1.y) +
                                wk_byte<WK_Q5>(w.mm, 6) * WKR_G(g1.z) + wk_byte<WK_Q5>(w.mm, 7) * WKR_G(g1.w);
#undef WKR_G
                const float dm = -dxc * w.dwm;
                const float p = dm * (float) tot;
                const float sn = summs + p;
                summs = live ? sn : summs;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float v = wk_hsum8(acc[r]);
        if (Q5) v = v + wk_from_lane(summs, r);
        if (l == 0 && n < N) epi_apply<EPI>(e, r, n, v, pre[r]);
    }
}

// The default rule, decided by the passes measured on the MI355X against the parent commit (DESIGN.md 4.3 has the table and says which cells are
// extrapolated): products of 2..7 rows go to the few-rows kernel at every width; products of 8 rows only at the model width d = 768, the one width at
// which the 8-row pass was faster by more than the spread of its three runs (Q6_K at d = 512 and d = 1280: within the spread, so the general kernel
// keeps them).  d is K, or N for the second MLP product (K = 4 N).  WHISPER_AMD_NO_FEW_ROWS=1 (read once per process; the switch of wa_quant.hip's
// k_qgemv_rows) sends everything back to k_kgemm_exact.
static bool kfew_rule(int M, int N, int K) {
    static const bool off = getenv("WHISPER_AMD_NO_FEW_ROWS") != nullptr;
    const int d = K == 4 * N ? N : K;
    return !off && M >= 2 && (M <= 7 || (M == 8 && d == 768));
}
// the kernel a route gives a product: 2 k_kgemv_rows, else what wa_kgemm_kernel says (1 k_kgemm_exact / k_kgemv_exact, 3 k_kgemm_mfma)
int wa_kgemm_few_kernel(wa_epi_mode mode, int wtype, int M, int N, int K, const wa_epi & e, int route) {
    const bool few_mode = mode == WA_EPI_F16 || mode == WA_EPI_GELU_F32 || mode == WA_EPI_RESID || mode == WA_EPI_F32 || mode == WA_EPI_DEC_QKV;
    if (M >= 2 && M <= 8 && few_mode && route != 1 && (route == 2 || kfew_rule(M, N, K))) return 2;
    return wa_kgemm_kernel(mode, wtype, M, N, K, e, route);        // (route 2 is route 0 to it)
}

template <int F>
static void kfew_launch(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq,
                        const int8_t * wsc, const float * wd, const float * wdm, int N, int K, const wa_epi & e) {
#define WA_ROWS_R(E, R) case R: hipLaunchKernelGGL((k_kgemv_rows<E, F, R>), dim3((N + 7) / 8), dim3(64), 0, s, xq, xd, xbs, wq, wsc, wd, wdm, N, K, e); break;
#define WA_ROWS_E(E) case E: switch (M) { WA_ROWS_R(E, 2) WA_ROWS_R(E, 3) WA_ROWS_R(E, 4) WA_ROWS_R(E, 5) WA_ROWS_R(E, 6) WA_ROWS_R(E, 7) WA_ROWS_R(E, 8) default: break; } break;
    switch (mode) {        // (the encoder's epilogues never see so few rows: they stay with k_kgemm_exact)
        WA_ROWS_E(WA_EPI_F16) WA_ROWS_E(WA_EPI_GELU_F32) WA_ROWS_E(WA_EPI_RESID) WA_ROWS_E(WA_EPI_F32) WA_ROWS_E(WA_EPI_DEC_QKV)
        default: break;
    }
#undef WA_ROWS_E
#undef WA_ROWS_R
}

// route 0: the rules pick the kernel; 1: never k_kgemv_rows (and wa_launch_kgemm_exact above 8 rows too); 2: k_kgemv_rows wherever it exists, the
// rule's kernel elsewhere; 3: wa_launch_kgemm_route's route 3
void wa_launch_kgemm_few_route(hipStream_t s, wa_epi_mode mode, int wtype, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq,
                               const int8_t * wsc, const float * wd, const float * wdm, int N, int K, const wa_epi & e, int route) {
    if (wa_kgemm_few_kernel(mode, wtype, M, N, K, e, route) != 2) {
        wa_launch_kgemm_route(s, mode, wtype, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e, route);
        return;
    }
    if (wtype == 13) kfew_launch<WK_Q5>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);
    else if (wtype == 10) kfew_launch<WK_Q2>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);
    else kfew_launch<WK_Q6>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);        // Q6_K, and Q3_K as the loader unpacks it
}

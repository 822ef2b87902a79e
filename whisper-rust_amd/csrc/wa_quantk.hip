// wa_quantk.hip - Q2_K / Q3_K / Q5_K / Q6_K weights (ggml K formats, 256-value blocks) in the reference's order.  The arithmetic is stated in host
// code in wa_quantk.h; these kernels restate it.
//
// With such a matrix the reference quantises the F32 activation row to Q8_K (quantize_row_q8_K_ref: the scale comes from the FIRST
// element of largest magnitude, with its sign) and forms every output as
//     sumi[l] = sum over the eight 32-element groups g of  sc(g, l) * sum_{e<4} w[32 g + 4 l + e] * x[32 g + 4 l + e]      exact integers
//     acc[l]  = fma( d_x * f32(d_w), (float) sumi[l], acc[l] )        l = 0..7, block after block
//     out     = hsum_float_8(acc)                                      (+ summs, Q5_K)
// (ggml_vec_dot_q6_K_q8_K / q5_K_q8_K, AVX2).  As in wa_quant.hip: 8 lanes per output row, lane l owns elements 4 l .. 4 l + 3 of every
// group (one v_dot4_i32_i8 and one integer multiply-add by the sub-block scale per group), three DPP adds are hsum_float_8.
// Q5_K: the quants are unsigned 0..31, and a scalar chain over the blocks runs beside the lane chain,
//     summs = summs + ((-d_x * f32(dmin_w)) * (float) sum_b m[b] * (bsums[2 b] + bsums[2 b + 1]))       a multiplication, then an addition
// In the one-row product lane b of the group forms m[b] * (its group's sum), three integer DPP adds bring the total to lane 0, which
// runs the chain; with 8 activation rows lane l runs the chain of activation row l and hands it to lane 0 over DPP.
// Layout (wa_quantk.h, made at load by wa_loader.cpp): quants int8 [row][lane][block][group][4] - a lane's 32 bytes of a block are two
// 16-byte loads -, scale bytes [row][block][16] (Q6_K: the lane's half first / second eight; Q5_K: scales, then minimums), d / dmin f32
// [row][block].  Activation rows: the same quant order, d f32 [row][block], the 16-element sums int16 [row][block][16].
// Q3_K, unpacked at load (quants -4..3, signed 6-bit scales in Q6_K's order, one d), IS a Q6_K matrix: it runs the Q6_K instantiations.
// Q2_K (quants 0..3; scale bytes in Q6_K's order, the scale in the low nibble and the minimum in the high one; d and dmin) is a format of
// its own (WK_Q2): the minimums go into the LANE accumulators, per block before the product term and by an fma of their own,
//     acc[l] = fma( -d_x * f32(dmin_w), (float) (m[2 l] * bsums[2 l] + m[2 l + 1] * bsums[2 l + 1]), acc[l] ),  then the fma above,
// and lane l's two minimums are bytes l and 8 + l of the block's 16: no exchange between lanes, with one activation row or with eight.
// This file is compiled twice: wa_quantk.o holds everything but Q2_K, wa_quantk_q2.o (-DWA_QK_Q2_TU) the Q2_K instantiations of the two
// products and their launcher - a code object of their own beside the fourteen + fourteen of Q5_K / Q6_K.
#include "wa_quantk_dev.h"      // the vector types, wk_hsum8, the format enum WK_Q6 / WK_Q5 / WK_Q2, wk_byte, wk_block and wk_from_lane: shared with wa_quantk_mfma.hip / wa_quantk_rows.hip

__device__ __forceinline__ int wk_isum8(int v) {      // integer sum of an 8-lane group, valid in its lane 0 (any order is exact)
    v += __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x102, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x101, 0xf, 0xf, true);
    return v;
}

// -------------------------------------------------------------------------------------------------
// quantize_row_q8_K_ref: one wave per 256-value block, lane i holds elements 4 i .. 4 i + 3.  The arg-max keeps the FIRST index on ties
// (opposite signs included): strictly-greater inside the lane, then the lowest lane that holds the wave's maximum.
// -------------------------------------------------------------------------------------------------
#ifndef WA_QK_Q2_TU
__global__ __launch_bounds__(256) void k_quantize_q8_K(const float * __restrict__ x, int ldx, int rows, int K, int8_t * __restrict__ qs,
                                                       float * __restrict__ qd, int16_t * __restrict__ qbs) {
    const int nb = K >> 8;
    const long gb = (long) blockIdx.x * 4 + (threadIdx.x >> 6);      // wave-uniform
    const int i = threadIdx.x & 63;
    if (gb >= (long) rows * nb) return;
    const int row = (int) (gb / nb), b = (int) (gb - (long) row * nb);
    const float4 v = *(const float4 *) (x + (size_t) row * ldx + b * 256 + 4 * i);
    float amax = fabsf(v.x), mx = v.x;
    if (fabsf(v.y) > amax) { amax = fabsf(v.y); mx = v.y; }
    if (fabsf(v.z) > amax) { amax = fabsf(v.z); mx = v.z; }
    if (fabsf(v.w) > amax) { amax = fabsf(v.w); mx = v.w; }
    const float wmax = wave_max(amax);
    const unsigned long long holders = __ballot(amax == wmax);
    const int first = __ffsll((long long) holders) - 1;
    const float max = __shfl(mx, first, WAVE);
    int q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    float d = 0.0f;
    if (wmax != 0.0f) {
        const float iscale = -127.f / max;
        q0 = min(127, (int) rintf(iscale * v.x)); q1 = min(127, (int) rintf(iscale * v.y));
        q2 = min(127, (int) rintf(iscale * v.z)); q3 = min(127, (int) rintf(iscale * v.w));
        d = 1.0f / iscale;
    }
    // element 4 i + e of the block: group g = i >> 3, lane l = i & 7
    *(int *) (qs + (((size_t) row * 8 + (i & 7)) * nb + b) * 32 + (i >> 3) * 4) = (q0 & 0xff) | ((q1 & 0xff) << 8) | ((q2 & 0xff) << 16) | ((q3 & 0xff) << 24);
    int s = (q0 + q1) + (q2 + q3);
    s += __builtin_amdgcn_update_dpp(0, s, 0xb1, 0xf, 0xf, true);        // quad_perm [1, 0, 3, 2]
    s += __builtin_amdgcn_update_dpp(0, s, 0x4e, 0xf, 0xf, true);        // quad_perm [2, 3, 0, 1]: the 16 elements of lanes 4 j .. 4 j + 3
    if ((i & 3) == 0) qbs[((size_t) row * nb + b) * 16 + (i >> 2)] = (int16_t) s;
    if (i == 0) qd[(size_t) row * nb + b] = d;
}
void wa_launch_quantize_q8_K(hipStream_t stream, const float * x, int ldx, int rows, int K, int8_t * qs, float * qd, int16_t * qbs) {
    const long nblk = (long) rows * (K >> 8);
    hipLaunchKernelGGL(k_quantize_q8_K, dim3((unsigned) ((nblk + 3) / 4)), dim3(256), 0, stream, x, ldx, rows, K, qs, qd, qbs);
}
#endif

// -------------------------------------------------------------------------------------------------
// M == 1 (the decode step): grid = ceil(N / 8) single-wave workgroups, 8 output rows x 8 lanes each; no LDS.
// One output row per 8 lanes: the row's dot product with the activation row (valid in lane l == 0 of the group).
// -------------------------------------------------------------------------------------------------
template <int F>
__device__ __forceinline__ float wk_row_dot(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int16_t * __restrict__ xbs,
                                            const int8_t * __restrict__ wq, const int8_t * __restrict__ wsc, const float * __restrict__ wd,
                                            const float * __restrict__ wdm, int nn, int nb, int l) {
    const wk_i4 * wl = (const wk_i4 *) (wq + ((size_t) nn * 8 + l) * nb * 32);
    const wk_i4 * xl = (const wk_i4 *) (xq + (size_t) l * nb * 32);
    constexpr bool Q5 = F == WK_Q5;
    // Q6_K, Q2_K: the lane's half of the 16 scales; Q5_K: the 8 scales (the minimums are the second eight)
    const int8_t * sl = wsc + (size_t) nn * nb * 16 + (Q5 ? 0 : 8 * (l >> 2));
    const float * dl = wd + (size_t) nn * nb;
    float acc = 0.0f, summs = 0.0f;
#pragma unroll 2
    for (int b = 0; b < nb; ++b) {
        const wk_i4 w0 = wl[2 * b], w1 = wl[2 * b + 1], x0 = xl[2 * b], x1 = xl[2 * b + 1];
        const wk_i2 s = *(const wk_i2 *) (sl + 16 * b);
        const float dx = xd[b];
        const float dd = dx * dl[b];
        const int t = wk_block<F>(w0, w1, x0, x1, s);
        if (F == WK_Q2) {                 // this lane's sub-blocks 2 l and 2 l + 1: bytes l and 8 + l of the block's scales, the minimum in the high nibble
            const uint8_t * sb = (const uint8_t *) wsc + ((size_t) nn * nb + b) * 16;
            const int bs2 = *(const int *) (xbs + 16 * b + 2 * l);
            const int mins = (int) (sb[l] >> 4) * ((bs2 << 16) >> 16) + (int) (sb[8 + l] >> 4) * (bs2 >> 16);
            const float dn = -dx * wdm[(size_t) nn * nb + b];
            acc = fmaf(dn, (float) mins, acc);
        }
        acc = fmaf(dd, (float) t, acc);
        if (Q5) {
            const int mb = (int) (unsigned char) sl[16 * b + 8 + l];                   // this lane's group: m[l] * (bsums[2 l] + bsums[2 l + 1])
            const int bs2 = *(const int *) (xbs + 16 * b + 2 * l);
            const int tot = wk_isum8(mb * (((bs2 << 16) >> 16) + (bs2 >> 16)));
            const float dm = -dx * wdm[(size_t) nn * nb + b];
            const float p = dm * (float) tot;
            summs = summs + p;
        }
    }
    const float v = wk_hsum8(acc);
    return Q5 ? v + summs : v;
}

template <int EPI, int F>
__global__ __launch_bounds__(64) void k_kgemv_exact(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int16_t * __restrict__ xbs,
                                                    const int8_t * __restrict__ wq, const int8_t * __restrict__ wsc, const float * __restrict__ wd,
                                                    const float * __restrict__ wdm, int N, int K, wa_epi e) {
    const int tid = threadIdx.x, l = tid & 7;
    const int n = blockIdx.x * 8 + (tid >> 3);
    const int nn = n < N ? n : N - 1;
    wa_epi_pre pre;
    if (l == 0) pre = epi_preload<EPI>(e, 0, nn);
    const float v = wk_row_dot<F>(xq, xd, xbs, wq, wsc, wd, wdm, nn, K >> 8, l);
    if (l == 0 && n < N) epi_apply<EPI>(e, 0, n, v, pre);
}

// -------------------------------------------------------------------------------------------------
// C[M][N] = xq Wq^T, M > 1; grid = (ceil(N / 32), ceil(M / 8)); 256 threads = 32 output rows x 8 lanes; the 8 activation rows in LDS
// -------------------------------------------------------------------------------------------------
template <int EPI, int F>
__global__ __launch_bounds__(256) void k_kgemm_exact(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int16_t * __restrict__ xbs, int M,
                                                     const int8_t * __restrict__ wq, const int8_t * __restrict__ wsc, const float * __restrict__ wd,
                                                     const float * __restrict__ wdm, int N, int K, wa_epi e) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // xs int8 [8][K] (kernel layout) | xds f32 [8][K/256] | Q5: xgs i32 [8][K/256][8]
    constexpr bool Q5 = F == WK_Q5;                                            // | Q2: xgs = the rows' 16-element sums in pairs, i16 x 2 [8][K/256][8]
    const int nb = K >> 8;
    int8_t * xs = (int8_t *) smem;
    float * xds = (float *) (smem + (size_t) 8 * K);
    int * xgs = (int *) (xds + 8 * nb);
    const int tid = threadIdx.x, l = tid & 7;
    const int m0 = blockIdx.y * 8, mt = min(8, M - m0);
    for (int c = tid; c < 8 * (K >> 4); c += 256) {
        const int m = c / (K >> 4), cc = c - m * (K >> 4);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m < mt) v = *(const uint4 *) (xq + (size_t) (m0 + m) * K + cc * 16);
        *(uint4 *) (xs + (size_t) m * K + cc * 16) = v;
    }
    for (int c = tid; c < 8 * nb; c += 256) {
        const int m = c / nb, b = c - m * nb;
        xds[c] = m < mt ? xd[(size_t) (m0 + m) * nb + b] : 0.0f;
    }
    if (Q5)
        for (int c = tid; c < 8 * nb * 8; c += 256) {          // the sums of the 32-element groups: bsums[2 g] + bsums[2 g + 1]
            const int m = c / (nb * 8), r = c - m * (nb * 8);
            int s = 0;
            if (m < mt) { const int bs2 = *(const int *) (xbs + (size_t) (m0 + m) * nb * 16 + 2 * r); s = ((bs2 << 16) >> 16) + (bs2 >> 16); }
            xgs[c] = s;
        }
    if (F == WK_Q2)
        for (int c = tid; c < 8 * nb * 8; c += 256) {          // bsums[2 l] | bsums[2 l + 1] << 16, as they lie in memory
            const int m = c / (nb * 8), r = c - m * (nb * 8);
            xgs[c] = m < mt ? *(const int *) (xbs + (size_t) (m0 + m) * nb * 16 + 2 * r) : 0;
        }
    __syncthreads();
    const int n = blockIdx.x * 32 + (tid >> 3);
    const int nn = n < N ? n : N - 1;
    float acc[8];
    float summs = 0.0f;       // Q5: THIS lane runs the minimum chain of activation row m = l
#pragma unroll
    for (int m = 0; m < 8; ++m) acc[m] = 0.0f;
    wa_epi_pre pre[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) if (l == 0 && m < mt) pre[m] = epi_preload<EPI>(e, m0 + m, nn);
    const wk_i4 * wl = (const wk_i4 *) (wq + ((size_t) nn * 8 + l) * nb * 32);
    const int8_t * sl = wsc + (size_t) nn * nb * 16;
    const float * dl = wd + (size_t) nn * nb;
    const wk_i4 * xl = (const wk_i4 *) (xs + (size_t) l * nb * 32);
    for (int b = 0; b < nb; ++b) {
        const wk_i4 w0 = wl[2 * b], w1 = wl[2 * b + 1];
        const wk_i2 s = *(const wk_i2 *) (sl + 16 * b + (Q5 ? 0 : 8 * (l >> 2)));
        const float dw = dl[b];
        int ma = 0, mb = 0; float dwm = 0.0f;        // Q2: the minimums of this lane's sub-blocks 2 l and 2 l + 1, and the block's dmin
        if (F == WK_Q2) {
            const uint8_t * sb = (const uint8_t *) sl + 16 * b;
            ma = sb[l] >> 4; mb = sb[8 + l] >> 4; dwm = wdm[(size_t) nn * nb + b];
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const wk_i4 x0 = xl[(size_t) m * (K >> 4) + 2 * b], x1 = xl[(size_t) m * (K >> 4) + 2 * b + 1];
            const float dx = xds[m * nb + b];
            const float dd = dx * dw;
            if (F == WK_Q2) {                        // the lane owns acc[m] of every activation row: the minimum term first, then the product term
                const int bs2 = xgs[(m * nb + b) * 8 + l];
                const float dn = -dx * dwm;
                acc[m] = fmaf(dn, (float) (ma * ((bs2 << 16) >> 16) + mb * (bs2 >> 16)), acc[m]);
            }
            acc[m] = fmaf(dd, (float) wk_block<F>(w0, w1, x0, x1, s), acc[m]);
        }
        if (Q5) {
            const wk_i2 mm = *(const wk_i2 *) (sl + 16 * b + 8);
            const wk_i4 g0 = *(const wk_i4 *) (xgs + (l * nb + b) * 8), g1 = *(const wk_i4 *) (xgs + (l * nb + b) * 8 + 4);
            const int tot = wk_byte<WK_Q5>(mm, 0) * g0.x + wk_byte<WK_Q5>(mm, 1) * g0.y + wk_byte<WK_Q5>(mm, 2) * g0.z + wk_byte<WK_Q5>(mm, 3) * g0.w +
                            wk_byte<WK_Q5>(mm, 4) * g1.x + wk_byte<WK_Q5>(mm, 5) * g1.y + wk_byte<WK_Q5>(mm, 6) * g1.z + wk_byte<WK_Q5>(mm, 7) * g1.w;
            const float dm = -xds[l * nb + b] * wdm[(size_t) nn * nb + b];
            const float p = dm * (float) tot;
            summs = summs + p;
        }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        float v = wk_hsum8(acc[m]);
        if (Q5) v = v + wk_from_lane(summs, m);
        if (l == 0 && n < N && m < mt) epi_apply<EPI>(e, m0 + m, n, v, pre[m]);
    }
}

// one format's instantiations: M == 1 the one-row kernel, else the 8-row kernel with its LDS (the Q8_K rows; Q5_K, Q2_K: and their sums)
template <int F>
static void wk_launch(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq,
                      const int8_t * wsc, const float * wd, const float * wdm, int N, int K, const wa_epi & e) {
    const dim3 grid((N + 31) / 32, (M + 7) / 8);
    const size_t lds = (size_t) 8 * K + (size_t) 8 * (K >> 8) * sizeof(float) + (F != WK_Q6 ? (size_t) 8 * (K >> 8) * 8 * sizeof(int) : 0);
#define WA_CASE(E) case E: { \
        if (M == 1) { hipLaunchKernelGGL((k_kgemv_exact<E, F>), dim3((N + 7) / 8), dim3(64), 0, s, xq, xd, xbs, wq, wsc, wd, wdm, N, K, e); break; } \
        if (lds > 48 * 1024) (void) hipFuncSetAttribute((const void *) k_kgemm_exact<E, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); \
        hipLaunchKernelGGL((k_kgemm_exact<E, F>), grid, dim3(256), lds, s, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e); } break;
    switch (mode) {
        WA_CASE(WA_EPI_F16) WA_CASE(WA_EPI_ENC_QKV) WA_CASE(WA_EPI_GELU_F32) WA_CASE(WA_EPI_RESID) WA_CASE(WA_EPI_F32) WA_CASE(WA_EPI_CROSS_KV) WA_CASE(WA_EPI_DEC_QKV)
        default: break;
    }
#undef WA_CASE
}

#ifdef WA_QK_Q2_TU
void wa_launch_kgemm_q2(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq,
                        const int8_t * wsc, const float * wd, const float * wdm, int N, int K, const wa_epi & e) {
    wk_launch<WK_Q2>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);
}
#else
void wa_launch_kgemm_q2(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq,
                        const int8_t * wsc, const float * wd, const float * wdm, int N, int K, const wa_epi & e);      // wa_quantk_q2.o
void wa_launch_kgemm_exact(hipStream_t s, wa_epi_mode mode, int wtype, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq,
                           const int8_t * wsc, const float * wd, const float * wdm, int N, int K, const wa_epi & e) {
    if (wtype == 13) wk_launch<WK_Q5>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);
    else if (wtype == 10) wa_launch_kgemm_q2(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);
    else wk_launch<WK_Q6>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);        // Q6_K, and Q3_K as the loader unpacks it
}

// -------------------------------------------------------------------------------------------------
// ggml_get_rows on the quantised token embedding (dequantize_row_q6_K / q3_K: (d * sc) * q; dequantize_row_q5_K / q2_K: (d * sc) * q,
// then - (dmin * m): no fma) + positional embedding.  fmt: WK_Q6 (Q6_K, Q3_K), WK_Q5 or WK_Q2
// -------------------------------------------------------------------------------------------------
__global__ void k_dec_embed_k(const int32_t * __restrict__ tok, const int32_t * __restrict__ pos, int n_tokens, int d, int fmt,
                              const int8_t * __restrict__ wq, const int8_t * __restrict__ wsc, const float * __restrict__ wd, const float * __restrict__ wdm,
                              const float * __restrict__ pe, float * __restrict__ x) {
    const int j = blockIdx.x;
    const int t = tok[j], p = pos[j], nb = d >> 8;
    for (int i = threadIdx.x; i < d; i += blockDim.x) {
        const int b = i >> 8, el = i & 255;
        const int q = (int) wq[(((size_t) t * 8 + ((el & 31) >> 2)) * nb + b) * 32 + (el >> 5) * 4 + (el & 3)];
        const int8_t * sc = wsc + ((size_t) t * nb + b) * 16;
        const float db = wd[(size_t) t * nb + b];
        float v;
        if (fmt == WK_Q5) {
            const float d1 = db * (float) (int) (unsigned char) sc[el >> 5];
            const float m1 = wdm[(size_t) t * nb + b] * (float) (int) (unsigned char) sc[8 + (el >> 5)];
            const float tq = d1 * (float) q;
            v = tq - m1;
        } else if (fmt == WK_Q2) {
            const int sb = (int) (unsigned char) sc[8 * ((el >> 4) & 1) + (el >> 5)];
            const float d1 = db * (float) (sb & 15);
            const float m1 = wdm[(size_t) t * nb + b] * (float) (sb >> 4);
            const float tq = d1 * (float) q;
            v = tq - m1;
        } else {
            const float d1 = db * (float) (int) sc[8 * ((el >> 4) & 1) + (el >> 5)];
            v = d1 * (float) q;
        }
        x[(size_t) j * d + i] = v + pe[(size_t) p * d + i];
    }
}
void wa_launch_dec_embed_k(hipStream_t stream, int wtype, const int32_t * tok, const int32_t * pos, int n_tokens, int d, const int8_t * wq, const int8_t * wsc,
                           const float * wd, const float * wdm, const float * pe, float * x) {
    hipLaunchKernelGGL(k_dec_embed_k, dim3(n_tokens), dim3(256), 0, stream, tok, pos, n_tokens, d, wtype == 13 ? WK_Q5 : wtype == 10 ? WK_Q2 : WK_Q6, wq, wsc, wd, wdm, pe, x);
}
#endif

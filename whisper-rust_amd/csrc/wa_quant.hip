// wa_quant.hip - quantised weights (ggml Q5_0 / Q8_0 model files) in the reference's order.
//
// With a quantised weight matrix the reference CPU path quantises the F32 activation row to Q8_0 (quantize_row_q8_0,
// ggml-cpu/arch/x86/quants.c, AVX2: d = max|x| / 127, q = rint(x * (127 / max|x|)), d stored as F16) and forms every output as
//     acc[l] = fma( f32(d_w) * f32(d_x),  (float) sum_{e<4} w[4l+e] * x[4l+e],  acc[l] )        l = 0..7, block after block
//     out    = ((acc0 + acc4) + (acc2 + acc6)) + ((acc1 + acc5) + (acc3 + acc7))                  (hsum_float_8)
// (ggml_vec_dot_q5_0_q8_0 / ggml_vec_dot_q8_0_q8_0, same file; the integer sums are exact: |w| <= 16 or 127, |x| <= 127).
// Here: 8 lanes per output row, lane l owns elements 4l..4l+3 of every 32-element block (one v_dot4_i32_i8 per block and
// token), the three DPP exchanges reproduce hsum_float_8.  Up to 8 activation rows share one pass over the weights.
// The weights are stored for this access pattern at load (wa_loader.cpp: signed bytes, [row][lane][block][4]).
// Bit-identical to the reference engine on the Q5_0 / Q8_0 goldens (tests/test_parity_gpu.py).
// Products of more than 8 activation rows take the integer sums from the int8 matrix cores instead (k_qgemm_mfma below): same chains, same bits.
//
// Q4_1 / Q5_1 (template flag Q1; the arithmetic is stated in host code in wa_quant1.h): the quants are the unsigned 4- / 5-bit values
// (0..31 fits a signed byte, so the same v_dot4_i32_i8), the weight is q * d + m, and the reference multiplies with a Q8_1 row, whose
// blocks carry s = f16(d * sum q) besides d (quantize_row_q8_1).  Beside the lane chain above runs a SCALAR chain over the blocks,
//     summs = summs + (f32(m_w) * f32(s_x))        a multiplication, then an addition - not an fma
// and the output is hsum_float_8(acc) + summs (ggml_vec_dot_q4_1_q8_1 / q5_1_q8_1).  In the one-row product every lane of a row's group
// runs that chain redundantly (one v_mul + one v_add per block); with 8 activation rows lane l of the group runs the chain of activation
// row l and hands it to lane 0 over DPP.  The minimums wm [row][block] and the sums xs [row][block] are read like the scales.
#include "wa_device.h"
#include <cstdlib>

// -------------------------------------------------------------------------------------------------
// quantize_row_q8_0: one 32-lane half-wave per block.  The quants are written in the kernel layout of the weights
// ([row][l = 0..7][block][4], wa_internal.h: wa_lin): lane l of a dot product reads four blocks with one 16-byte load.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_quantize_q8_0(const float * __restrict__ x, int ldx, int rows, int K, int8_t * __restrict__ qs,
                                                       float * __restrict__ qd, float * __restrict__ qsum) {
    const int nb = K >> 5;
    const long g = (long) blockIdx.x * blockDim.x + threadIdx.x;
    const long gb = g >> 5;
    const int l = (int) (g & 31);
    if (gb >= (long) rows * nb) return;
    const int row = (int) (gb / nb), b = (int) (gb - (long) row * nb);
    wa_q8_store(x[(size_t) row * ldx + b * 32 + l], row, b, l, nb, qs, qd, qsum);
}
void wa_launch_quantize_q8_0(hipStream_t stream, const float * x, int ldx, int rows, int K, int8_t * qs, float * qd, float * qsum) {
    const long n = (long) rows * K;
    hipLaunchKernelGGL(k_quantize_q8_0, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream, x, ldx, rows, K, qs, qd, qsum);
}

typedef int   wq_i4 __attribute__((ext_vector_type(4)));
typedef float wq_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wq_hsum8(float v) {
    v = v + dpp_f32<0x104>(v);          // row_shl:4  acc[l] + acc[l+4]
    v = v + dpp_f32<0x102>(v);          // row_shl:2  (a0+a4)+(a2+a6) | (a1+a5)+(a3+a7)
    v = v + dpp_f32<0x101>(v);          // row_shl:1  the two halves
    return v;
}
#define WQ_BLOCK(acc, w, dw, x, dx) acc = fmaf((dw) * (dx), (float) __builtin_amdgcn_sdot4((w), (x), 0, false), acc)
#define WQ_STEP4(acc, W, DW, X, DX) do { WQ_BLOCK(acc, (W).x, (DW).x, (X).x, (DX).x); WQ_BLOCK(acc, (W).y, (DW).y, (X).y, (DX).y); \
                                         WQ_BLOCK(acc, (W).z, (DW).z, (X).z, (DX).z); WQ_BLOCK(acc, (W).w, (DW).w, (X).w, (DX).w); } while (0)
// the minimum chain of Q4_1 / Q5_1, four blocks in order: two roundings per block (the file is built with -ffp-contract=off)
#define WQ_MIN(sm, m, sx) do { const float wq_p = (m) * (sx); sm = sm + wq_p; } while (0)
#define WQ_MIN4(sm, M, SX) do { WQ_MIN(sm, (M).x, (SX).x); WQ_MIN(sm, (M).y, (SX).y); WQ_MIN(sm, (M).z, (SX).z); WQ_MIN(sm, (M).w, (SX).w); } while (0)
// lane 0 of an 8-lane group reads lane m's value (m = 0..7, a constant once the caller's loop is unrolled): row_shl:m
__device__ __forceinline__ float wq_from_lane(float v, int m) {
    switch (m) {
        case 1: return dpp_f32<0x101>(v); case 2: return dpp_f32<0x102>(v); case 3: return dpp_f32<0x103>(v); case 4: return dpp_f32<0x104>(v);
        case 5: return dpp_f32<0x105>(v); case 6: return dpp_f32<0x106>(v); case 7: return dpp_f32<0x107>(v); default: return v;
    }
}

// -------------------------------------------------------------------------------------------------
// C[M][N] = xq Wq^T, M > 1; grid = (ceil(N / 32), ceil(M / 8)); 256 threads = 32 output rows x 8 lanes; the 8 activation rows in LDS
// -------------------------------------------------------------------------------------------------
template <int EPI, bool Q1>
__global__ __launch_bounds__(256) void k_qgemm_exact(const int8_t * __restrict__ xq, const float * __restrict__ xd, int M, const int8_t * __restrict__ wq,
                                                     const float * __restrict__ wd, int N, int K, wa_epi e, const float * __restrict__ xsum,
                                                     const float * __restrict__ wm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // xs int8 [8][K] (kernel layout) | xds f32 [8][K/32] | Q1: xss f32 [8][K/32]
    const int nb = K >> 5;
    int8_t * xs = (int8_t *) smem;
    float * xds = (float *) (smem + (size_t) 8 * K);
    float * xss = xds + 8 * nb;
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
        if (Q1) xss[c] = m < mt ? xsum[(size_t) (m0 + m) * nb + b] : 0.0f;
    }
    __syncthreads();
    const int n = blockIdx.x * 32 + (tid >> 3);
    const int nn = n < N ? n : N - 1;
    float acc[8];
    float summs = 0.0f;       // Q1: THIS lane runs the minimum chain of activation row m = l
#pragma unroll
    for (int m = 0; m < 8; ++m) acc[m] = 0.0f;
    wa_epi_pre pre[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) if (l == 0 && m < mt) pre[m] = epi_preload<EPI>(e, m0 + m, nn);
    const int * wl = (const int *) wq + ((size_t) nn * 8 + l) * nb;            // this lane's quads, block after block
    const float * dl = wd + (size_t) nn * nb;
    const int * xl = (const int *) xs + (size_t) l * nb;
    const float * ml = Q1 ? wm + (size_t) nn * nb : dl;
    const float * sxl = xss + l * nb;
    if ((nb & 3) == 0) {
        wq_i4 wn = *(const wq_i4 *) wl; wq_f4 dn = *(const wq_f4 *) dl; wq_f4 mn = dn;
        if (Q1) mn = *(const wq_f4 *) ml;
        for (int b = 0; b < nb; b += 4) {
            const wq_i4 w = wn; const wq_f4 dw = dn; const wq_f4 mw = mn;
            const int bn = min(b + 4, nb - 4);
            wn = *(const wq_i4 *) (wl + bn); dn = *(const wq_f4 *) (dl + bn);
            if (Q1) mn = *(const wq_f4 *) (ml + bn);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const wq_i4 x = *(const wq_i4 *) (xl + (size_t) m * (K >> 2) + b);
                const wq_f4 dx = *(const wq_f4 *) (xds + m * nb + b);
                WQ_STEP4(acc[m], w, dw, x, dx);
            }
            if (Q1) { const wq_f4 sx = *(const wq_f4 *) (sxl + b); WQ_MIN4(summs, mw, sx); }
        }
    } else {
        for (int b = 0; b < nb; ++b) {
            const int w = wl[b]; const float dw = dl[b];
#pragma unroll
            for (int m = 0; m < 8; ++m) WQ_BLOCK(acc[m], w, dw, xl[(size_t) m * (K >> 2) + b], xds[m * nb + b]);
            if (Q1) WQ_MIN(summs, ml[b], sxl[b]);
        }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        float v = wq_hsum8(acc[m]);
        if (Q1) v = v + wq_from_lane(summs, m);
        if (l == 0 && n < N && m < mt) epi_apply<EPI>(e, m0 + m, n, v, pre[m]);
    }
}

// -------------------------------------------------------------------------------------------------
// The same product on the int8 matrix cores, M > 8.  v_mfma_i32_16x16x4_4b_i8 computes FOUR independent 16 x 16 products with K = 4 bytes; its
// operand and result mapping, confirmed on the MI355X by tools/micro/mfma_i8_blocks.hip (one-hot rows, random bytes, one-hot K-bytes):
//     A: lane L holds the four K-bytes of block L / 16, row L % 16          B: lane L holds the four K-bytes of block L / 16, column L % 16
//     D: register 4 blk + r of lane L is block blk, row 4 (L / 16) + r, column L % 16
// Here block = lane-sum index: the int at ((const int *) q)[(row * 8 + l) * nb + b] of the kernel layout IS one operand, rows = activation rows,
// columns = weight rows, and two instructions (l = 0..3, l = 4..7) give all eight integer lane sums of a 16 x 16 output tile for one quant block -
// exact, as any integer order is.  Every lane then holds, for its column and its rows, the eight sums of the reference's eight AVX2 lanes:
// f32(dw) * f32(dx) is rounded once per (row, column, block), the eight chains acc[l] = fma(dw dx, (float) sum_l, acc[l]) run block after block, and
// hsum_float_8 is lane-local (no DPP).  Q1: the lane runs the minimum chains of its (row, column) pairs.  Bit-identical to k_qgemm_exact.
// Two forms of one body (RS = result rows a lane works on), 256 threads each:
//   RS = 4  grid (ceil(N / 64), ceil(M / 16)): the 4 waves are 4 column tiles of one row tile, every lane keeps all four rows the instruction
//           gives it (32 chains) - the fewest VALU operations per output; for grids that fill the chip (the encoder).
//   RS = 1  grid (ceil(N / 16), ceil(M / 16)): the 4 waves share ONE tile; wave w feeds the instruction the rows 4 i + w in the places 4 i .. 4 i + 3,
//           so its register r = 0 holds row 4 (L / 16) + w, and works on that row only (8 chains; the other registers repeat it and are not
//           read).  The integer work is done four times over in the otherwise idle matrix pipe; the VALU chain of a wave - which is what a
//           prompt pass of a few row tiles waits for - is a quarter as long.
// The row tile's scales (and Q8_1 block sums) are staged in LDS once - the kernel's only barrier; the quants come straight from global memory / L2
// (the 4 waves' common operand rows meet in the vector cache), the next four blocks' loads in flight while the current four are worked on.
// Nothing waits for another workgroup.  Rows beyond M and columns beyond N read the last valid row / column and store nothing.
// -------------------------------------------------------------------------------------------------
typedef int wq_i16 __attribute__((ext_vector_type(16)));

// one quant block of the tile: s0 / s1 = the lane sums l = 0..3 / 4..7 (register 4 t + r: l = t (+ 4), row r of the lane's)
#define WQ_MFMA_BLOCK(acc, summs, A0, A1, B0, B1, DW, DX, MW, SX) do { \
        const wq_i16 wq_z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
        const wq_i16 s0 = __builtin_amdgcn_mfma_i32_16x16x4i8((A0), (B0), wq_z, 0, 0, 0); \
        const wq_i16 s1 = __builtin_amdgcn_mfma_i32_16x16x4i8((A1), (B1), wq_z, 0, 0, 0); \
        _Pragma("unroll") for (int r = 0; r < RS; ++r) { \
            const float wq_p = (DW) * (DX)[r]; \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) { \
                acc[r][t]     = fmaf(wq_p, (float) s0[4 * t + r], acc[r][t]); \
                acc[r][4 + t] = fmaf(wq_p, (float) s1[4 * t + r], acc[r][4 + t]); \
            } \
            if (Q1) WQ_MIN(summs[r], (MW), (SX)[r]); \
        } } while (0)

template <int EPI, bool Q1, int RS>
__global__ __launch_bounds__(256, RS == 1 ? 4 : Q1 ? 2 : 3) void k_qgemm_mfma(const int8_t * __restrict__ xq, const float * __restrict__ xd, int M,
                                                                              const int8_t * __restrict__ wq, const float * __restrict__ wd, int N, int K, wa_epi e,
                                                                              const float * __restrict__ xsum, const float * __restrict__ wm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // the row tile's scales xds f32 [16][K/32] | Q1: its block sums xss f32 [16][K/32]
    const int nb = K >> 5;
    float * xds = (float *) smem, * xss = xds + 16 * nb;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 16, n0 = (RS == 4 ? blockIdx.x * 4 + wv : blockIdx.x) * 16;
    for (int i = threadIdx.x; i < 16 * nb; i += 256) {
        const int r = i / nb, b = i - r * nb;
        const size_t src = (size_t) min(m0 + r, M - 1) * nb + b;
        xds[i] = xd[src];
        if (Q1) xss[i] = xsum[src];
    }
    __syncthreads();                                       // the kernel's only barrier, before any wave leaves
    if (n0 >= N) return;                                   // (a whole wave)
    const int n = n0 + c, nn = n < N ? n : N - 1;
    const int ma = min(RS == 4 ? m0 + c : m0 + (c & ~3) + wv, M - 1);         // the activation row whose bytes this lane feeds
    const int r0 = RS == 4 ? 4 * g : 4 * g + wv;                                // the tile rows r0 .. r0 + RS - 1 are this lane's results
    wa_epi_pre pre[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) pre[r] = epi_preload<EPI>(e, min(m0 + r0 + r, M - 1), nn);
    // 32-bit element offsets from the (uniform) array bases: the launcher sends no product here whose arrays they could not index
    const unsigned xo = ((unsigned) ma * 8 + g) * nb, wo = ((unsigned) nn * 8 + g) * nb, h = 4 * (unsigned) nb;      // l = g; l = 4 + g: + h
    const unsigned so = (unsigned) nn * nb;
    const int * xi = (const int *) xq, * wi = (const int *) wq;
    const float * wmn = Q1 ? wm : wd;
    const float * dxl = xds + r0 * nb, * sxl = Q1 ? xss + r0 * nb : dxl;          // the lane's rows in LDS: row r at + r nb
    float acc[RS][8], summs[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        summs[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[r][t] = 0.0f;
    }
    if ((nb & 3) == 0) {
        wq_i4 a0n = *(const wq_i4 *) (xi + xo), a1n = *(const wq_i4 *) (xi + xo + h), b0n = *(const wq_i4 *) (wi + wo), b1n = *(const wq_i4 *) (wi + wo + h);
        wq_f4 dn = *(const wq_f4 *) (wd + so), mn = dn;
        if (Q1) mn = *(const wq_f4 *) (wmn + so);
        for (int b = 0; b < nb; b += 4) {
            const wq_i4 a0 = a0n, a1 = a1n, b0 = b0n, b1 = b1n; const wq_f4 dw = dn, mw = mn;
            const unsigned bn = (unsigned) min(b + 4, nb - 4);
            a0n = *(const wq_i4 *) (xi + xo + bn); a1n = *(const wq_i4 *) (xi + xo + h + bn);
            b0n = *(const wq_i4 *) (wi + wo + bn); b1n = *(const wq_i4 *) (wi + wo + h + bn);
            dn = *(const wq_f4 *) (wd + so + bn);
            if (Q1) mn = *(const wq_f4 *) (wmn + so + bn);
            wq_f4 dx4[RS], sx4[RS];
#pragma unroll
            for (int r = 0; r < RS; ++r) { dx4[r] = *(const wq_f4 *) (dxl + r * nb + b); sx4[r] = dx4[r]; if (Q1) sx4[r] = *(const wq_f4 *) (sxl + r * nb + b); }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float dx[RS], sx[RS];
#pragma unroll
                for (int r = 0; r < RS; ++r) { dx[r] = dx4[r][j]; sx[r] = sx4[r][j]; }
                WQ_MFMA_BLOCK(acc, summs, a0[j], a1[j], b0[j], b1[j], dw[j], dx, mw[j], sx);
            }
        }
    } else {
        for (int b = 0; b < nb; ++b) {
            float dx[RS], sx[RS];
#pragma unroll
            for (int r = 0; r < RS; ++r) { dx[r] = dxl[r * nb + b]; sx[r] = sxl[r * nb + b]; }
            WQ_MFMA_BLOCK(acc, summs, xi[xo + b], xi[xo + h + b], wi[wo + b], wi[wo + h + b], wd[so + b], dx, wmn[so + b], sx);
        }
    }
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        float v = ((acc[r][0] + acc[r][4]) + (acc[r][2] + acc[r][6])) + ((acc[r][1] + acc[r][5]) + (acc[r][3] + acc[r][7]));       // hsum_float_8
        if (Q1) v = v + summs[r];
        if (n < N && m0 + r0 + r < M) epi_apply<EPI>(e, m0 + r0 + r, n, v, pre[r]);
    }
}

// -------------------------------------------------------------------------------------------------
// M == 1 (the decode step): grid = ceil(N / 8) single-wave workgroups, 8 output rows x 8 lanes each; no LDS, the activation row is
// read from L2 with the same 16-byte pattern as the weights; 16 blocks (4 loads of each kind) in flight ahead of the arithmetic
// -------------------------------------------------------------------------------------------------
// one output row per 8 lanes: the row's dot product with the activation row (valid in lane l == 0 of the group)
template <bool Q1>
__device__ __forceinline__ float wq_row_dot(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int8_t * __restrict__ wq,
                                            const float * __restrict__ wd, int nn, int nb, int l, const float * __restrict__ xsum,
                                            const float * __restrict__ wm) {
    const int * wl = (const int *) wq + ((size_t) nn * 8 + l) * nb;
    const float * dl = wd + (size_t) nn * nb;
    const int * xl = (const int *) xq + (size_t) l * nb;
    const float * ml = Q1 ? wm + (size_t) nn * nb : dl;
    const float * sl = Q1 ? xsum : xd;
    float acc = 0.0f, summs = 0.0f;
    if ((nb & 3) == 0) {
        wq_i4 wn[4], xn[4]; wq_f4 dn[4], en[4], mn[4], sn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int bj = min(4 * j, nb - 4);
            wn[j] = *(const wq_i4 *) (wl + bj); dn[j] = *(const wq_f4 *) (dl + bj); xn[j] = *(const wq_i4 *) (xl + bj); en[j] = *(const wq_f4 *) (xd + bj);
            if (Q1) { mn[j] = *(const wq_f4 *) (ml + bj); sn[j] = *(const wq_f4 *) (sl + bj); }
        }
        for (int b = 0; b < nb; b += 16) {
            wq_i4 w[4], x[4]; wq_f4 dw[4], dx[4], mw[4], sx[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { w[j] = wn[j]; x[j] = xn[j]; dw[j] = dn[j]; dx[j] = en[j]; if (Q1) { mw[j] = mn[j]; sx[j] = sn[j]; } }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int bj = min(b + 16 + 4 * j, nb - 4);
                wn[j] = *(const wq_i4 *) (wl + bj); dn[j] = *(const wq_f4 *) (dl + bj); xn[j] = *(const wq_i4 *) (xl + bj); en[j] = *(const wq_f4 *) (xd + bj);
                if (Q1) { mn[j] = *(const wq_f4 *) (ml + bj); sn[j] = *(const wq_f4 *) (sl + bj); }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) if (b + 4 * j < nb) { WQ_STEP4(acc, w[j], dw[j], x[j], dx[j]); if (Q1) WQ_MIN4(summs, mw[j], sx[j]); }
        }
    } else {
        for (int b = 0; b < nb; ++b) { WQ_BLOCK(acc, wl[b], dl[b], xl[b], xd[b]); if (Q1) WQ_MIN(summs, ml[b], sl[b]); }
    }
    const float v = wq_hsum8(acc);
    return Q1 ? v + summs : v;
}

template <int EPI, bool Q1>
__global__ __launch_bounds__(64) void k_qgemv_exact(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int8_t * __restrict__ wq,
                                                    const float * __restrict__ wd, int N, int K, wa_epi e, const float * __restrict__ xsum,
                                                    const float * __restrict__ wm) {
    const int tid = threadIdx.x, l = tid & 7;
    const int n = blockIdx.x * 8 + (tid >> 3);
    const int nn = n < N ? n : N - 1;
    wa_epi_pre pre;
    if (l == 0) pre = epi_preload<EPI>(e, 0, nn);
    const float v = wq_row_dot<Q1>(xq, xd, wq, wd, nn, K >> 5, l, xsum, wm);
    if (l == 0 && n < N) epi_apply<EPI>(e, 0, n, v, pre);
}

// -------------------------------------------------------------------------------------------------
// M = R = 2..8 (a beam / best_of step, a small batch): the one-row kernel's shape - grid = ceil(N / 8) single-wave workgroups, 8 output
// rows x 8 lanes, no LDS, 16 blocks of weight loads in flight - with R accumulators: the lane's weight quads and scales are loaded ONCE per four
// blocks and meet the R activation rows, which every wave reads from L2 with the same 16-byte pattern (R K bytes, shared by all workgroups).
// Per (activation row, output) the arithmetic is WQ_BLOCK / WQ_MIN block after block, as in k_qgemm_exact: the results are the same bits.
// Against k_qgemm_exact (32 output rows per workgroup, one load group in flight) a narrow matrix gets 4 x the workgroups: N = 768 -> 96, not 24.
// With a minimum, lane l of an output row's group runs the chain of activation row min(l, R - 1) and hands it to lane 0 (as k_qgemm_exact).
// -------------------------------------------------------------------------------------------------
template <int EPI, bool Q1, int R>
__global__ __launch_bounds__(64) void k_qgemv_rows(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int8_t * __restrict__ wq,
                                                   const float * __restrict__ wd, int N, int K, wa_epi e, const float * __restrict__ xsum,
                                                   const float * __restrict__ wm) {
    const int tid = threadIdx.x, l = tid & 7, nb = K >> 5;
    const int n = blockIdx.x * 8 + (tid >> 3);
    const int nn = n < N ? n : N - 1;
    wa_epi_pre pre[R];
#pragma unroll
    for (int r = 0; r < R; ++r) if (l == 0) pre[r] = epi_preload<EPI>(e, r, nn);
    const int * wl = (const int *) wq + ((size_t) nn * 8 + l) * nb;
    const float * dl = wd + (size_t) nn * nb;
    const int * xl = (const int *) xq + (size_t) l * nb;            // row r: + r * (K >> 2)
    const float * ml = Q1 ? wm + (size_t) nn * nb : dl;
    const float * sl = Q1 ? xsum + (size_t) (l < R ? l : R - 1) * nb : xd;
    float acc[R];
    float summs = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
    if ((nb & 3) == 0) {
        wq_i4 wn[4]; wq_f4 dn[4], mn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int bj = min(4 * j, nb - 4);
            wn[j] = *(const wq_i4 *) (wl + bj); dn[j] = *(const wq_f4 *) (dl + bj);
            if (Q1) mn[j] = *(const wq_f4 *) (ml + bj);
        }
        for (int b = 0; b < nb; b += 16) {
            wq_i4 w[4]; wq_f4 dw[4], mw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { w[j] = wn[j]; dw[j] = dn[j]; if (Q1) mw[j] = mn[j]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int bj = min(b + 16 + 4 * j, nb - 4);
                wn[j] = *(const wq_i4 *) (wl + bj); dn[j] = *(const wq_f4 *) (dl + bj);
                if (Q1) mn[j] = *(const wq_f4 *) (ml + bj);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int bj = min(b + 4 * j, nb - 4);                 // (clamped: the loads of a round's four groups go out together, whatever the guard below says)
                wq_i4 x[R]; wq_f4 dx[R], sx;
#pragma unroll
                for (int r = 0; r < R; ++r) { x[r] = *(const wq_i4 *) (xl + (size_t) r * (K >> 2) + bj); dx[r] = *(const wq_f4 *) (xd + (size_t) r * nb + bj); }
                if (Q1) sx = *(const wq_f4 *) (sl + bj);
                if (b + 4 * j < nb) {
#pragma unroll
                    for (int r = 0; r < R; ++r) WQ_STEP4(acc[r], w[j], dw[j], x[r], dx[r]);
                    if (Q1) WQ_MIN4(summs, mw[j], sx);
                }
            }
        }
    } else {
        for (int b = 0; b < nb; ++b) {
            const int w = wl[b]; const float dw = dl[b];
#pragma unroll
            for (int r = 0; r < R; ++r) WQ_BLOCK(acc[r], w, dw, xl[(size_t) r * (K >> 2) + b], xd[(size_t) r * nb + b]);
            if (Q1) WQ_MIN(summs, ml[b], sl[b]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float v = wq_hsum8(acc[r]);
        if (Q1) v = v + wq_from_lane(summs, r);
        if (l == 0 && n < N) epi_apply<EPI>(e, r, n, v, pre[r]);
    }
}

// the first MLP product of the decode step: 4 waves = 32 output rows = one Q8_0 block of the GELU output (N % 32 == 0)
template <bool Q1>
__global__ __launch_bounds__(256) void k_qgemv_gelu_q8(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int8_t * __restrict__ wq,
                                                       const float * __restrict__ wd, int N, int K, const float * __restrict__ bias,
                                                       const wa_f16 * __restrict__ gelu, int8_t * __restrict__ oq, float * __restrict__ oqd,
                                                       const float * __restrict__ xsum, const float * __restrict__ wm, float * __restrict__ oqs) {
    __shared__ float g[32];
    const int tid = threadIdx.x, l = tid & 7;
    const int n = blockIdx.x * 32 + (tid >> 3);
    const float bn = l == 0 ? bias[n] : 0.0f;
    const float v = wq_row_dot<Q1>(xq, xd, wq, wd, n, K >> 5, l, xsum, wm);
    if (l == 0) g[tid >> 3] = wa_gelu(v + bn, gelu);
    __syncthreads();
    if (tid < 32) wa_q8_store(g[tid], 0, blockIdx.x, tid, N >> 5, oq, oqd, Q1 ? oqs : nullptr);
}
void wa_launch_qgemv_gelu_q8(hipStream_t s, const int8_t * xq, const float * xd, const int8_t * wq, const float * wd, int N, int K, const float * bias,
                             const wa_f16 * gelu, int8_t * oq, float * oqd, const float * xs, const float * wm, float * oqs) {
    if (wm) hipLaunchKernelGGL(k_qgemv_gelu_q8<true>, dim3(N / 32), dim3(256), 0, s, xq, xd, wq, wd, N, K, bias, gelu, oq, oqd, xs, wm, oqs);
    else    hipLaunchKernelGGL(k_qgemv_gelu_q8<false>, dim3(N / 32), dim3(256), 0, s, xq, xd, wq, wd, N, K, bias, gelu, oq, oqd, xs, wm, oqs);
}

// The default rule: every product of 2..8 rows goes to the few-rows kernel.  Measured on the MI355X (M = 5 and 8 at d = 768 and 1280, the logits
// product at d = 768 with 5 rows) it is the faster one for every product timed; the other row counts and widths follow those points unmeasured.
// WHISPER_AMD_NO_FEW_ROWS=1 (read once per process) goes back.
static bool few_rows_rule(int M) {
    static const bool off = getenv("WHISPER_AMD_NO_FEW_ROWS") != nullptr;
    return !off && M >= 2 && M <= 8;
}
// The matrix-core rule: every product of more than 8 rows whose rows belong to one state.  Measured on the MI355X k_qgemm_mfma is the
// faster one for every shape class timed.  WHISPER_AMD_NO_QMFMA=1 (read once per process) goes back to k_qgemm_exact.
static bool qmfma_rule(int M, int N, int K) {
    static const bool off = getenv("WHISPER_AMD_NO_QMFMA") != nullptr;
    (void) N; (void) K;
    return !off && M >= 9;
}
// the kernel a route gives a product: 1 k_qgemm_exact (k_qgemv_exact for M == 1), 2 k_qgemv_rows, 3 k_qgemm_mfma
int wa_qgemm_exact_kernel(wa_epi_mode mode, int M, int N, int K, const wa_epi & e, int route) {
    const bool few_mode = mode == WA_EPI_F16 || mode == WA_EPI_GELU_F32 || mode == WA_EPI_RESID || mode == WA_EPI_F32 || mode == WA_EPI_DEC_QKV;
    if (M >= 2 && M <= 8 && few_mode && route != 1 && (route == 2 || few_rows_rule(M))) return 2;       // (route 3 below 9 rows: the rule's kernel)
    const bool idx32 = (long long) (M > N ? M : N) * K < (1ll << 33);         // k_qgemm_mfma indexes the quants by 32-bit int offsets
    if (M >= 9 && !e.rowp && idx32 && route != 1 && route != 2 && (route == 3 || qmfma_rule(M, N, K))) return 3;
    return 1;
}
// route 0: the rules above pick the kernel; 1: k_qgemm_exact (k_qgemv_exact for M == 1) whatever they say; 2: k_qgemv_rows wherever it exists (M = 2..8, the
// epilogues of the decoder); 3: k_qgemm_mfma wherever it applies (M >= 9, no rowp) - the kernel tests compare them
void wa_launch_qgemm_exact_route(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, int M, const int8_t * wq, const float * wd, int N, int K,
                                 const wa_epi & e, const float * xs, const float * wm, int route) {
    const int kernel = wa_qgemm_exact_kernel(mode, M, N, K, e, route);
    if (kernel == 3) {
        // the form with four rows per lane where its 64-column workgroups still give every CU two of them (the encoder); the one-row form for the
        // few row tiles of a prompt pass, which would leave most of the chip idle otherwise and wait for long single waves
        const bool wide = (long) ((N + 63) / 64) * ((M + 15) / 16) >= 512;
        const dim3 grid(wide ? (N + 63) / 64 : (N + 15) / 16, (M + 15) / 16);
        const size_t lds = (size_t) (wm ? 32 : 16) * (K >> 5) * sizeof(float);           // <= 20 KiB at K = 5120
#define WA_MFMA_L(E, Q1, RS) hipLaunchKernelGGL((k_qgemm_mfma<E, Q1, RS>), grid, dim3(256), lds, s, xq, xd, M, wq, wd, N, K, e, xs, wm)
#define WA_CASE(E) case E: if (wm) { if (wide) WA_MFMA_L(E, true, 4); else WA_MFMA_L(E, true, 1); } \
                           else    { if (wide) WA_MFMA_L(E, false, 4); else WA_MFMA_L(E, false, 1); } \
                           break;
        switch (mode) {
            WA_CASE(WA_EPI_F16) WA_CASE(WA_EPI_ENC_QKV) WA_CASE(WA_EPI_GELU_F32) WA_CASE(WA_EPI_RESID) WA_CASE(WA_EPI_F32) WA_CASE(WA_EPI_CROSS_KV) WA_CASE(WA_EPI_DEC_QKV)
            default: break;
        }
#undef WA_CASE
#undef WA_MFMA_L
        return;
    }
    const bool few = kernel == 2;
    if (few) {
#define WA_ROWS_R(E, Q1, R) case R: hipLaunchKernelGGL((k_qgemv_rows<E, Q1, R>), dim3((N + 7) / 8), dim3(64), 0, s, xq, xd, wq, wd, N, K, e, xs, wm); return;
#define WA_ROWS_Q(E, Q1) switch (M) { WA_ROWS_R(E, Q1, 2) WA_ROWS_R(E, Q1, 3) WA_ROWS_R(E, Q1, 4) WA_ROWS_R(E, Q1, 5) WA_ROWS_R(E, Q1, 6) WA_ROWS_R(E, Q1, 7) WA_ROWS_R(E, Q1, 8) default: break; }
#define WA_ROWS_E(E) case E: if (wm) WA_ROWS_Q(E, true) else WA_ROWS_Q(E, false) break;
        switch (mode) {        // (the encoder's epilogues never see so few rows: they stay with k_qgemm_exact)
            WA_ROWS_E(WA_EPI_F16) WA_ROWS_E(WA_EPI_GELU_F32) WA_ROWS_E(WA_EPI_RESID) WA_ROWS_E(WA_EPI_F32) WA_ROWS_E(WA_EPI_DEC_QKV)
            default: break;
        }
#undef WA_ROWS_E
#undef WA_ROWS_Q
#undef WA_ROWS_R
    }
    const dim3 grid((N + 31) / 32, (M + 7) / 8);
    const size_t lds = (size_t) 8 * K + (size_t) (wm ? 16 : 8) * (K >> 5) * sizeof(float);
#define WA_CASE_Q(E, Q1) { \
        if (M == 1) { hipLaunchKernelGGL((k_qgemv_exact<E, Q1>), dim3((N + 7) / 8), dim3(64), 0, s, xq, xd, wq, wd, N, K, e, xs, wm); break; } \
        if (lds > 48 * 1024) (void) hipFuncSetAttribute((const void *) k_qgemm_exact<E, Q1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); \
        hipLaunchKernelGGL((k_qgemm_exact<E, Q1>), grid, dim3(256), lds, s, xq, xd, M, wq, wd, N, K, e, xs, wm); }
#define WA_CASE(E) case E: if (wm) WA_CASE_Q(E, true) else WA_CASE_Q(E, false) break;
    switch (mode) {
        WA_CASE(WA_EPI_F16) WA_CASE(WA_EPI_ENC_QKV) WA_CASE(WA_EPI_GELU_F32) WA_CASE(WA_EPI_RESID) WA_CASE(WA_EPI_F32) WA_CASE(WA_EPI_CROSS_KV) WA_CASE(WA_EPI_DEC_QKV)
        default: break;
    }
#undef WA_CASE
#undef WA_CASE_Q
}
void wa_launch_qgemm_exact(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, int M, const int8_t * wq, const float * wd, int N, int K,
                           const wa_epi & e, const float * xs, const float * wm) {
    wa_launch_qgemm_exact_route(s, mode, xq, xd, M, wq, wd, N, K, e, xs, wm, 0);
}

// -------------------------------------------------------------------------------------------------
// ggml_get_rows on the quantised token embedding (dequantize_row_q5_0 / q8_0, ggml-quants.c: q * d; dequantize_row_q4_1 / q5_1 with
// wm set: q * d, then + m - two roundings) + positional embedding
// -------------------------------------------------------------------------------------------------
__global__ void k_dec_embed_q(const int32_t * __restrict__ tok, const int32_t * __restrict__ pos, int n_tokens, int d,
                              const int8_t * __restrict__ wq, const float * __restrict__ wd, const float * __restrict__ pe, float * __restrict__ x,
                              const float * __restrict__ wm) {
    const int j = blockIdx.x;
    const int t = tok[j], p = pos[j], nb = d >> 5;
    for (int i = threadIdx.x; i < d; i += blockDim.x) {
        const int b = i >> 5, el = i & 31;
        const int q = (int) wq[(((size_t) t * 8 + (el >> 2)) * nb + b) * 4 + (el & 3)];
        float v = (float) q * wd[(size_t) t * nb + b];
        if (wm) v = v + wm[(size_t) t * nb + b];
        x[(size_t) j * d + i] = v + pe[(size_t) p * d + i];
    }
}
void wa_launch_dec_embed_q(hipStream_t stream, const int32_t * tok, const int32_t * pos, int n_tokens, int d, const int8_t * wq, const float * wd,
                           const float * pe, float * x, const float * wm) {
    hipLaunchKernelGGL(k_dec_embed_q, dim3(n_tokens), dim3(256), 0, stream, tok, pos, n_tokens, d, wq, wd, pe, x, wm);
}

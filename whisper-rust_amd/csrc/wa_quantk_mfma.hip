// wa_quantk_mfma.hip - the K-format products (Q2_K / Q3_K / Q5_K / Q6_K weights x Q8_K rows, wa_quantk.hip) of more than 8 activation rows on the int8
// matrix cores, and the launcher that picks between this kernel and the general ones.  A code object of its own (build/wa_quantk_mfma.o).
//
// v_mfma_i32_16x16x4_4b_i8 computes FOUR independent 16 x 16 products with K = 4 bytes (the map was pinned on the MI355X by
// tools/micro/mfma_i8_blocks.hip and is the one k_qgemm_mfma of wa_quant.hip uses):
//     A: lane L holds the four K-bytes of slot L / 16, row L % 16          B: lane L holds the four K-bytes of slot L / 16, column L % 16
//     D: register 4 slot + r of lane L is slot, row 4 (L / 16) + r, column L % 16
// Rows = activation rows, columns = weight rows, slot = lane-sum index within a half: l = 4 h + slot.  The int at ((row * 8 + l) * nb + b) * 8 + g of the
// kernel layout (int8 [row][l][block b][group g][4]) IS one operand, so one instruction per (b, g, h) with C = 0 gives the sixteen 4-element dot
// products of that group for a lane's column; each is multiplied by the sub-block scale - sc[8 h + g] of the lane's column (Q6_K, Q3_K, Q2_K: the low
// nibble) or sc[g] (Q5_K): ONE scale per lane and instruction - and added to the lane's integer lane sums (|dot4| <= 16 256, |scale| <= 128: a 24-bit
// multiply-add).  Integer sums are exact in any order; everything behind them is k_kgemm_exact's, per (row, column, block):
//     dd = dx * dw, rounded once;   Q2_K first: acc[l] = fma(-dx * dmin, (float) (m[2 l] bsums[2 l] + m[2 l + 1] bsums[2 l + 1]), acc[l]);
//     acc[l] = fma(dd, (float) t_l, acc[l]), l = 0..7;   Q5_K: summs = summs + ((-dx * dmin) * (float) sum_g m[g] (bsums[2 g] + bsums[2 g + 1]))
// and at the row's end hsum_float_8 in wk_hsum8's order - lane-local, no DPP - (+ summs, Q5_K), then the epilogue.  Bit-identical to k_kgemm_exact.
// Two forms of one body (RS = result rows a lane works on), 256 threads each, as k_qgemm_mfma:
//   RS = 4  grid (ceil(N / 64), ceil(M / 16)): the 4 waves are 4 column tiles of one row tile; a lane keeps the four rows the instruction gives it.
//           Taken from 128 such workgroups on (kmfma_wide below).
//   RS = 1  grid (ceil(N / 16), ceil(M / 16)): the 4 waves share ONE tile; wave w feeds the instruction the rows 4 i + w in the places 4 i .. 4 i + 3,
//           so its register r = 0 holds row 4 (L / 16) + w and it works on that row only - a quarter of the VALU chain, for the few tiles of a prompt pass.
// Staged in LDS once, behind the kernel's only barrier: the tile's dx, dw (dmin), the columns' scale bytes, Q5_K's group sums / Q2_K's bsums pairs.  The
// quants come straight from global memory / L2, the next block's loads in flight.  Rows beyond M and columns beyond N read the last valid one and store
// nothing.  Nothing waits for another workgroup.  Every offset into the quants is 64-bit.
#include "wa_quantk_dev.h"
#include <stdlib.h>

typedef int wk_i16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int wk_ubyte(wk_i2 s, int g) { return (int) (((unsigned) (g < 4 ? s.x : s.y) >> (8 * (g & 3))) & 0xffu); }

template <int EPI, int F, int RS>
__global__ __launch_bounds__(256, RS == 4 ? 2 : 3) void k_kgemm_mfma(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int16_t * __restrict__ xbs, int M,
                                                    const int8_t * __restrict__ wq, const int8_t * __restrict__ wsc, const float * __restrict__ wd,
                                                    const float * __restrict__ wdm, int N, int K, wa_epi e) {
    // scs i8 [CT][nb][16] | dws f32 [CT][nb] | MIN: dms f32 [CT][nb] | xds f32 [16][nb] | MIN: xgs i32 [16][nb][8]  (every part a multiple of 16 bytes)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool Q5 = F == WK_Q5, Q2 = F == WK_Q2, MIN = Q5 || Q2;
    constexpr int CT = RS == 4 ? 64 : 16;                      // the workgroup's columns
    const int nb = K >> 8;
    wk_i2 * scs = (wk_i2 *) smem;
    float * dws = (float *) (smem + (size_t) CT * nb * 16);
    float * dms = dws + (MIN ? CT * nb : 0);
    float * xds = dms + CT * nb;
    int * xgs = (int *) (xds + 16 * nb);
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 16, nc0 = blockIdx.x * CT;
    for (int i = threadIdx.x; i < CT * nb; i += 256) {
        const int ct = i / nb, b = i - ct * nb;
        const size_t src = (size_t) min(nc0 + ct, N - 1) * nb + b;
        scs[2 * i] = *(const wk_i2 *) (wsc + src * 16); scs[2 * i + 1] = *(const wk_i2 *) (wsc + src * 16 + 8);
        dws[i] = wd[src];
        if (MIN) dms[i] = wdm[src];
    }
    for (int i = threadIdx.x; i < 16 * nb; i += 256) {
        const int r = i / nb, b = i - r * nb;
        xds[i] = xd[(size_t) min(m0 + r, M - 1) * nb + b];
    }
    if (MIN)
        for (int i = threadIdx.x; i < 16 * nb * 8; i += 256) {          // Q5: bsums[2 g] + bsums[2 g + 1]; Q2: bsums[2 l] | bsums[2 l + 1] << 16, as they lie in memory
            const int r = i / (nb * 8), j = i - r * (nb * 8);
            const int bs2 = *(const int *) (xbs + (size_t) min(m0 + r, M - 1) * nb * 16 + 2 * j);
            xgs[i] = Q5 ? ((bs2 << 16) >> 16) + (bs2 >> 16) : bs2;
        }
    __syncthreads();                                           // the kernel's only barrier, before any wave leaves
    const int n0 = nc0 + (RS == 4 ? wv * 16 : 0);
    if (n0 >= N) return;                                       // (a whole wave)
    const int ct = (RS == 4 ? wv * 16 : 0) + c;                // the lane's column in the staged arrays
    const int n = n0 + c, nn = n < N ? n : N - 1;
    const int ma = min(RS == 4 ? m0 + c : m0 + (c & ~3) + wv, M - 1);         // the activation row whose bytes this lane feeds
    const int r0 = RS == 4 ? 4 * g : 4 * g + wv;                                // the tile rows r0 .. r0 + RS - 1 are this lane's results
    wa_epi_pre pre[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) pre[r] = epi_preload<EPI>(e, min(m0 + r0 + r, M - 1), nn);
    // 16-byte quads: the lane's (row, l = g, block b) is quads 2 b, 2 b + 1 from the base; l = 4 + g lies hs quads behind
    const wk_i4 * xa = (const wk_i4 *) xq + ((size_t) ma * 8 + g) * nb * 2;
    const wk_i4 * wb = (const wk_i4 *) wq + ((size_t) nn * 8 + g) * nb * 2;
    const size_t hs = (size_t) 8 * nb;
    const wk_i2 * scl = scs + (size_t) ct * nb * 2;
    const float * dwl = dws + ct * nb, * dml = dms + ct * nb;
    const float * dxl = xds + r0 * nb;
    const int * gsl = xgs + r0 * nb * 8;
    float acc[RS][8], summs[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        summs[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[r][t] = 0.0f;
    }
    wk_i4 an[4] = { xa[0], xa[1], xa[hs], xa[hs + 1] }, bn[4] = { wb[0], wb[1], wb[hs], wb[hs + 1] };
    for (int b = 0; b < nb; ++b) {
        wk_i4 a[4], w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = an[j]; w[j] = bn[j]; }
        const size_t qn = (size_t) 2 * min(b + 1, nb - 1);
        an[0] = xa[qn]; an[1] = xa[qn + 1]; an[2] = xa[hs + qn]; an[3] = xa[hs + qn + 1];
        bn[0] = wb[qn]; bn[1] = wb[qn + 1]; bn[2] = wb[hs + qn]; bn[3] = wb[hs + qn + 1];
        const wk_i2 sa = scl[2 * b], sb = scl[2 * b + 1];                      // the column's scale bytes 0..7 | 8..15 of this block
        const float dw = dwl[b];
        float dx[RS];
#pragma unroll
        for (int r = 0; r < RS; ++r) dx[r] = dxl[r * nb + b];
        if (Q2) {                  // the minimum term of sub-blocks 2 l and 2 l + 1 (bytes l and 8 + l, high nibble), before the product term
            const float dwm = dml[b];
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const wk_i4 p0 = *(const wk_i4 *) (gsl + (r * nb + b) * 8), p1 = *(const wk_i4 *) (gsl + (r * nb + b) * 8 + 4);
                const float dn = -dx[r] * dwm;
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    const int bs2 = l < 4 ? p0[l] : p1[l - 4];
                    const int mins = (wk_ubyte(sa, l) >> 4) * ((bs2 << 16) >> 16) + (wk_ubyte(sb, l) >> 4) * (bs2 >> 16);
                    acc[r][l] = fmaf(dn, (float) mins, acc[r][l]);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int t[RS][4];
#pragma unroll
            for (int r = 0; r < RS; ++r)
#pragma unroll
                for (int u = 0; u < 4; ++u) t[r][u] = 0;
#pragma unroll
            for (int gg = 0; gg < 8; ++gg) {
                const wk_i16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                const wk_i16 s = __builtin_amdgcn_mfma_i32_16x16x4i8(a[2 * h + (gg >> 2)][gg & 3], w[2 * h + (gg >> 2)][gg & 3], z, 0, 0, 0);
                const int sc = Q5 ? wk_byte<F>(sa, gg) : wk_byte<F>(h ? sb : sa, gg);
#pragma unroll
                for (int r = 0; r < RS; ++r)
#pragma unroll
                    for (int u = 0; u < 4; ++u) t[r][u] += __mul24(sc, s[4 * u + r]);      // register 4 u + r: l = 4 h + u, row r of the lane's
            }
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const float dd = dx[r] * dw;
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[r][4 * h + u] = fmaf(dd, (float) t[r][u], acc[r][4 * h + u]);
            }
        }
        if (Q5) {                  // the lane runs the minimum chain of its own outputs; the minimums are the block's scale bytes 8..15
            const float dwm = dml[b];
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const wk_i4 g0 = *(const wk_i4 *) (gsl + (r * nb + b) * 8), g1 = *(const wk_i4 *) (gsl + (r * nb + b) * 8 + 4);
                const int tot = wk_byte<WK_Q5>(sb, 0) * g0.x + wk_byte<WK_Q5>(sb, 1) * g0.y + wk_byte<WK_Q5>(sb, 2) * g0.z + wk_byte<WK_Q5>(sb, 3) * g0.w +
                                wk_byte<WK_Q5>(sb, 4) * g1.x + wk_byte<WK_Q5>(sb, 5) * g1.y + wk_byte<WK_Q5>(sb, 6) * g1.z + wk_byte<WK_Q5>(sb, 7) * g1.w;
                const float dm = -dx[r] * dwm;
                const float p = dm * (float) tot;
                summs[r] = summs[r] + p;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        float v = wk_hsum8_local(acc[r]);
        if (Q5) v = v + summs[r];
        if (n < N && m0 + r0 + r < M) epi_apply<EPI>(e, m0 + r0 + r, n, v, pre[r]);
    }
}

// the LDS of one workgroup: RS = 4 at K = 5120 with minimums is 42 240 B
static size_t kmfma_lds(bool min, bool wide, int K) {
    const size_t nb = (size_t) (K >> 8), ct = wide ? 64 : 16;
    return ct * nb * 16 + ct * nb * 4 * (min ? 2 : 1) + 16 * nb * 4 + (min ? 16 * nb * 8 * 4 : 0);
}
// The form with four rows per lane from 128 workgroups of 64 columns x 16 rows on, the one-row form below.  Measured on small:q6_k prompt passes
// (DESIGN.md 4.3): at 84 such workgroups (100 tokens, N = 768) the one-row form is the faster one, at 144 and 156 (40 tokens, N = 3072; 200 tokens,
// N = 768) the four-rows form; with k_qgemm_mfma's threshold of 512 the passes of 100 and 200 tokens were slower than with k_kgemm_exact.
static bool kmfma_wide(int M, int N) { return (long) ((N + 63) / 64) * ((M + 15) / 16) >= 128; }

// The matrix-core rule, as for the other formats (wa_quant.hip): every product of more than 8 rows whose rows belong to one state.  Measured on the
// MI355X k_kgemm_mfma is the faster one for every class timed: encoder grids and prompt passes of 12 .. 200 tokens.
// WHISPER_AMD_NO_QMFMA=1 (read once per process) goes back to k_kgemm_exact.
static bool kmfma_rule(int M) {
    static const bool off = getenv("WHISPER_AMD_NO_QMFMA") != nullptr;
    return !off && M >= 9;
}
// the kernel a route gives a product: 1 k_kgemm_exact (k_kgemv_exact for M == 1), 3 k_kgemm_mfma
int wa_kgemm_kernel(wa_epi_mode mode, int wtype, int M, int N, int K, const wa_epi & e, int route) {
    const bool has_mode = mode == WA_EPI_F16 || mode == WA_EPI_ENC_QKV || mode == WA_EPI_GELU_F32 || mode == WA_EPI_RESID || mode == WA_EPI_F32 ||
                          mode == WA_EPI_CROSS_KV || mode == WA_EPI_DEC_QKV;
    const bool fits = kmfma_lds(wtype == 13 || wtype == 10, kmfma_wide(M, N), K) <= 64 * 1024;
    if (M >= 9 && !e.rowp && has_mode && fits && route != 1 && (route == 3 || kmfma_rule(M))) return 3;
    return 1;
}

template <int F>
static void kmfma_launch(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq,
                         const int8_t * wsc, const float * wd, const float * wdm, int N, int K, const wa_epi & e) {
    const bool wide = kmfma_wide(M, N);
    const dim3 grid(wide ? (N + 63) / 64 : (N + 15) / 16, (M + 15) / 16);
    const size_t lds = kmfma_lds(F != WK_Q6, wide, K);
#define WA_MFMA_L(E, RS) do { \
        if (lds > 48 * 1024) (void) hipFuncSetAttribute((const void *) k_kgemm_mfma<E, F, RS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); \
        hipLaunchKernelGGL((k_kgemm_mfma<E, F, RS>), grid, dim3(256), lds, s, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e); } while (0)
#define WA_CASE(E) case E: if (wide) WA_MFMA_L(E, 4); else WA_MFMA_L(E, 1); break;
    switch (mode) {
        WA_CASE(WA_EPI_F16) WA_CASE(WA_EPI_ENC_QKV) WA_CASE(WA_EPI_GELU_F32) WA_CASE(WA_EPI_RESID) WA_CASE(WA_EPI_F32) WA_CASE(WA_EPI_CROSS_KV) WA_CASE(WA_EPI_DEC_QKV)
        default: break;
    }
#undef WA_CASE
#undef WA_MFMA_L
}

// route 0: the rule above picks the kernel; 1: wa_launch_kgemm_exact whatever it says; 3: k_kgemm_mfma wherever it applies (M >= 9, no rowp)
void wa_launch_kgemm_route(hipStream_t s, wa_epi_mode mode, int wtype, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq,
                           const int8_t * wsc, const float * wd, const float * wdm, int N, int K, const wa_epi & e, int route) {
    if (wa_kgemm_kernel(mode, wtype, M, N, K, e, route) != 3) { wa_launch_kgemm_exact(s, mode, wtype, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e); return; }
    if (wtype == 13) kmfma_launch<WK_Q5>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);
    else if (wtype == 10) kmfma_launch<WK_Q2>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);
    else kmfma_launch<WK_Q6>(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);        // Q6_K, and Q3_K as the loader unpacks it
}

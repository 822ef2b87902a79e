// wa_quant4.hip - Q4_0 (first half; Q4_K: second half) weights in the interleaved form of the reference (its CPU repack: ggml_gemv_q4_0_8x8_q8_0 / ggml_gemm_q4_0_8x8_q8_0) x Q8_0
// activation rows.  The arithmetic and the layouts are stated in host code in wa_quant4.h; a code object of its own (build/wa_quant4.o).
//
// Every output carries ONE float chain over the 32-value blocks, in block order,
//     acc = fma((float) isum_b, f32(d_w) * f32(d_x), acc),        isum_b the exact integer dot product of the block,
// with no lane partial sums and no horizontal sum.  So the integer part is wide and the float part narrow and serial, and the two kernels here
// split them:
//
//   k_q4gemv_rows  R = 1..8 activation rows (the single-token step, beams, lock-step rows, and slices of anything larger when the matrix-core
//                  kernel is switched off).  One wave = 8 outputs x 8 lanes.  The lanes of an output SPLIT THE BLOCKS: in a round of 32 blocks lane j
//                  takes blocks 4 j .. 4 j + 3 (16-byte loads: four blocks of one nibble word plane; any K with nb % 4 != 0: lane j takes blocks
//                  j, j + 8, ..), unpacks the nibbles to signed bytes once, and for each of the R rows forms isum_b with eight v_dot4_i32_i8 and the
//                  once-rounded scale product; both go to LDS as floats, [output][row][block of the round].  Behind the barrier lane r < R of the
//                  output's group runs the chain of activation row r over the round, in block order - R chains advance side by side in the
//                  group's lanes, so eight rows cost the serial time of one - and at the end applies the epilogue of (row r, output).  All R rows
//                  are served by one pass over the weights.
//   k_q4gemm_mfma  more than 8 rows: one wave = one 16 x 16 output tile.  One block is K = 32, so ONE v_mfma_i32_16x16x32_i8 with a zero
//                  accumulator gives the tile's 256 exact isum_b: lane (c, g) feeds activation row c's bytes of lanes g and 4 + g of the activation
//                  layout (elements 4 g .. 4 g + 3 and 16 + 4 g .. + 3) and the weight row c's nibble word (g, b), unpacked on the way from the load
//                  into the operand registers - low nibbles and high nibbles ARE those two element runs, in the same byte order; an integer sum
//                  is exact in any order, so only the pairing of the bytes matters.  The lane's four results (rows 4 g .. 4 g + 3, column c) feed
//                  four chains in registers, block after block.  No LDS, no barrier; the next four blocks' loads are in flight.
//
// Rows beyond M and columns beyond N read the last valid one and store nothing.  Every epilogue of wa_launch_qgemm_exact exists for both kernels.
#include "wa_device.h"
#include <cstdlib>

typedef int   q4_i4 __attribute__((ext_vector_type(4)));
typedef float q4_f4 __attribute__((ext_vector_type(4)));

// four unsigned nibble values 0..15, one per byte -> minus 8 in every byte
__device__ __forceinline__ int q4_s8(unsigned nib) {
    const unsigned r = nib ^ 0x08080808u;                                    // 8..15 -> 0..7; 0..7 -> 8..15, bit 3 set: the sign
    return (int) (r | (((r >> 3) & 0x01010101u) * 0xf0u));
}
// nibble word (g, b) -> the signed bytes of activation lanes g (low nibbles) and 4 + g (high nibbles)
#define Q4_UNPACK(u, lo, hi) do { lo = q4_s8((u) & 0x0f0f0f0fu); hi = q4_s8(((u) >> 4) & 0x0f0f0f0fu); } while (0)

// -------------------------------------------------------------------------------------------------
// R = 1..8 rows; grid = ceil(N / 8) single-wave workgroups.  x rows m0 .. m0 + R - 1 are xq / xd's first R rows (the launcher offsets the pointers).
// -------------------------------------------------------------------------------------------------
// one block of one output: the eight signed words of the weight block against the R activation rows -> fs / ps [row][bl]
template <int R>
__device__ __forceinline__ void q4_block_rows(const int w[8], float dw, const int * __restrict__ xi, const float * __restrict__ xd, int nb, int b,
                                              float (* fs)[32], float (* ps)[32], int bl) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int s = 0;
#pragma unroll
        for (int l = 0; l < 8; ++l) s = __builtin_amdgcn_sdot4(w[l], xi[((size_t) r * 8 + l) * nb + b], s, false);
        fs[r][bl] = (float) s;
        ps[r][bl] = dw * xd[(size_t) r * nb + b];
    }
}

template <int EPI, int R>
__global__ __launch_bounds__(64) void k_q4gemv_rows(const int8_t * __restrict__ xq, const float * __restrict__ xd, int m0, const unsigned * __restrict__ wq,
                                                    const float * __restrict__ wd, int N, int K, wa_epi e) {
    __shared__ __attribute__((aligned(16))) float fs[8][R][32], ps[8][R][32];      // (float) isum and the scale product: [output][row][block of the round]
    const int tid = threadIdx.x, j = tid & 7, o = tid >> 3, nb = K >> 5;
    const int n = blockIdx.x * 8 + o;
    const int nn = n < N ? n : N - 1;
    const int rr = j < R ? j : R - 1;                                         // the activation row whose chain this lane runs (j >= R: idle copies)
    const wa_epi_pre pre = epi_preload<EPI>(e, m0 + rr, nn);
    const unsigned * wl = wq + (size_t) nn * 4 * nb;                           // word (g, b) at g nb + b
    const float * dl = wd + (size_t) nn * nb;
    const int * xi = (const int *) xq;
    float acc = 0.0f;
    for (int b0 = 0; b0 < nb; b0 += 32) {
        const int cnt = min(32, nb - b0);
        if ((nb & 3) == 0) {
            if (4 * j < cnt) {                                                 // blocks b0 + 4 j .. + 3, 16-byte loads
                const int b = b0 + 4 * j;
                q4_i4 u[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) u[g] = *(const q4_i4 *) (wl + (size_t) g * nb + b);
                const q4_f4 dw = *(const q4_f4 *) (dl + b);
                int w[4][8];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int g = 0; g < 4; ++g) Q4_UNPACK((unsigned) u[g][i], w[i][g], w[i][4 + g]);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    q4_i4 x[8];
#pragma unroll
                    for (int l = 0; l < 8; ++l) x[l] = *(const q4_i4 *) (xi + ((size_t) r * 8 + l) * nb + b);
                    const q4_f4 dx = *(const q4_f4 *) (xd + (size_t) r * nb + b);
                    q4_f4 f, p;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        int s = 0;
#pragma unroll
                        for (int l = 0; l < 8; ++l) s = __builtin_amdgcn_sdot4(w[i][l], x[l][i], s, false);
                        f[i] = (float) s;
                        p[i] = dw[i] * dx[i];
                    }
                    *(q4_f4 *) &fs[o][r][4 * j] = f;
                    *(q4_f4 *) &ps[o][r][4 * j] = p;
                }
            }
        } else {
            for (int bl = j; bl < cnt; bl += 8) {
                const int b = b0 + bl;
                int w[8];
#pragma unroll
                for (int g = 0; g < 4; ++g) Q4_UNPACK(wl[(size_t) g * nb + b], w[g], w[4 + g]);
                q4_block_rows<R>(w, dl[b], xi, xd, nb, b, fs[o], ps[o], bl);
            }
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) acc = fmaf(fs[o][rr][t], ps[o][rr][t], acc);      // the chain of (row rr, output n): block order, one lane
        __syncthreads();
    }
    if (j < R && n < N) epi_apply<EPI>(e, m0 + j, n, acc, pre);
}

// -------------------------------------------------------------------------------------------------
// M > 8 on the int8 matrix cores; grid = (ceil(N / 16), ceil(M / 16)) single-wave workgroups
// -------------------------------------------------------------------------------------------------
#define Q4_MFMA_BLOCK(acc, ALO, AHI, U, DW, DX) do { \
        int q4_lo, q4_hi; \
        Q4_UNPACK((unsigned) (U), q4_lo, q4_hi); \
        const long q4_a = (long) (((unsigned long) (unsigned) (AHI) << 32) | (unsigned long) (unsigned) (ALO)); \
        const long q4_b = (long) (((unsigned long) (unsigned) q4_hi << 32) | (unsigned long) (unsigned) q4_lo); \
        const q4_i4 q4_z = {0, 0, 0, 0}; \
        const q4_i4 q4_s = __builtin_amdgcn_mfma_i32_16x16x32_i8(q4_a, q4_b, q4_z, 0, 0, 0); \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) { const float q4_p = (DW) * (DX)[r]; acc[r] = fmaf((float) q4_s[r], q4_p, acc[r]); } \
    } while (0)

template <int EPI>
__global__ __launch_bounds__(64) void k_q4gemm_mfma(const int8_t * __restrict__ xq, const float * __restrict__ xd, int M, const unsigned * __restrict__ wq,
                                                    const float * __restrict__ wd, int N, int K, wa_epi e) {
    const int nb = K >> 5, lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
    const int n = n0 + c, nn = n < N ? n : N - 1;
    const int ma = min(m0 + c, M - 1);                                         // the activation row whose bytes this lane feeds
    const int r0 = 4 * g;                                                      // the tile rows r0 .. r0 + 3, column c, are this lane's results
    wa_epi_pre pre[4];
    const float * dxl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int mr = min(m0 + r0 + r, M - 1);
        pre[r] = epi_preload<EPI>(e, mr, nn);
        dxl[r] = xd + (size_t) mr * nb;
    }
    const int * xa = (const int *) xq + ((size_t) ma * 8 + g) * nb;           // lane l = g of the row; l = 4 + g lies h words behind
    const size_t h = (size_t) 4 * nb;
    const unsigned * wb = wq + ((size_t) nn * 4 + g) * nb;
    const float * dwl = wd + (size_t) nn * nb;
    float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if ((nb & 3) == 0) {
        q4_i4 an = *(const q4_i4 *) xa, bn = *(const q4_i4 *) (xa + h), un = *(const q4_i4 *) wb;
        q4_f4 dn = *(const q4_f4 *) dwl, en[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) en[r] = *(const q4_f4 *) dxl[r];
        for (int b = 0; b < nb; b += 4) {
            const q4_i4 a0 = an, a1 = bn, u = un; const q4_f4 dw = dn;
            q4_f4 dx4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) dx4[r] = en[r];
            const int bq = min(b + 4, nb - 4);
            an = *(const q4_i4 *) (xa + bq); bn = *(const q4_i4 *) (xa + h + bq); un = *(const q4_i4 *) (wb + bq); dn = *(const q4_f4 *) (dwl + bq);
#pragma unroll
            for (int r = 0; r < 4; ++r) en[r] = *(const q4_f4 *) (dxl[r] + bq);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float dx[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) dx[r] = dx4[r][i];
                Q4_MFMA_BLOCK(acc, a0[i], a1[i], u[i], dw[i], dx);
            }
        }
    } else {
        for (int b = 0; b < nb; ++b) {
            float dx[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) dx[r] = dxl[r][b];
            Q4_MFMA_BLOCK(acc, xa[b], xa[h + b], wb[b], dwl[b], dx);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (n < N && m0 + r0 + r < M) epi_apply<EPI>(e, m0 + r0 + r, n, acc[r], pre[r]);
}

// The matrix-core rule, as for the other formats: every product of more than 8 rows.  WHISPER_AMD_NO_QMFMA=1 (read once per process) sends them through
// k_q4gemv_rows in slices of 8 rows instead: the same chains, the same bits.
static bool q4mfma_rule(int M) {
    static const bool off = getenv("WHISPER_AMD_NO_QMFMA") != nullptr;
    return !off && M >= 9;
}
// the kernel a route gives a product: 2 k_q4gemv_rows, 3 k_q4gemm_mfma.  Route 0: the rule; 2: k_q4gemv_rows whatever M; 3: k_q4gemm_mfma whatever M
int wa_q4gemm_kernel(int M, int route) { return route == 3 || (route != 2 && q4mfma_rule(M)) ? 3 : 2; }

template <int EPI>
static void q4_launch(hipStream_t s, const int8_t * xq, const float * xd, int M, const unsigned * wq, const float * wd, int N, int K, const wa_epi & e, int route) {
    if (wa_q4gemm_kernel(M, route) == 3) {
        hipLaunchKernelGGL((k_q4gemm_mfma<EPI>), dim3((N + 15) / 16, (M + 15) / 16), dim3(64), 0, s, xq, xd, M, wq, wd, N, K, e);
        return;
    }
    const int nb = K >> 5;
    for (int m0 = 0; m0 < M; m0 += 8) {
        const int8_t * xq0 = xq + (size_t) m0 * K; const float * xd0 = xd + (size_t) m0 * nb;
#define WA_Q4_R(R) case R: hipLaunchKernelGGL((k_q4gemv_rows<EPI, R>), dim3((N + 7) / 8), dim3(64), 0, s, xq0, xd0, m0, wq, wd, N, K, e); break;
        switch (M - m0 < 8 ? M - m0 : 8) { WA_Q4_R(1) WA_Q4_R(2) WA_Q4_R(3) WA_Q4_R(4) WA_Q4_R(5) WA_Q4_R(6) WA_Q4_R(7) WA_Q4_R(8) default: break; }
#undef WA_Q4_R
    }
}

void wa_launch_q4gemm_route(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, int M, const uint8_t * wq, const float * wd, int N, int K,
                            const wa_epi & e, int route) {
    if (M < 1 || N < 1 || K < 32 || (K & 31)) return;
    const unsigned * w = (const unsigned *) wq;
#define WA_CASE(E) case E: q4_launch<E>(s, xq, xd, M, w, wd, N, K, e, route); break;
    switch (mode) {
        WA_CASE(WA_EPI_F16) WA_CASE(WA_EPI_ENC_QKV) WA_CASE(WA_EPI_GELU_F32) WA_CASE(WA_EPI_RESID) WA_CASE(WA_EPI_F32) WA_CASE(WA_EPI_CROSS_KV) WA_CASE(WA_EPI_DEC_QKV)
        default: break;
    }
#undef WA_CASE
}
void wa_launch_q4gemm(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, int M, const uint8_t * wq, const float * wd, int N, int K,
                      const wa_epi & e) {
    wa_launch_q4gemm_route(s, mode, xq, xd, M, wq, wd, N, K, e, 0);
}

// =================================================================================================
// Q4_K weights in the interleaved form (ggml_gemv_q4_K_8x8_q8_K / ggml_gemm_q4_K_8x8_q8_K) x Q8_K activation rows; wa_quant4.h states the arithmetic.
// Two chains per output, acc and accmin, out = acc - accmin.  The rows below n4 = wa_q4_K_rows4(M) are the reference's gemm rows: the four-row quantiser's
// sign rule, and a chain step per PAIR of sub-blocks; the rows from n4 on are its gemv rows: the row quantiser, one step per 256-value block.
//   k_q8k_quant4     the Q8_K quantiser with either rule, into the buffers of wa_launch_quantize_q8_K
//   k_q4kgemv_rows   R = 1..8 rows, one wave = 8 outputs x 8 lanes; the lanes of an output split the BLOCKS (lane j: blocks j, j + 8, ..): per block 64
//                    v_dot4_i32_i8 per row on the nibbles unpacked once, the sub-block scales and the minimum term in int32; the float forms of the
//                    pair sums (gemm rows) or of the block sum (gemv rows) and the two scale products go to LDS, and lane r < R runs both chains of row r
//   k_q4kgemm_mfma   more than 8 rows, one wave = one 16 x 16 tile: eight v_mfma_i32_16x16x32_i8 per block (one per sub-block), scaled and summed
//                    in int32 per lane, the minimum term from the rows' bsums, both chains in registers.  A lane's four rows 4 g .. 4 g + 3 lie on
//                    one side of n4 (a multiple of 4): the step rule is uniform per lane.
//   k_q4k_plain_rows the plain product (the token embedding -> logits): Q5_K's eight-lane chains and four minimum chains (ggml_vec_dot_q4_K_q8_K)
// =================================================================================================
typedef int q4_i2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int q4_ub(q4_i4 v, int i) { return (int) (((unsigned) v[i >> 2] >> (8 * (i & 3))) & 0xffu); }      // byte i of 16
__device__ __forceinline__ int q4_pair16(int v) { return ((v << 16) >> 16) + (v >> 16); }                                      // the two int16 halves, added

__global__ __launch_bounds__(256) void k_q8k_quant4(const float * __restrict__ x, int ldx, int rows, int n4, int K, int8_t * __restrict__ qs,
                                                    float * __restrict__ qd, int16_t * __restrict__ qbs) {
    const int nb = K >> 8;
    const long gb = (long) blockIdx.x * 4 + (threadIdx.x >> 6);      // wave-uniform: one wave per 256-value block, lane i holds elements 4 i .. 4 i + 3
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
    const unsigned long long plus = __ballot(v.x == wmax || v.y == wmax || v.z == wmax || v.w == wmax);      // an element equal to + max|x|
    const float fmx = __shfl(mx, __ffsll((long long) holders) - 1, WAVE);                                     // the FIRST element of largest magnitude
    int q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    float d = 0.0f;
    if (wmax != 0.0f) {
        const bool four = row < n4;
        const float iscale = four ? (plus ? -127.f / wmax : 127.f / wmax) : -127.f / fmx;
        q0 = (int) rintf(iscale * v.x); q1 = (int) rintf(iscale * v.y); q2 = (int) rintf(iscale * v.z); q3 = (int) rintf(iscale * v.w);
        const int lo = four ? -128 : -2147483647 - 1;                         // the four-row form saturates in its packs, the row form clamps with min(127, .)
        q0 = max(lo, min(127, q0)); q1 = max(lo, min(127, q1)); q2 = max(lo, min(127, q2)); q3 = max(lo, min(127, q3));
        d = 1.0f / iscale;
    }
    *(int *) (qs + (((size_t) row * 8 + (i & 7)) * nb + b) * 32 + (i >> 3) * 4) = (q0 & 0xff) | ((q1 & 0xff) << 8) | ((q2 & 0xff) << 16) | ((q3 & 0xff) << 24);
    int s = (q0 + q1) + (q2 + q3);
    s += __builtin_amdgcn_update_dpp(0, s, 0xb1, 0xf, 0xf, true);        // quad_perm [1, 0, 3, 2]
    s += __builtin_amdgcn_update_dpp(0, s, 0x4e, 0xf, 0xf, true);        // quad_perm [2, 3, 0, 1]: the 16 elements of lanes 4 j .. 4 j + 3
    if ((i & 3) == 0) qbs[((size_t) row * nb + b) * 16 + (i >> 2)] = (int16_t) s;
    if (i == 0) qd[(size_t) row * nb + b] = d;
}
void wa_launch_quantize_q8_K4(hipStream_t stream, const float * x, int ldx, int rows, int K, int8_t * qs, float * qd, int16_t * qbs) {
    const long nblk = (long) rows * (K >> 8);
    const int n4 = rows > 3 ? rows & ~3 : 0;
    hipLaunchKernelGGL(k_q8k_quant4, dim3((unsigned) ((nblk + 3) / 4)), dim3(256), 0, stream, x, ldx, rows, n4, K, qs, qd, qbs);
}

#define Q4K_RB 16        // blocks per round of the few-rows kernel's LDS
template <int EPI, int R>
__global__ __launch_bounds__(64) void k_q4kgemv_rows(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int16_t * __restrict__ xbs, int m0, int n4,
                                                     const unsigned * __restrict__ wq, const uint8_t * __restrict__ wsc, const float * __restrict__ wd,
                                                     const float * __restrict__ wdm, int N, int K, wa_epi e) {
    // (float) pair sums [4] (gemv rows: [0] = the block's sum) of the product and of the minimum term, and the two scale products: [output][row][block of the round]
    __shared__ __attribute__((aligned(16))) float fs[8][R][Q4K_RB][4], fm[8][R][Q4K_RB][4], ps[8][R][Q4K_RB], pm[8][R][Q4K_RB];
    const int tid = threadIdx.x, j = tid & 7, o = tid >> 3, nb = K >> 8;
    const int n = blockIdx.x * 8 + o;
    const int nn = n < N ? n : N - 1;
    const int rr = j < R ? j : R - 1;                                         // the activation row whose chains this lane runs
    const bool gemm_rr = m0 + rr < n4;
    const wa_epi_pre pre = epi_preload<EPI>(e, m0 + rr, nn);
    float acc = 0.0f, accm = 0.0f;
    for (int b0 = 0; b0 < nb; b0 += Q4K_RB) {
        const int cnt = min(Q4K_RB, nb - b0);
        for (int bl = j; bl < cnt; bl += 8) {
            const int b = b0 + bl;
            q4_i4 w[8];
#pragma unroll
            for (int l = 0; l < 8; ++l) w[l] = *(const q4_i4 *) (wq + (((size_t) nn * 8 + l) * nb + b) * 4);
            const q4_i4 scv = *(const q4_i4 *) (wsc + ((size_t) nn * nb + b) * 16);
            const float dw = wd[(size_t) nn * nb + b], dmw = wdm[(size_t) nn * nb + b];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                int t[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };                        // the sub-blocks' dot products
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    const q4_i4 * xp = (const q4_i4 *) (xq + (size_t) r * K + ((size_t) l * nb + b) * 32);
                    const q4_i4 x0 = xp[0], x1 = xp[1];                       // sub-blocks 0..3 | 4..7 of lane l
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const unsigned wv = (unsigned) w[l][u];
                        t[2 * u]     = __builtin_amdgcn_sdot4((int) (wv & 0x0f0f0f0fu), u < 2 ? x0[2 * u] : x1[2 * u - 4], t[2 * u], false);
                        t[2 * u + 1] = __builtin_amdgcn_sdot4((int) ((wv >> 4) & 0x0f0f0f0fu), u < 2 ? x0[2 * u + 1] : x1[2 * u - 3], t[2 * u + 1], false);
                    }
                }
                const q4_i4 * bp = (const q4_i4 *) (xbs + ((size_t) r * nb + b) * 16);
                const q4_i4 bs0 = bp[0], bs1 = bp[1];                         // int k: bsums[2 k] | bsums[2 k + 1] << 16 - sub-block k's two halves
                int ip[4], im[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int sa = q4_pair16(u < 2 ? bs0[2 * u] : bs1[2 * u - 4]), sb = q4_pair16(u < 2 ? bs0[2 * u + 1] : bs1[2 * u - 3]);
                    ip[u] = q4_ub(scv, 2 * u) * t[2 * u] + q4_ub(scv, 2 * u + 1) * t[2 * u + 1];
                    im[u] = q4_ub(scv, 8 + 2 * u) * sa + q4_ub(scv, 9 + 2 * u) * sb;
                }
                q4_f4 f, g;
                if (m0 + r < n4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) { f[u] = (float) ip[u]; g[u] = (float) im[u]; }
                } else {
                    f[0] = (float) ((ip[0] + ip[1]) + (ip[2] + ip[3])); g[0] = (float) ((im[0] + im[1]) + (im[2] + im[3]));
                    f[1] = f[2] = f[3] = 0.0f; g[1] = g[2] = g[3] = 0.0f;
                }
                *(q4_f4 *) fs[o][r][bl] = f;
                *(q4_f4 *) fm[o][r][bl] = g;
                const float dx = xd[(size_t) r * nb + b];
                ps[o][r][bl] = dw * dx;
                pm[o][r][bl] = dmw * dx;
            }
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {                                       // both chains of (row rr, output n): block order, one lane
            const q4_f4 f = *(const q4_f4 *) fs[o][rr][t], g = *(const q4_f4 *) fm[o][rr][t];
            const float p = ps[o][rr][t], q = pm[o][rr][t];
            acc = fmaf(f[0], p, acc); accm = fmaf(g[0], q, accm);
            if (gemm_rr) {
#pragma unroll
                for (int u = 1; u < 4; ++u) { acc = fmaf(f[u], p, acc); accm = fmaf(g[u], q, accm); }
            }
        }
        __syncthreads();
    }
    if (j < R && n < N) epi_apply<EPI>(e, m0 + j, n, acc - accm, pre);
}

template <int EPI>
__global__ __launch_bounds__(64) void k_q4kgemm_mfma(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int16_t * __restrict__ xbs, int M, int n4,
                                                     const unsigned * __restrict__ wq, const uint8_t * __restrict__ wsc, const float * __restrict__ wd,
                                                     const float * __restrict__ wdm, int N, int K, wa_epi e) {
    const int nb = K >> 8, lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
    const int n = n0 + c, nn = n < N ? n : N - 1;
    const int ma = min(m0 + c, M - 1);                                         // the activation row whose bytes this lane feeds
    const int r0 = 4 * g;                                                      // the tile rows r0 .. r0 + 3, column c, are this lane's results
    const bool four = m0 + r0 < n4;                                            // gemm rows: a chain step per pair of sub-blocks
    wa_epi_pre pre[4];
    const float * dxl[4]; const q4_i4 * bsl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int mr = min(m0 + r0 + r, M - 1);
        pre[r] = epi_preload<EPI>(e, mr, nn);
        dxl[r] = xd + (size_t) mr * nb;
        bsl[r] = (const q4_i4 *) (xbs + (size_t) mr * nb * 16);
    }
    const q4_i4 * xa = (const q4_i4 *) (xq + (size_t) ma * K);                 // lane l, block b: quads 2 (l nb + b), + 1
    const q4_i4 * wb = (const q4_i4 *) wq + (size_t) nn * 8 * nb;              // lane l, block b: quad l nb + b
    float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, accm[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int b = 0; b < nb; ++b) {
        const q4_i4 a0 = xa[2 * ((size_t) g * nb + b)], a1 = xa[2 * ((size_t) g * nb + b) + 1];
        const q4_i4 a2 = xa[2 * ((size_t) (4 + g) * nb + b)], a3 = xa[2 * ((size_t) (4 + g) * nb + b) + 1];
        const q4_i4 w0 = wb[(size_t) g * nb + b], w1 = wb[(size_t) (4 + g) * nb + b];
        const q4_i4 scv = *(const q4_i4 *) (wsc + ((size_t) nn * nb + b) * 16);
        const float dw = wd[(size_t) nn * nb + b], dmw = wdm[(size_t) nn * nb + b];
        float p[4], q[4]; q4_i4 bs0[4], bs1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float dx = dxl[r][b]; p[r] = dw * dx; q[r] = dmw * dx; bs0[r] = bsl[r][2 * b]; bs1[r] = bsl[r][2 * b + 1]; }
        int ts[4] = { 0, 0, 0, 0 }, ms[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned wa = (unsigned) w0[u], wc = (unsigned) w1[u];
            const q4_i4 z = {0, 0, 0, 0};
            const int xl0 = u < 2 ? a0[2 * u] : a1[2 * u - 4], xh0 = u < 2 ? a2[2 * u] : a3[2 * u - 4];              // sub-block 2 u: lanes g, 4 + g
            const int xl1 = u < 2 ? a0[2 * u + 1] : a1[2 * u - 3], xh1 = u < 2 ? a2[2 * u + 1] : a3[2 * u - 3];      // sub-block 2 u + 1
            const long A0 = (long) (((unsigned long) (unsigned) xh0 << 32) | (unsigned long) (unsigned) xl0);
            const long A1 = (long) (((unsigned long) (unsigned) xh1 << 32) | (unsigned long) (unsigned) xl1);
            const long B0 = (long) (((unsigned long) (wc & 0x0f0f0f0fu) << 32) | (unsigned long) (wa & 0x0f0f0f0fu));
            const long B1 = (long) (((unsigned long) ((wc >> 4) & 0x0f0f0f0fu) << 32) | (unsigned long) ((wa >> 4) & 0x0f0f0f0fu));
            const q4_i4 s0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(A0, B0, z, 0, 0, 0);
            const q4_i4 s1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(A1, B1, z, 0, 0, 0);
            const int sc0 = q4_ub(scv, 2 * u), sc1 = q4_ub(scv, 2 * u + 1), mn0 = q4_ub(scv, 8 + 2 * u), mn1 = q4_ub(scv, 9 + 2 * u);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tp = sc0 * s0[r] + sc1 * s1[r];
                const int mp = mn0 * q4_pair16(u < 2 ? bs0[r][2 * u] : bs1[r][2 * u - 4]) + mn1 * q4_pair16(u < 2 ? bs0[r][2 * u + 1] : bs1[r][2 * u - 3]);
                if (four) { acc[r] = fmaf((float) tp, p[r], acc[r]); accm[r] = fmaf((float) mp, q[r], accm[r]); }
                else { ts[r] += tp; ms[r] += mp; }
            }
        }
        if (!four) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc[r] = fmaf((float) ts[r], p[r], acc[r]); accm[r] = fmaf((float) ms[r], q[r], accm[r]); }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (n < N && m0 + r0 + r < M) epi_apply<EPI>(e, m0 + r0 + r, n, acc[r] - accm[r], pre[r]);
}

template <int EPI>
static void q4k_launch(hipStream_t s, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const unsigned * wq, const uint8_t * wsc, const float * wd,
                       const float * wdm, int N, int K, const wa_epi & e, int route) {
    const int n4 = M > 3 ? M & ~3 : 0, nb = K >> 8;
    if (wa_q4gemm_kernel(M, route) == 3) {
        hipLaunchKernelGGL((k_q4kgemm_mfma<EPI>), dim3((N + 15) / 16, (M + 15) / 16), dim3(64), 0, s, xq, xd, xbs, M, n4, wq, wsc, wd, wdm, N, K, e);
        return;
    }
    for (int m0 = 0; m0 < M; m0 += 8) {
        const int8_t * xq0 = xq + (size_t) m0 * K; const float * xd0 = xd + (size_t) m0 * nb; const int16_t * xb0 = xbs + (size_t) m0 * nb * 16;
#define WA_Q4_R(R) case R: hipLaunchKernelGGL((k_q4kgemv_rows<EPI, R>), dim3((N + 7) / 8), dim3(64), 0, s, xq0, xd0, xb0, m0, n4, wq, wsc, wd, wdm, N, K, e); break;
        switch (M - m0 < 8 ? M - m0 : 8) { WA_Q4_R(1) WA_Q4_R(2) WA_Q4_R(3) WA_Q4_R(4) WA_Q4_R(5) WA_Q4_R(6) WA_Q4_R(7) WA_Q4_R(8) default: break; }
#undef WA_Q4_R
    }
}
void wa_launch_q4kgemm_route(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const uint8_t * wq, const uint8_t * wsc,
                             const float * wd, const float * wdm, int N, int K, const wa_epi & e, int route) {
    if (M < 1 || N < 1 || K < 256 || (K & 255)) return;
    const unsigned * w = (const unsigned *) wq;
#define WA_CASE(E) case E: q4k_launch<E>(s, xq, xd, xbs, M, w, wsc, wd, wdm, N, K, e, route); break;
    switch (mode) {
        WA_CASE(WA_EPI_F16) WA_CASE(WA_EPI_ENC_QKV) WA_CASE(WA_EPI_GELU_F32) WA_CASE(WA_EPI_RESID) WA_CASE(WA_EPI_F32) WA_CASE(WA_EPI_CROSS_KV) WA_CASE(WA_EPI_DEC_QKV)
        default: break;
    }
#undef WA_CASE
}
void wa_launch_q4kgemm(hipStream_t s, wa_epi_mode mode, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const uint8_t * wq, const uint8_t * wsc,
                       const float * wd, const float * wdm, int N, int K, const wa_epi & e) {
    wa_launch_q4kgemm_route(s, mode, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e, 0);
}

// -------------------------------------------------------------------------------------------------
// the plain product, rows m0 .. m0 + R - 1 -> out f32 [m][ldo]; grid = ceil(N / 8) single-wave workgroups, 8 lanes per output: lane l owns elements
// 4 l .. 4 l + 3 of every sub-block (Q5_K's layout and lane chains); lane l runs minimum chain l & 3 of every row, lanes 0..3 meet over DPP
// -------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64) void k_q4k_plain_rows(const int8_t * __restrict__ xq, const float * __restrict__ xd, const int16_t * __restrict__ xbs,
                                                       const int8_t * __restrict__ wq, const uint8_t * __restrict__ wsc, const float * __restrict__ wd,
                                                       const float * __restrict__ wdm, int N, int K, float * __restrict__ out, int ldo) {
    const int tid = threadIdx.x, l = tid & 7, k = l & 3, nb = K >> 8;
    const int n = blockIdx.x * 8 + (tid >> 3);
    const int nn = n < N ? n : N - 1;
    const q4_i4 * wl = (const q4_i4 *) (wq + ((size_t) nn * 8 + l) * nb * 32);
    float acc[R], am[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { acc[r] = 0.0f; am[r] = 0.0f; }
    for (int b = 0; b < nb; ++b) {
        const q4_i4 w0 = wl[2 * b], w1 = wl[2 * b + 1];
        const q4_i4 scv = *(const q4_i4 *) (wsc + ((size_t) nn * nb + b) * 16);
        const float dw = wd[(size_t) nn * nb + b], dmw = wdm[(size_t) nn * nb + b];
        const unsigned mw = (unsigned) (k < 2 ? scv.z : scv.w) >> (16 * (k & 1));             // m[2 k] | m[2 k + 1] << 8
        const int ma = (int) (mw & 0xffu), mb = (int) ((mw >> 8) & 0xffu);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const q4_i4 * xp = (const q4_i4 *) (xq + (size_t) r * K + ((size_t) l * nb + b) * 32);
            const q4_i4 x0 = xp[0], x1 = xp[1];
            int sumi = 0;
#pragma unroll
            for (int g = 0; g < 8; ++g) sumi += q4_ub(scv, g) * __builtin_amdgcn_sdot4(g < 4 ? w0[g] : w1[g - 4], g < 4 ? x0[g] : x1[g - 4], 0, false);
            const float dx = xd[(size_t) r * nb + b];
            const float dd = dx * dw;
            acc[r] = fmaf(dd, (float) sumi, acc[r]);
            const q4_i2 bs = *(const q4_i2 *) (xbs + ((size_t) r * nb + b) * 16 + 4 * k);      // bsums 4 k .. 4 k + 3: sub-blocks 2 k and 2 k + 1
            const float dm = -dx * dmw;
            am[r] = fmaf(dm, (float) (ma * q4_pair16(bs.x) + mb * q4_pair16(bs.y)), am[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float v = acc[r];
        v = v + dpp_f32<0x104>(v); v = v + dpp_f32<0x102>(v); v = v + dpp_f32<0x101>(v);      // hsum_float_8
        float m = am[r];
        m = m + dpp_f32<0x102>(m);                                                             // lane 0: am0 + am2, lane 1: am1 + am3
        m = m + dpp_f32<0x101>(m);
        if (l == 0 && n < N) out[(size_t) r * ldo + n] = v + m;
    }
}
void wa_launch_q4k_plain(hipStream_t s, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq, const int8_t * wsc, const float * wd,
                         const float * wdm, int N, int K, float * out, int ldo) {
    if (M < 1 || N < 1 || K < 256 || (K & 255)) return;
    const int nb = K >> 8;
    for (int m0 = 0; m0 < M; m0 += 8) {
        const int8_t * xq0 = xq + (size_t) m0 * K; const float * xd0 = xd + (size_t) m0 * nb; const int16_t * xb0 = xbs + (size_t) m0 * nb * 16;
        float * o0 = out + (size_t) m0 * ldo;
#define WA_Q4_R(R) case R: hipLaunchKernelGGL((k_q4k_plain_rows<R>), dim3((N + 7) / 8), dim3(64), 0, s, xq0, xd0, xb0, wq, (const uint8_t *) wsc, wd, wdm, N, K, o0, ldo); break;
        switch (M - m0 < 8 ? M - m0 : 8) { WA_Q4_R(1) WA_Q4_R(2) WA_Q4_R(3) WA_Q4_R(4) WA_Q4_R(5) WA_Q4_R(6) WA_Q4_R(7) WA_Q4_R(8) default: break; }
#undef WA_Q4_R
    }
}

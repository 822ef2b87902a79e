// Host reference of the K-format kernels (whisper-rust_amd/csrc/wa_quantk.hip): the functions of wa_quantk.h behind C entry points that
// take and give the KERNEL layout (quants [row][8][block][8][4], scale bytes [row][block][16], d / dmin [row][block], activation sums
// [row][block][16]), and beside them deliberately wrong variants - each must move some expected value, or the cases that pin it are missing:
//   quantiser  variant 1: the LAST element of largest magnitude gives the scale's sign
//   unpack     variant 1: the two nibble halves of a byte swapped
//   product    variant 1: the lane chain as a multiplication and an addition (no fma)      2: hsum_float_8 in lane order
//              variant 3: (Q5_K) the summs step as one fma                                4: (Q5_K) summs added before the lane sums' halves meet
// tests/native/kquant_math.cpp includes this file and holds variant 0 to the reference library.
#include "wa_quantk.h"

#include <vector>

static void kq_unpack_block(int type, const uint8_t * blk, int8_t q[256], int8_t sc[16], float & d, float & dmin, int variant) {
    if (variant == 0) { wa_qk_unpack(type, blk, q, sc, d, dmin); return; }
    std::vector<uint8_t> t(blk, blk + wa_qk_block_bytes(type));
    uint8_t * qs = t.data() + (type == WA_TYPE_Q6_K ? 0 : 48);
    for (int i = 0; i < 128; ++i) qs[i] = (uint8_t) ((qs[i] >> 4) | (qs[i] << 4));
    wa_qk_unpack(type, t.data(), q, sc, d, dmin);
}

static void kq_q8_K_row(const float * x, int nb, int8_t * q, float * d, int16_t * bsums, int variant) {
    if (variant == 0) { wa_q8_K_row(x, nb, q, d, bsums); return; }
    for (int b = 0; b < nb; ++b, x += 256, q += 256, bsums += 16) {
        float max = 0.0f, amax = 0.0f;
        for (int j = 0; j < 256; ++j) { const float ax = fabsf(x[j]); if (ax >= amax) { amax = ax; max = x[j]; } }      // >= : the last index
        if (!(amax != 0.0f)) { d[b] = 0.0f; memset(q, 0, 256); memset(bsums, 0, 32); continue; }
        const float iscale = -127.f / max;
        for (int j = 0; j < 256; ++j) { const float p = iscale * x[j]; const int v = (int) rintf(p); q[j] = (int8_t) (v < 127 ? v : 127); }
        for (int j = 0; j < 16; ++j) { int s = 0; for (int i = 0; i < 16; ++i) s += q[16 * j + i]; bsums[j] = (int16_t) s; }
        d[b] = 1.0f / iscale;
    }
}

static float kq_dot(int type, int nb, const int8_t * wq, const int8_t * wsc, const float * wd, const float * wdmin, const int8_t * xq,
                    const float * xd, const int16_t * xbs, int variant) {
    if (variant == 0) return wa_qk_dot(type, nb, wq, wsc, wd, wdmin, xq, xd, xbs);
    float acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    float summs = 0.0f;
    for (int b = 0; b < nb; ++b) {
        const float dd = xd[b] * wd[b];
        if (type == WA_TYPE_Q5_K) {
            const float dm = -xd[b] * wdmin[b];
            int s = 0;
            for (int g = 0; g < 8; ++g) s += (int) wsc[16 * b + 8 + g] * ((int) xbs[16 * b + 2 * g] + (int) xbs[16 * b + 2 * g + 1]);
            if (variant == 3) summs = fmaf(dm, (float) s, summs);
            else { const float p = dm * (float) s; summs = summs + p; }
        }
        for (int l = 0; l < 8; ++l) {
            int sumi = 0;
            for (int g = 0; g < 8; ++g) {
                int sum4 = 0;
                for (int e = 0; e < 4; ++e) sum4 += (int) wq[256 * b + 32 * g + 4 * l + e] * (int) xq[256 * b + 32 * g + 4 * l + e];
                sumi += wa_qk_scale_of(type, wsc + 16 * b, 32 * g + 4 * l) * sum4;
            }
            if (variant == 1) { const float p = dd * (float) sumi; acc[l] = acc[l] + p; }
            else acc[l] = fmaf(dd, (float) sumi, acc[l]);
        }
    }
    if (variant == 2) { float v = acc[0]; for (int l = 1; l < 8; ++l) v = v + acc[l]; return type == WA_TYPE_Q5_K ? v + summs : v; }
    if (variant == 4 && type == WA_TYPE_Q5_K) return (((acc[0] + acc[4]) + (acc[2] + acc[6])) + summs) + ((acc[1] + acc[5]) + (acc[3] + acc[7]));
    const float v = wa_qk_hsum8(acc);
    return type == WA_TYPE_Q5_K ? v + summs : v;
}

// element order <-> kernel layout of one row's quants
static void kq_to_layout(const int8_t * q, size_t row, size_t nb, int8_t * qs) {
    for (size_t b = 0; b < nb; ++b) for (int e = 0; e < 256; ++e) qs[wa_qk_quant_index(row, nb, b, e)] = q[256 * b + e];
}
static void kq_from_layout(const int8_t * qs, size_t row, size_t nb, int8_t * q) {
    for (size_t b = 0; b < nb; ++b) for (int e = 0; e < 256; ++e) q[256 * b + e] = qs[wa_qk_quant_index(row, nb, b, e)];
}

extern "C" {

// raw blocks of a [n_rows][K] matrix -> the loader's arrays
void kq_unpack_rows(int type, int n_rows, int K, const uint8_t * blocks, int8_t * qs, int8_t * sc, float * d, float * dmin, int variant) {
    const size_t nb = (size_t) K / 256, bsz = wa_qk_block_bytes(type);
    std::vector<int8_t> q(K);
    for (size_t r = 0; r < (size_t) n_rows; ++r) {
        for (size_t b = 0; b < nb; ++b) {
            float dd, dm;
            kq_unpack_block(type, blocks + (r * nb + b) * bsz, &q[256 * b], sc + (r * nb + b) * 16, dd, dm, variant);
            d[r * nb + b] = dd; dmin[r * nb + b] = dm;
        }
        kq_to_layout(q.data(), r, nb, qs);
    }
}

void kq_q8_K_rows(const float * x, int ldx, int rows, int K, int8_t * qs, float * d, int16_t * bsums, int variant) {
    const size_t nb = (size_t) K / 256;
    std::vector<int8_t> q(K);
    for (size_t r = 0; r < (size_t) rows; ++r) {
        kq_q8_K_row(x + r * ldx, (int) nb, q.data(), d + r * nb, bsums + r * nb * 16, variant);
        kq_to_layout(q.data(), r, nb, qs);
    }
}

// out [M][N] = the raw products (before any epilogue)
void kq_gemm(int type, int M, int N, int K, const int8_t * wqs, const int8_t * wsc, const float * wd, const float * wdmin, const int8_t * xqs,
             const float * xd, const int16_t * xbs, float * out, int variant) {
    const size_t nb = (size_t) K / 256;
    std::vector<int8_t> w(K), xall((size_t) M * K);
    for (size_t m = 0; m < (size_t) M; ++m) kq_from_layout(xqs, m, nb, &xall[m * K]);
    for (size_t n = 0; n < (size_t) N; ++n) {
        kq_from_layout(wqs, n, nb, w.data());
        for (size_t m = 0; m < (size_t) M; ++m)
            out[m * N + n] = kq_dot(type, (int) nb, w.data(), wsc + n * nb * 16, wd + n * nb, wdmin + n * nb, &xall[m * K], xd + m * nb, xbs + m * nb * 16, variant);
    }
}

// rows `tok` of the matrix dequantised, + pe[pos]: out [n][K]
void kq_embed(int type, int n, const int32_t * tok, const int32_t * pos, int K, const int8_t * wqs, const int8_t * wsc, const float * wd, const float * wdmin,
              const float * pe, float * out) {
    const size_t nb = (size_t) K / 256;
    std::vector<int8_t> q(K);
    for (int j = 0; j < n; ++j) {
        const size_t t = (size_t) tok[j];
        kq_from_layout(wqs, t, nb, q.data());
        for (int i = 0; i < K; ++i) {
            const size_t b = (size_t) i >> 8;
            const float v = wa_qk_dequant(type, &q[256 * b], wsc + (t * nb + b) * 16, wd[t * nb + b], wdmin[t * nb + b], i & 255);
            out[(size_t) j * K + i] = v + pe[(size_t) pos[j] * K + i];
        }
    }
}

}

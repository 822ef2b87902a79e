// wa_quant4.h - ggml's Q4_0 and Q4_K as the reference multiplies them, restated in scalar host code.  Host-compilable on its own
// (tests/native/quant4_math.cpp holds it to the reference library bit for bit); the kernels of wa_quant4.hip restate THIS arithmetic.
// Build with -ffp-contract=off: `a * b + c` below is two roundings, fmaf one.
//
//   block_q4_0 { f16 d; u8 qs[16]; }       18 bytes, 32 values: element j < 16 is the low nibble of qs[j], element 16 + j the high one,
//                                          weight = d (q - 8)
//
// The reference (AVX2 build with its CPU repack, ggml-cpu/repack.cpp) keeps a Q4_0 matrix in one of two forms, by how the graph uses it:
//
//   interleaved  every matrix that is only ever a MUL_MAT weight and has a multiple of 8 rows - here all 2-D weights but the token
//                embedding: eight rows side by side (block_q4_0x8), multiplied by ggml_gemv_q4_0_8x8_q8_0 / ggml_gemm_q4_0_8x8_q8_0
//                (arch/x86/repack.cpp).  Each OUTPUT carries ONE chain over the blocks, in block order:
//                    acc = fma((float) isum_b, f32(d_w) * f32(d_x), acc)        isum_b = sum_{e < 32} (q_w[e] - 8) q_x[e], exact
//                There are no lane partial sums and no horizontal sum; gemv and gemm build the same chain, so a value does not depend on
//                the number of activation rows.  The activation rows are Q8_0; ggml_quantize_mat_q8_0_4x8, which quantises groups of four
//                rows, gives the quants and scales of the row quantiser (d = max|x| / 127, id = 127 / max|x|, rint(x id), d through F16).
//   plain        the token embedding (a GET_ROWS weight; n_vocab is no multiple of 8 either), hence the logits product:
//                ggml_vec_dot_q4_0_q8_0 - the eight-lane chains and hsum_float_8 of the Q5_0 product (wa_quant.hip) on the values q - 8 -
//                and dequantize_row_q4_0: (float) (q - 8) * d.
//
// Kernel layouts, made once at load:
//   interleaved  nibble words u32 [row][g = 0..3][block]: byte e of word (g, b) is the file's qs[4 g + e] of block b - low nibble element
//                4 g + e, high nibble element 16 + 4 g + e, both still unsigned (the kernels subtract 8) - so 16 bytes of a (row, g) are
//                four whole blocks' share of lanes g and 4 + g of the activation layout; scales f32 [row][block].  4 + 1 bits per weight.
//   plain        the layout of Q5_0 (wa_quant1.h: signed bytes q - 8 [row][lane l = 0..7][block][4], scales f32 [row][block]); the
//                kernels of wa_quant.hip take it as it is.
//
// Q4_K (second half of this file) follows the same split - interleaved: ggml_gemv_q4_K_8x8_q8_K / ggml_gemm_q4_K_8x8_q8_K, two chains per output; plain:
// ggml_vec_dot_q4_K_q8_K - and adds a second quantiser rule for the Q8_K activation rows; see there.
#pragma once
#include "wa_quant1.h"
#include "wa_quantk.h"

#define WA_TYPE_Q4_0  2        // ggml tensor type, and ftype % 1000 of such a file
#define WA_Q4_0_BYTES 18

// one block on file -> its 32 signed quants q - 8 and its scale
inline void wa_q4_0_unpack(const uint8_t * blk, int8_t q[32], float & d) {
    uint16_t dh; memcpy(&dh, blk, 2);
    d = wa_q1_h2f(dh);
    for (int j = 0; j < 16; ++j) {
        q[j]      = (int8_t) ((int) (blk[2 + j] & 0x0f) - 8);
        q[j + 16] = (int8_t) ((int) (blk[2 + j] >> 4) - 8);
    }
}

// `rows` rows of nb blocks on file -> the interleaved kernel layout.  THE definition of what the model loader writes for such a matrix.
inline void wa_q4_0_pack_rows(const uint8_t * src, size_t rows, size_t nb, uint8_t * qs, float * qd) {
    for (size_t r = 0; r < rows; ++r)
        for (size_t b = 0; b < nb; ++b) {
            const uint8_t * blk = src + (r * nb + b) * WA_Q4_0_BYTES;
            uint16_t dh; memcpy(&dh, blk, 2);
            qd[r * nb + b] = wa_q1_h2f(dh);
            for (int g = 0; g < 4; ++g) memcpy(qs + ((r * 4 + g) * nb + b) * 4, blk + 2 + 4 * g, 4);
        }
}
// element e (0..31) of block b of row r of that layout, as the signed value q - 8
inline int wa_q4_0_packed_at(const uint8_t * qs, size_t r, size_t nb, size_t b, int e) {
    const uint8_t v = qs[((r * 4 + (size_t) ((e & 15) >> 2)) * nb + b) * 4 + (size_t) (e & 3)];
    return (int) (e < 16 ? v & 0x0f : v >> 4) - 8;
}
// the same rows -> the plain kernel layout (the token embedding)
inline void wa_q4_0_plain_rows(const uint8_t * src, size_t rows, size_t nb, int8_t * qs, float * qd) {
    for (size_t r = 0; r < rows; ++r)
        for (size_t b = 0; b < nb; ++b) {
            int8_t v[32];
            wa_q4_0_unpack(src + (r * nb + b) * WA_Q4_0_BYTES, v, qd[r * nb + b]);
            for (int l = 0; l < 8; ++l) memcpy(qs + ((r * 8 + l) * nb + b) * 4, v + 4 * l, 4);
        }
}

// dequantize_row_q4_0
inline float wa_q4_0_dequant(int8_t q, float d) { return (float) q * d; }

// quantize_row_q8_0 / one row of ggml_quantize_mat_q8_0_4x8: quants [block][32] and d [block] as the F32 value of its F16 field
inline void wa_q8_0_row(const float * x, int nb, int8_t * q, float * d) {
    for (int b = 0; b < nb; ++b) {
        float a = 0.0f;
        for (int e = 0; e < 32; ++e) a = fmaxf(a, fabsf(x[32 * b + e]));
        const float df = a / 127.f;
        const float id = a != 0.0f ? 127.f / a : 0.0f;
        for (int e = 0; e < 32; ++e) q[32 * b + e] = (int8_t) (int) rintf(x[32 * b + e] * id);      // to nearest, ties to even
        d[b] = wa_q1_h2f(wa_q1_f2h(df));
    }
}

// one output of the interleaved product: weight row (wq [block][32] signed, wd [block]) x activation row (xq [block][32], xd [block])
inline float wa_q4_0_dot8(int nb, const int8_t * wq, const float * wd, const int8_t * xq, const float * xd) {
    float acc = 0.0f;
    for (int b = 0; b < nb; ++b) {
        int isum = 0;
        for (int e = 0; e < 32; ++e) isum += (int) wq[32 * b + e] * (int) xq[32 * b + e];
        const float p = wd[b] * xd[b];
        acc = fmaf((float) isum, p, acc);
    }
    return acc;
}
// one output of the plain product (ggml_vec_dot_q4_0_q8_0)
inline float wa_q4_0_dot_plain(int nb, const int8_t * wq, const float * wd, const int8_t * xq, const float * xd) {
    float acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int b = 0; b < nb; ++b) {
        const float dd = wd[b] * xd[b];
        for (int l = 0; l < 8; ++l) {
            int sum4 = 0;
            for (int e = 0; e < 4; ++e) sum4 += (int) wq[32 * b + 4 * l + e] * (int) xq[32 * b + 4 * l + e];
            acc[l] = fmaf(dd, (float) sum4, acc[l]);
        }
    }
    return wa_q1_hsum8(acc);
}

// =====================================================================================================================================
// Q4_K
//   block_q4_K { f16 d; f16 dmin; u8 scales[12]; u8 qs[128]; }      144 bytes, 256 values in 8 sub-blocks of 32
//       weight e of sub-block s = (d sc[s]) q - (dmin m[s]),  q unsigned 0..15, sc / m unsigned 6-bit (get_scale_min_k4)
//       sub-block s, element i: nibble (s & 1) of qs[32 (s / 2) + i]
//
//   interleaved  per output TWO chains, in block order (Q8_K activation rows: d_x f32, 16-element sums bsums):
//                    acc    = fma((float) sum_s sc[s] isum_s,                          f32(d_w)    * d_x, acc)      isum_s: the sub-block's exact dot product
//                    accmin = fma((float) sum_s m[s] (bsums[2 s] + bsums[2 s + 1]),    f32(dmin_w) * d_x, accmin)
//                    out    = acc - accmin
//                the inner sums exact in int32 and converted to F32 once (to nearest even: the first can pass 2^24).  How far the inner sums
//                run depends on the row's PLACE in the product of M rows: rows below M - M % 4 (M > 3) are multiplied by ggml_gemm_q4_K_8x8_q8_K,
//                which takes a chain step per PAIR of sub-blocks (s = 2 j, 2 j + 1: four steps per block, the same scale product each); the
//                leftover rows, and every row of a product of up to three, by ggml_gemv_q4_K_8x8_q8_K: one step per block, s = 0..7.
//                The ACTIVATION ROWS depend on it too: the product of M rows quantises rows below M - M % 4 in groups of four by
//                ggml_quantize_mat_q8_K_4x8 and the leftover rows by quantize_row_q8_K_ref (wa_q8_K_row).  The four-row form takes
//                iscale = -127 / max|x| when ANY element equals + max|x|, else + 127 / max|x| - the row form takes the sign of the FIRST element
//                of largest magnitude; a block that holds - m before + m gets opposite signs of d and of every quant - and saturates to
//                [-128, 127] in its packs where the row form clamps with min(127, .).  d = 1 / iscale and the sums are formed alike.
//   plain        ggml_vec_dot_q4_K_q8_K: the eight-lane chains of the Q5_K product, acc[l] = fma(d_x f32(d_w), (float) sumi[l], acc[l]), and FOUR minimum
//                chains  acc_m[k] = fma(-d_x f32(dmin_w), (float) (m[2 k] s[2 k] + m[2 k + 1] s[2 k + 1]), acc_m[k]),  s[j] = bsums[2 j] + bsums[2 j + 1];
//                out = hsum_float_8(acc) + ((acc_m[0] + acc_m[2]) + (acc_m[1] + acc_m[3])).  dequantize_row_q4_K is Q5_K's: (d sc) q - (dmin m).
//
// Kernel layouts:
//   interleaved  nibble words u32 [row][l = 0..7][block][j = 0..3]: byte e of word (l, b, j) is the file's qs[32 j + 4 l + e] of block b - low nibble element
//                4 l + e of sub-block 2 j, high nibble the same element of sub-block 2 j + 1: the share of activation lane l, 16 bytes per block;
//                scale bytes u8 [row][block][16] (sc[0..7], then m[0..7], expanded once); d, dmin f32 [row][block].
//   plain        the arrays of Q5_K (wa_quantk.h: wa_qk_unpack_rows) with quants 0..15; the embedding fetch is Q5_K's kernel.
#define WA_TYPE_Q4_K  12
#define WA_Q4_K_BYTES 144

// one block on file -> q[256] 0..15 in element order, sc[16] (scales, then minimums), d, dmin
inline void wa_q4_K_unpack(const uint8_t * blk, int8_t q[256], uint8_t sc[16], float & d, float & dmin) {
    uint16_t h;
    memcpy(&h, blk, 2); d = wa_q1_h2f(h); memcpy(&h, blk + 2, 2); dmin = wa_q1_h2f(h);
    const uint8_t * s = blk + 4, * qs = blk + 16;
    for (int b = 0; b < 8; ++b) {
        for (int i = 0; i < 32; ++i) q[32 * b + i] = (int8_t) ((b & 1) ? qs[32 * (b >> 1) + i] >> 4 : qs[32 * (b >> 1) + i] & 0xf);
        if (b < 4) { sc[b] = s[b] & 63; sc[8 + b] = s[b + 4] & 63; }                                       // get_scale_min_k4
        else       { sc[b] = (uint8_t) ((s[b + 4] & 0xf) | ((s[b - 4] >> 6) << 4)); sc[8 + b] = (uint8_t) ((s[b + 4] >> 4) | ((s[b] >> 6) << 4)); }
    }
}
// `rows` rows of nb blocks on file -> the interleaved kernel layout.  THE definition of what the model loader writes for such a matrix.
inline void wa_q4_K_pack_rows(const uint8_t * src, size_t rows, size_t nb, uint8_t * qs, uint8_t * qsc, float * qd, float * qm) {
    for (size_t r = 0; r < rows; ++r)
        for (size_t b = 0; b < nb; ++b) {
            const uint8_t * blk = src + (r * nb + b) * WA_Q4_K_BYTES;
            int8_t v[256];
            wa_q4_K_unpack(blk, v, qsc + (r * nb + b) * 16, qd[r * nb + b], qm[r * nb + b]);
            for (int l = 0; l < 8; ++l)
                for (int j = 0; j < 4; ++j) memcpy(qs + (((r * 8 + l) * nb + b) * 4 + j) * 4, blk + 16 + 32 * j + 4 * l, 4);
        }
}
// element e (0..255) of block b of row r of that layout
inline int wa_q4_K_packed_at(const uint8_t * qs, size_t r, size_t nb, size_t b, int e) {
    const int s = e >> 5, i = e & 31;
    const uint8_t v = qs[(((r * 8 + (size_t) (i >> 2)) * nb + b) * 4 + (size_t) (s >> 1)) * 4 + (size_t) (i & 3)];
    return (s & 1) ? v >> 4 : v & 0x0f;
}
// the same rows -> the plain kernel layout: Q5_K's arrays (the token embedding)
inline void wa_q4_K_plain_rows(const uint8_t * src, size_t rows, size_t nb, int8_t * qs, int8_t * qsc, float * qd, float * qm) {
    for (size_t r = 0; r < rows; ++r)
        for (size_t b = 0; b < nb; ++b) {
            int8_t v[256];
            wa_q4_K_unpack(src + (r * nb + b) * WA_Q4_K_BYTES, v, (uint8_t *) qsc + (r * nb + b) * 16, qd[r * nb + b], qm[r * nb + b]);
            for (int g = 0; g < 8; ++g)
                for (int l = 0; l < 8; ++l) memcpy(qs + wa_qk_quant_index(r, nb, b, 32 * g + 4 * l), v + 32 * g + 4 * l, 4);
        }
}

// one row of ggml_quantize_mat_q8_K_4x8 (rows below M - M % 4 of an interleaved product; the leftover rows take wa_q8_K_row)
inline void wa_q8_K_row4(const float * x, int nb, int8_t * q, float * d, int16_t * bsums) {
    for (int b = 0; b < nb; ++b, x += 256, q += 256, bsums += 16) {
        float amax = 0.0f;
        for (int j = 0; j < 256; ++j) amax = fmaxf(amax, fabsf(x[j]));
        if (!(amax != 0.0f)) { d[b] = 0.0f; memset(q, 0, 256); memset(bsums, 0, 32); continue; }
        bool pos = false;
        for (int j = 0; j < 256; ++j) pos = pos || x[j] == amax;
        const float iscale = pos ? -127.f / amax : 127.f / amax;
        for (int j = 0; j < 256; ++j) {
            const int v = (int) rintf(x[j] * iscale);
            q[j] = (int8_t) (v < -128 ? -128 : v > 127 ? 127 : v);
        }
        for (int j = 0; j < 16; ++j) { int s = 0; for (int i = 0; i < 16; ++i) s += q[16 * j + i]; bsums[j] = (int16_t) s; }
        d[b] = 1.0f / iscale;
    }
}

// the rows of a product of M that take the four-row quantiser and the gemm's chain steps: those below this
inline int wa_q4_K_rows4(int M) { return M > 3 ? M - M % 4 : 0; }

// one output of the interleaved product: weight row (wq [block][256] 0..15, wsc [block][16], wd, wdm [block]) x activation row.  gemm: the row lies
// below wa_q4_K_rows4(M) - a chain step per pair of sub-blocks; else one per block.
inline float wa_q4_K_dot8(int nb, const int8_t * wq, const uint8_t * wsc, const float * wd, const float * wdm, const int8_t * xq, const float * xd,
                          const int16_t * xbs, bool gemm) {
    float acc = 0.0f, accmin = 0.0f;
    for (int b = 0; b < nb; ++b) {
        const float p = wd[b] * xd[b], pm = wdm[b] * xd[b];
        int isum = 0, imin = 0;
        for (int s = 0; s < 8; ++s) {
            int t = 0;
            for (int e = 0; e < 32; ++e) t += (int) wq[256 * b + 32 * s + e] * (int) xq[256 * b + 32 * s + e];
            isum += (int) wsc[16 * b + s] * t;
            imin += (int) wsc[16 * b + 8 + s] * ((int) xbs[16 * b + 2 * s] + (int) xbs[16 * b + 2 * s + 1]);
            if ((gemm && (s & 1)) || s == 7) {
                acc = fmaf((float) isum, p, acc);
                accmin = fmaf((float) imin, pm, accmin);
                isum = imin = 0;
            }
        }
    }
    return acc - accmin;
}
// one output of the plain product (ggml_vec_dot_q4_K_q8_K)
inline float wa_q4_K_dot_plain(int nb, const int8_t * wq, const uint8_t * wsc, const float * wd, const float * wdm, const int8_t * xq, const float * xd,
                               const int16_t * xbs) {
    float acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, am[4] = { 0, 0, 0, 0 };
    for (int b = 0; b < nb; ++b) {
        const float dd = xd[b] * wd[b], dm = -xd[b] * wdm[b];
        for (int k = 0; k < 4; ++k) {
            int s = 0;
            for (int u = 2 * k; u < 2 * k + 2; ++u) s += (int) wsc[16 * b + 8 + u] * ((int) xbs[16 * b + 2 * u] + (int) xbs[16 * b + 2 * u + 1]);
            am[k] = fmaf(dm, (float) s, am[k]);
        }
        for (int l = 0; l < 8; ++l) {
            int sumi = 0;
            for (int g = 0; g < 8; ++g) {
                int sum4 = 0;
                for (int e = 0; e < 4; ++e) sum4 += (int) wq[256 * b + 32 * g + 4 * l + e] * (int) xq[256 * b + 32 * g + 4 * l + e];
                sumi += (int) wsc[16 * b + g] * sum4;
            }
            acc[l] = fmaf(dd, (float) sumi, acc[l]);
        }
    }
    const float m = (am[0] + am[2]) + (am[1] + am[3]);
    return wa_qk_hsum8(acc) + m;
}

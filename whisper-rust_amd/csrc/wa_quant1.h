// wa_quant1.h - the ggml block formats with a per-block minimum (Q4_1, Q5_1) and the Q8_1 activation row they are multiplied
// with, restated in scalar host code: the block unpack the loader runs, and one output of the reference's AVX2 product
// (quantize_row_q8_1, ggml_vec_dot_q4_1_q8_1 / q5_1_q8_1, ggml-cpu/arch/x86/quants.c; dequantize_row_q4_1 / q5_1, ggml-quants.c).
// Host-compilable on its own (tests/native/quant1_math.cpp holds it to the reference library bit for bit); the kernels of
// wa_quant.hip restate THIS arithmetic.  Build with -ffp-contract=off: `a * b + c` below is two roundings, fmaf one.
//
//   block_q4_1 { f16 d; f16 m; u8 qs[16]; }            20 bytes      weight e = q[e] * d + m,  q unsigned 0..15
//   block_q5_1 { f16 d; f16 m; u32 qh; u8 qs[16]; }    24 bytes                                q unsigned 0..31
//   element j < 16: low nibble of qs[j], element j + 16: high nibble, bit j / j + 16 of qh: the fifth bit
//   block_q8_1 { f16 d; f16 s; i8 qs[32]; }            d = max|x| / 127, q = rint(x * (127 / max|x|)), s = f16(d_f32 * sum q)
//
//   out = hsum_float_8(acc) + summs,   acc[l] = fma(f32(d_w) * f32(d_x), (float) sum_{e<4} q_w[4l+e] q_x[4l+e], acc[l])   l = 0..7
//                                      summs  = summs + (f32(m_w) * f32(s_x))      (a multiplication, then an addition), block after block
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#define WA_Q4_1_BYTES 20
#define WA_Q5_1_BYTES 24

// IEEE half <-> float in integer arithmetic (any host compiler): exact widening; narrowing to nearest even, infinity beyond the
// range (65520 and up), subnormals kept, NaN stays NaN - what vcvtps2ph / v_cvt_f16_f32 store.
inline float wa_q1_h2f(uint16_t h) {
    const uint32_t sign = (uint32_t) (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    uint32_t u;
    if (e == 31u) u = sign | 0x7f800000u | (m << 13);
    else if (e != 0u) u = sign | ((e + 112u) << 23) | (m << 13);
    else if (m == 0u) u = sign;
    else { float f = (float) m * 0x1p-24f; memcpy(&u, &f, 4); u |= sign; }
    float r; memcpy(&r, &u, 4); return r;
}
inline uint16_t wa_q1_f2h(float f) {
    uint32_t u; memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t) ((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t) (sign | 0x7e00u | ((u >> 13) & 0x3ffu));       // NaN (quiet)
    if (u >= 0x477ff000u) return (uint16_t) (sign | 0x7c00u);                              // >= 65520: infinity
    if (u < 0x38800000u) {                                                                 // below 2^-14: a subnormal half (or zero)
        float a; memcpy(&a, &u, 4);
        const float r = a + 0.5f;             // one rounding, to nearest even, at the spacing 2^-24 of the subnormal halfs
        uint32_t v; memcpy(&v, &r, 4);
        return (uint16_t) (sign | (v - 0x3f000000u));
    }
    const uint32_t v = u + 0xfffu + ((u >> 13) & 1u);                                      // to nearest, ties to even, at bit 13
    return (uint16_t) (sign | ((v - 0x38000000u) >> 13));
}

// ggml tensor type 3 (Q4_1) or 7 (Q5_1): bytes of one 32-element block, 0 for any other type
inline size_t wa_q1_block_bytes(int type) { return type == 3 ? WA_Q4_1_BYTES : type == 7 ? WA_Q5_1_BYTES : 0; }

// one block on file -> its 32 unsigned quants (as signed bytes: 0..31 fits), scale and minimum
inline void wa_q1_unpack(int type, const uint8_t * blk, int8_t q[32], float & d, float & m) {
    uint16_t dh, mh; memcpy(&dh, blk, 2); memcpy(&mh, blk + 2, 2);
    d = wa_q1_h2f(dh); m = wa_q1_h2f(mh);
    uint32_t qh = 0;
    const uint8_t * qs = blk + 4;
    if (type == 7) { memcpy(&qh, blk + 4, 4); qs = blk + 8; }
    for (int j = 0; j < 16; ++j) {
        q[j]      = (int8_t) ((qs[j] & 0x0f) | (((qh >> j) & 1u) << 4));
        q[j + 16] = (int8_t) ((qs[j] >> 4)   | (((qh >> (j + 16)) & 1u) << 4));
    }
}

// The two formats without a minimum, block_q5_0 { f16 d; u32 qh; u8 qs[16]; } (22 bytes, ggml type 6) and block_q8_0 { f16 d; i8 qs[32]; }
// (34 bytes, type 8; ggml-common.h:187-214): one block on file -> its 32 signed quants and scale.  Q5_0: element j < 16 is the low nibble
// of qs[j], j + 16 the high nibble, bit e of qh the fifth bit, and the value is that minus 16.
inline size_t wa_q0_block_bytes(int type) { return type == 6 ? 22 : type == 8 ? 34 : 0; }
inline void wa_q0_unpack(int type, const uint8_t * blk, int8_t q[32], float & d) {
    uint16_t dh; memcpy(&dh, blk, 2);
    d = wa_q1_h2f(dh);
    if (type == 6) {
        uint32_t qh; memcpy(&qh, blk + 2, 4);
        for (int j = 0; j < 16; ++j) {
            q[j]      = (int8_t) ((int) ((blk[6 + j] & 0x0f) | (((qh >> j) & 1u) << 4)) - 16);
            q[j + 16] = (int8_t) ((int) ((blk[6 + j] >> 4)   | (((qh >> (j + 16)) & 1u) << 4)) - 16);
        }
    } else memcpy(q, blk + 2, 32);
}

// `rows` rows of nb blocks of a 32-value format (type 6, 8, 3 or 7) on file -> the kernel layout the model loader writes: quants
// [row][lane l = 0..7][block][4] (element 4 l + e of block b), scales [row][block] and - Q4_1 / Q5_1 only, else qm is null - minimums
// [row][block].  THE definition of that layout: the host load path runs it, and the device unpack kernels (wa_load.hip) are held to it.
inline void wa_q32_unpack_rows(int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, float * qd, float * qm) {
    const size_t bsz = wa_q0_block_bytes(type) ? wa_q0_block_bytes(type) : wa_q1_block_bytes(type);
    for (size_t r = 0; r < rows; ++r)
        for (size_t b = 0; b < nb; ++b) {
            const uint8_t * blk = src + (r * nb + b) * bsz;
            int8_t v[32];
            if (qm) wa_q1_unpack(type, blk, v, qd[r * nb + b], qm[r * nb + b]);
            else wa_q0_unpack(type, blk, v, qd[r * nb + b]);
            for (int l = 0; l < 8; ++l) memcpy(qs + ((r * 8 + l) * nb + b) * 4, v + 4 * l, 4);
        }
}

// dequantize_row_q4_1 / q5_1: q * d, then + m
inline float wa_q1_dequant(int8_t q, float d, float m) { const float t = (float) q * d; return t + m; }

// quantize_row_q8_1 of n = 32 nb values: quants [block][32], d [block] and s [block], both as the F32 value of their F16 field
inline void wa_q8_1_row(const float * x, int nb, int8_t * q, float * d, float * s) {
    for (int b = 0; b < nb; ++b) {
        float a = 0.0f;
        for (int e = 0; e < 32; ++e) a = fmaxf(a, fabsf(x[32 * b + e]));
        const float df = a / 127.f;
        const float id = a != 0.0f ? 127.f / a : 0.0f;
        int sum = 0;
        for (int e = 0; e < 32; ++e) {
            const int v = (int) rintf(x[32 * b + e] * id);        // to nearest, ties to even
            q[32 * b + e] = (int8_t) v;
            sum += v;
        }
        d[b] = wa_q1_h2f(wa_q1_f2h(df));
        s[b] = wa_q1_h2f(wa_q1_f2h(df * (float) sum));             // the UNROUNDED d times the exact integer sum, one rounding to F32, one to F16
    }
}

// hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
inline float wa_q1_hsum8(const float a[8]) { return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7])); }

// one output: weight row (unpacked: wq [block][32], wd, wm [block]) x activation row (xq [block][32], xd, xs [block])
inline float wa_q1_dot(int nb, const int8_t * wq, const float * wd, const float * wm, const int8_t * xq, const float * xd, const float * xs) {
    float acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    float summs = 0.0f;
    for (int b = 0; b < nb; ++b) {
        const float p = wm[b] * xs[b];
        summs = summs + p;
        const float dd = wd[b] * xd[b];
        for (int l = 0; l < 8; ++l) {
            int sum4 = 0;
            for (int e = 0; e < 4; ++e) sum4 += (int) wq[32 * b + 4 * l + e] * (int) xq[32 * b + 4 * l + e];
            acc[l] = fmaf(dd, (float) sum4, acc[l]);
        }
    }
    return wa_q1_hsum8(acc) + summs;
}

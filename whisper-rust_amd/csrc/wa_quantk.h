// wa_quantk.h - the ggml K formats the reference multiplies without its CPU repack (Q2_K, Q3_K, Q5_K, Q6_K) and the Q8_K activation row
// they are multiplied with, restated in scalar host code: the block unpack the loader runs, the dequantisation of a row (token embedding),
// the Q8_K row, and one output of the reference's AVX2 product (quantize_row_q8_K_ref, dequantize_row_q2_K / q3_K / q5_K / q6_K,
// ggml-quants.c; ggml_vec_dot_q2_K_q8_K / q3_K_q8_K / q5_K_q8_K / q6_K_q8_K, ggml-cpu/arch/x86/quants.c).  Host-compilable on its own (tests/native/kquant_math.cpp holds it
// to the reference library bit for bit); the kernels of wa_quantk.hip restate THIS arithmetic.  Build with -ffp-contract=off:
// `a * b + c` below is two roundings, fmaf one.
//
//   block_q5_K { f16 d; f16 dmin; u8 scales[12]; u8 qh[32]; u8 qs[128]; }   176 bytes, 256 values in 8 sub-blocks of 32
//       weight e of sub-block b = (d sc[b]) q - (dmin m[b]),  q unsigned 0..31, sc / m unsigned 6-bit (get_scale_min_k4)
//       sub-block b, element i: nibble (b & 1) of qs[32 (b / 2) + i], fifth bit = bit b of qh[i]
//   block_q6_K { u8 ql[128]; u8 qh[64]; i8 scales[16]; f16 d; }             210 bytes, 256 values in 16 sub-blocks of 16
//       weight e = d sc[e / 16] (q - 32),  q unsigned 0..63; per 128-value half (ql + 64 h, qh + 32 h), l = 0..31:
//       e = l: low nibble of ql[l], qh bits 0-1 | e = 32 + l: low nibble of ql[32 + l], bits 2-3 |
//       e = 64 + l: high nibble of ql[l], bits 4-5 | e = 96 + l: high nibble of ql[32 + l], bits 6-7      (of qh[l])
//   block_q3_K { u8 hmask[32]; u8 qs[64]; u8 scales[12]; f16 d; }           110 bytes, 256 values in 16 sub-blocks of 16
//       weight e = d sc[e / 16] q,  q signed -4..3, sc signed -32..31: once unpacked, Q6_K's arithmetic with nothing added
//       e = 128 n + 32 j + l (l < 32): q = ((qs[32 n + l] >> 2 j) & 3) - (bit 4 n + j of hmask[l] set ? 0 : 4)
//       sc[k] = (low nibble of scales[k], k < 8, else high nibble of scales[k - 8]) | ((scales[8 + (k & 3)] >> 2 (k >> 2)) & 3) << 4, minus 32
//   block_q2_K { u8 scales[16]; u8 qs[64]; f16 d; f16 dmin; }               84 bytes, 256 values in 16 sub-blocks of 16
//       weight e = (d sc[e / 16]) q - (dmin m[e / 16]),  q unsigned 0..3 = (qs[32 n + l] >> 2 j) & 3 as above,
//       sc[s] = scales[s] & 15, m[s] = scales[s] >> 4
//   block_q8_K { f32 d; i8 qs[256]; i16 bsums[16]; }
//       max = the signed value of the FIRST element whose |x| is strictly larger than every earlier |x|; iscale = -127 / max;
//       q = min(127, nearest_int(iscale x)); d = 1 / iscale; bsums[j] = sum of q[16 j .. 16 j + 15]; max 0: d = 0, quants 0
//
//   out = hsum_float_8(acc) [+ summs],  per 256-value block:  acc[l] = fma(d_x f32(d_w), (float) sumi[l], acc[l])   l = 0..7
//       sumi[l] = sum over the eight 32-element groups g of  sc(g, l) * sum_{e<4} q_w[32 g + 4 l + e] q_x[32 g + 4 l + e]    (exact integers)
//       sc(g, l): Q5_K sc[g];  Q6_K, Q3_K and Q2_K scales[2 g + (l >= 4)]
//       Q5_K only: summs = summs + ((-d_x f32(dmin_w)) * (float) sum_b m[b] (bsums[2 b] + bsums[2 b + 1]))   a multiplication, then an addition
//       Q2_K only: the minimums enter the LANE accumulators, per block BEFORE the product term, each by an fma:
//           acc[l] = fma(-d_x f32(dmin_w), (float) (m[2 l] bsums[2 l] + m[2 l + 1] bsums[2 l + 1]), acc[l]),  then the fma of the first line
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#define WA_QK_K       256
#define WA_Q5_K_BYTES 176
#define WA_Q6_K_BYTES 210
#define WA_Q2_K_BYTES 84
#define WA_Q3_K_BYTES 110
#define WA_TYPE_Q2_K  10       // ggml tensor types (and ftype % 1000 of such a file)
#define WA_TYPE_Q3_K  11
#define WA_TYPE_Q5_K  13
#define WA_TYPE_Q6_K  14

inline float wa_qk_h2f(uint16_t h) {        // IEEE half -> float in integer arithmetic: exact
    const uint32_t sign = (uint32_t) (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    uint32_t u;
    if (e == 31u) u = sign | 0x7f800000u | (m << 13);
    else if (e != 0u) u = sign | ((e + 112u) << 23) | (m << 13);
    else if (m == 0u) u = sign;
    else { float f = (float) m * 0x1p-24f; memcpy(&u, &f, 4); u |= sign; }
    float r; memcpy(&r, &u, 4); return r;
}

inline size_t wa_qk_block_bytes(int type) {
    return type == WA_TYPE_Q5_K ? WA_Q5_K_BYTES : type == WA_TYPE_Q6_K ? WA_Q6_K_BYTES : type == WA_TYPE_Q2_K ? WA_Q2_K_BYTES : type == WA_TYPE_Q3_K ? WA_Q3_K_BYTES : 0;
}
inline bool wa_wtype_is_k(int type) { return type == WA_TYPE_Q5_K || type == WA_TYPE_Q6_K || type == WA_TYPE_Q2_K || type == WA_TYPE_Q3_K; }
inline bool wa_qk_has_min(int type) { return type == WA_TYPE_Q5_K || type == WA_TYPE_Q2_K; }        // the formats with a dmin array

// One 256-value block on file -> the kernel's view of it: q[256] signed bytes in element order (Q6_K: q - 32, Q5_K: 0..31, Q3_K: -4..3,
// Q2_K: 0..3), sc[16] the sub-block scale bytes as the product reads them, d (and dmin, Q5_K and Q2_K only, else 0).
//   Q6_K: sc[8 h + g] = scales[2 g + h]: the scale of elements 16 h .. 16 h + 15 of 32-element group g (lanes 4 h .. 4 h + 3)
//   Q3_K: the same order, the 6-bit scales assembled and minus 32
//   Q2_K: the same order, the file's bytes as they are: scale in the low nibble, minimum in the high one
//   Q5_K: sc[g] = the 6-bit scale of group g, sc[8 + g] = its 6-bit minimum
inline void wa_qk_unpack(int type, const uint8_t * blk, int8_t q[256], int8_t sc[16], float & d, float & dmin) {
    uint16_t h;
    if (type == WA_TYPE_Q6_K) {
        const uint8_t * ql = blk, * qh = blk + 128; const int8_t * s = (const int8_t *) blk + 192;
        memcpy(&h, blk + 208, 2); d = wa_qk_h2f(h); dmin = 0.0f;
        for (int hf = 0; hf < 2; ++hf, ql += 64, qh += 32)
            for (int l = 0; l < 32; ++l) {
                q[128 * hf + l]      = (int8_t) ((int) ((ql[l]      & 0xf) | (((qh[l] >> 0) & 3) << 4)) - 32);
                q[128 * hf + 32 + l] = (int8_t) ((int) ((ql[32 + l] & 0xf) | (((qh[l] >> 2) & 3) << 4)) - 32);
                q[128 * hf + 64 + l] = (int8_t) ((int) ((ql[l]      >> 4)  | (((qh[l] >> 4) & 3) << 4)) - 32);
                q[128 * hf + 96 + l] = (int8_t) ((int) ((ql[32 + l] >> 4)  | (((qh[l] >> 6) & 3) << 4)) - 32);
            }
        for (int g = 0; g < 8; ++g) { sc[g] = s[2 * g]; sc[8 + g] = s[2 * g + 1]; }
    } else if (type == WA_TYPE_Q3_K) {
        const uint8_t * hm = blk, * qs = blk + 32, * s = blk + 96;
        memcpy(&h, blk + 108, 2); d = wa_qk_h2f(h); dmin = 0.0f;
        for (int n = 0; n < 2; ++n)
            for (int j = 0; j < 4; ++j)
                for (int l = 0; l < 32; ++l)
                    q[128 * n + 32 * j + l] = (int8_t) ((int) ((qs[32 * n + l] >> (2 * j)) & 3) - (((hm[l] >> (4 * n + j)) & 1) ? 0 : 4));
        for (int k = 0; k < 16; ++k) {
            const int lo = k < 8 ? s[k] & 0xf : s[k - 8] >> 4, hi = (s[8 + (k & 3)] >> (2 * (k >> 2))) & 3;
            sc[8 * (k & 1) + (k >> 1)] = (int8_t) ((lo | (hi << 4)) - 32);
        }
    } else if (type == WA_TYPE_Q2_K) {
        const uint8_t * s = blk, * qs = blk + 16;
        memcpy(&h, blk + 80, 2); d = wa_qk_h2f(h); memcpy(&h, blk + 82, 2); dmin = wa_qk_h2f(h);
        for (int n = 0; n < 2; ++n)
            for (int j = 0; j < 4; ++j)
                for (int l = 0; l < 32; ++l) q[128 * n + 32 * j + l] = (int8_t) ((qs[32 * n + l] >> (2 * j)) & 3);
        for (int g = 0; g < 8; ++g) { sc[g] = (int8_t) s[2 * g]; sc[8 + g] = (int8_t) s[2 * g + 1]; }
    } else {
        const uint8_t * s = blk + 4, * qh = blk + 16, * qs = blk + 48;
        memcpy(&h, blk, 2); d = wa_qk_h2f(h); memcpy(&h, blk + 2, 2); dmin = wa_qk_h2f(h);
        for (int b = 0; b < 8; ++b) {
            for (int i = 0; i < 32; ++i) {
                const int nib = (b & 1) ? qs[32 * (b >> 1) + i] >> 4 : qs[32 * (b >> 1) + i] & 0xf;
                q[32 * b + i] = (int8_t) (nib | (((qh[i] >> b) & 1) << 4));
            }
            if (b < 4) { sc[b] = (int8_t) (s[b] & 63); sc[8 + b] = (int8_t) (s[b + 4] & 63); }                  // get_scale_min_k4
            else       { sc[b] = (int8_t) ((s[b + 4] & 0xf) | ((s[b - 4] >> 6) << 4)); sc[8 + b] = (int8_t) ((s[b + 4] >> 4) | ((s[b] >> 6) << 4)); }
        }
    }
}
// the scale of element e (0..255) of an unpacked block, and (Q5_K, Q2_K) the minimum of its sub-block
inline int wa_qk_scale_of(int type, const int8_t sc[16], int e) {
    if (type == WA_TYPE_Q5_K) return sc[e >> 5];
    const int s = sc[8 * ((e >> 4) & 1) + (e >> 5)];
    return type == WA_TYPE_Q2_K ? s & 15 : s;
}
inline int wa_qk_min_of(int type, const int8_t sc[16], int e) {
    return type == WA_TYPE_Q5_K ? sc[8 + (e >> 5)] : type == WA_TYPE_Q2_K ? (uint8_t) sc[8 * ((e >> 4) & 1) + (e >> 5)] >> 4 : 0;
}

// dequantize_row_q6_K / q3_K: (d * sc) * q - two multiplications; dequantize_row_q5_K / q2_K: (d * sc) * q, then - (dmin * m) - no fma anywhere
inline float wa_qk_dequant(int type, const int8_t q[256], const int8_t sc[16], float d, float dmin, int e) {
    const float d1 = d * (float) wa_qk_scale_of(type, sc, e);
    const float t = d1 * (float) q[e];
    if (!wa_qk_has_min(type)) return t;
    const float m1 = dmin * (float) wa_qk_min_of(type, sc, e);
    return t - m1;
}

// quantize_row_q8_K_ref of n = 256 nb values: quants [block][256], d [block], bsums [block][16].  (The reference leaves the bsums of
// an all-zero block unwritten; they are multiplied by d = 0 only.  Here they are 0.)
inline void wa_q8_K_row(const float * x, int nb, int8_t * q, float * d, int16_t * bsums) {
    for (int b = 0; b < nb; ++b, x += 256, q += 256, bsums += 16) {
        float max = 0.0f, amax = 0.0f;
        for (int j = 0; j < 256; ++j) { const float ax = fabsf(x[j]); if (ax > amax) { amax = ax; max = x[j]; } }
        if (!(amax != 0.0f)) { d[b] = 0.0f; memset(q, 0, 256); memset(bsums, 0, 32); continue; }
        const float iscale = -127.f / max;
        for (int j = 0; j < 256; ++j) {
            const float p = iscale * x[j];
            const int v = (int) rintf(p);                  // nearest_int: to nearest, ties to even
            q[j] = (int8_t) (v < 127 ? v : 127);
        }
        for (int j = 0; j < 16; ++j) { int s = 0; for (int i = 0; i < 16; ++i) s += q[16 * j + i]; bsums[j] = (int16_t) s; }
        d[b] = 1.0f / iscale;
    }
}

// hsum_float_8: ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7))
inline float wa_qk_hsum8(const float a[8]) { return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7])); }

// one output: weight row (unpacked: wq [block][256], wsc [block][16], wd, wdmin [block]) x activation row (xq [block][256], xd [block],
// xbs [block][16])
inline float wa_qk_dot(int type, int nb, const int8_t * wq, const int8_t * wsc, const float * wd, const float * wdmin, const int8_t * xq,
                       const float * xd, const int16_t * xbs) {
    float acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    float summs = 0.0f;
    for (int b = 0; b < nb; ++b) {
        const float dd = xd[b] * wd[b];
        if (type == WA_TYPE_Q5_K) {
            const float dm = -xd[b] * wdmin[b];
            int s = 0;
            for (int g = 0; g < 8; ++g) s += (int) wsc[16 * b + 8 + g] * ((int) xbs[16 * b + 2 * g] + (int) xbs[16 * b + 2 * g + 1]);
            const float p = dm * (float) s;
            summs = summs + p;
        }
        if (type == WA_TYPE_Q2_K) {        // the minimums of sub-blocks 2 l, 2 l + 1 into lane l, before the product term
            const float dn = -xd[b] * wdmin[b];
            for (int l = 0; l < 8; ++l) {
                const int s = wa_qk_min_of(type, wsc + 16 * b, 32 * l) * (int) xbs[16 * b + 2 * l] + wa_qk_min_of(type, wsc + 16 * b, 32 * l + 16) * (int) xbs[16 * b + 2 * l + 1];
                acc[l] = fmaf(dn, (float) s, acc[l]);
            }
        }
        for (int l = 0; l < 8; ++l) {
            int sumi = 0;
            for (int g = 0; g < 8; ++g) {
                int sum4 = 0;
                for (int e = 0; e < 4; ++e) sum4 += (int) wq[256 * b + 32 * g + 4 * l + e] * (int) xq[256 * b + 32 * g + 4 * l + e];
                sumi += wa_qk_scale_of(type, wsc + 16 * b, 32 * g + 4 * l) * sum4;
            }
            acc[l] = fmaf(dd, (float) sumi, acc[l]);
        }
    }
    const float v = wa_qk_hsum8(acc);
    return type == WA_TYPE_Q5_K ? v + summs : v;
}

// ---- kernel layout (made once at load; the Q8_K quantiser writes activation rows into the same quant order) ----
//   quants  int8 [row][lane l = 0..7][block][group g = 0..7][4]: element 32 g + 4 l + e of a block - a lane's 32 bytes per block are contiguous
//   scales  int8 [row][block][16] as wa_qk_unpack orders them;  d (and dmin) f32 [row][block];  activation sums int16 [row][block][16]
inline size_t wa_qk_quant_index(size_t row, size_t nb, size_t b, int e) {
    return ((row * 8 + (size_t) ((e & 31) >> 2)) * nb + b) * 32 + (size_t) (e >> 5) * 4 + (size_t) (e & 3);
}

// `rows` rows of nb blocks of a K format on file -> the kernel layout above: quants, scale bytes, d and - Q5_K / Q2_K only, else qm is null -
// dmin.  THE definition of what the model loader writes: the host load path runs it, and the device unpack kernels (wa_load.hip) are held to it.
inline void wa_qk_unpack_rows(int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, int8_t * qsc, float * qd, float * qm) {
    const size_t bsz = wa_qk_block_bytes(type);
    for (size_t r = 0; r < rows; ++r)
        for (size_t b = 0; b < nb; ++b) {
            int8_t v[256]; float dd, dm;
            wa_qk_unpack(type, src + (r * nb + b) * bsz, v, qsc + (r * nb + b) * 16, dd, dm);
            qd[r * nb + b] = dd;
            if (qm) qm[r * nb + b] = dm;
            for (int g = 0; g < 8; ++g)
                for (int l = 0; l < 8; ++l) memcpy(qs + wa_qk_quant_index(r, nb, b, 32 * g + 4 * l), v + 32 * g + 4 * l, 4);
        }
}

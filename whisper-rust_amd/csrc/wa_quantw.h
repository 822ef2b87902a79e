// wa_quantw.h - F32 / F16 values -> ggml weight blocks, restated in scalar host code from the behaviour of the reference's
// quantize_row_q{4_0,4_1,5_0,5_1,8_0}_ref and quantize_row_q{4,5,6}_K_ref with their helpers nearest_int, make_qkx2_quants and make_qx_quants
// (rmse_type 1, no weights) - ggml-quants.c, which is built as ISO C: no contraction, no fast-math.  Host-compilable on its own
// (tests/native/quantw_math.cpp holds it to ggml_quantize_chunk of the reference library byte for byte); it is the host path of
// whisper_amd_quantize_rows (where = 0), and the kernels of wa_quantw.hip restate THIS arithmetic.  Build with -ffp-contract=off.
//
// What makes the bytes come out:
//   * every F32 operation is one rounding of its own: `a * b + c` is a multiplication and an addition, (w * x) * l and (w * l) * l associate to the left;
//   * every sum runs in element order, one chain per sum;
//   * divisions and sqrtf are correctly rounded, F32 -> F16 rounds to nearest even (wa_q1_f2h);
//   * the 32-value formats take the FIRST element of largest magnitude (strict >), and the first smallest / largest element of Q4_1 / Q5_1
//     (which decides the sign of a zero minimum or scale);
//   * (int8_t)(v + 8.5f) truncates towards zero, then MIN(15, .); a v outside the int range (a subnormal scale's reciprocal is infinite)
//     converts as x86 does, to INT_MIN, whose low byte is 0 (wa_qw_trunc).
//
// The two searches, and why neither has a closed form:
//   * make_qkx2_quants (Q4_K, Q5_K) walks is = 0..nstep.  An accepted candidate (mad < best_mad, strict) replaces not only scale and best_mad
//     but `min` itself, and every LATER candidate's grid - iscale = (rmin + rdelta is + nmax) / (max - min) and l = nearest_int(iscale (x - min)) -
//     is built on that new min.  So "the lowest is whose mad equals the minimum over all candidates" holds only between two acceptances:
//     PROOF for one stretch: with min fixed, the candidates is0..nstep are independent of one another; the walk accepts the first one below
//     best_mad, nothing before it changes any state, so the state after it is a function of (min, best_mad, is) alone.  The whole walk is
//     therefore "repeat: evaluate every remaining candidate on the current min, accept the LOWEST is with mad < best_mad, continue behind it" -
//     which is what the kernel does with its candidates spread over lanes (a round per acceptance, at most nstep + 1 rounds).
//   * make_qx_quants (Q6_K): the candidates is = -9..9 are independent (iscale = -(32 + 0.1 is) / max), but the acceptance test
//     sumlx^2 > best suml2 moves `best` with every accepted candidate: the ordered replay over the candidates' (sumlx, suml2) is needed.
#pragma once
#include "wa_quant1.h"

#define WA_QW_GROUP_MAX_EPS 1e-15f
// the three scalar helpers are shared with the kernels (no HIP include: the attributes exist only where hipcc compiles this file)
#ifdef __HIPCC__
#define WA_QW_HD __host__ __device__
#else
#define WA_QW_HD
#endif

// values and bytes of one block of ggml type 2 Q4_0 / 3 Q4_1 / 6 Q5_0 / 7 Q5_1 / 8 Q8_0 / 12 Q4_K / 13 Q5_K / 14 Q6_K; 0 for every other type
WA_QW_HD inline int wa_qw_block_values(int type) { return type == 2 || type == 3 || type == 6 || type == 7 || type == 8 ? 32 : type >= 12 && type <= 14 ? 256 : 0; }
WA_QW_HD inline size_t wa_qw_block_bytes(int type) {
    return type == 2 ? 18 : type == 3 ? 20 : type == 6 ? 22 : type == 7 ? 24 : type == 8 ? 34 : type == 12 ? 144 : type == 13 ? 176 : type == 14 ? 210 : 0;
}

WA_QW_HD inline bool wa_qw_finite(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return (u & 0x7f800000u) != 0x7f800000u; }
// float -> int as cvttss2si: towards zero, INT_MIN when out of range or NaN
WA_QW_HD inline int wa_qw_trunc(float v) { return v > -2147483648.0f && v < 2147483648.0f ? (int) v : (int) 0x80000000u; }
WA_QW_HD inline int wa_qw_nearest_int(float v) {
    const float t = v + 12582912.f;
    int32_t i; __builtin_memcpy(&i, &t, 4);
    return (i & 0x007fffff) - 0x00400000;
}
inline void wa_qw_put16(uint8_t * p, uint16_t h) { memcpy(p, &h, 2); }

// ---- 32-value formats --------------------------------------------------------------------------------------------------------------
inline void wa_qw_block32(int type, const float * x, uint8_t * y) {
    if (type == 8) {
        float amax = 0.0f;
        for (int j = 0; j < 32; ++j) { const float a = fabsf(x[j]); amax = amax > a ? amax : a; }
        const float d = amax / 127, id = d ? 1.0f / d : 0.0f;
        wa_qw_put16(y, wa_q1_f2h(d));
        for (int j = 0; j < 32; ++j) y[2 + j] = (uint8_t) (int8_t) wa_qw_trunc(roundf(x[j] * id));
        return;
    }
    if (type == 2 || type == 6) {
        const int half = type == 2 ? 8 : 16, top = 2 * half - 1;
        float amax = 0.0f, max = 0.0f;
        for (int j = 0; j < 32; ++j) if (amax < fabsf(x[j])) { amax = fabsf(x[j]); max = x[j]; }
        const float d = max / (float) -half, id = d ? 1.0f / d : 0.0f, off = (float) half + 0.5f;
        wa_qw_put16(y, wa_q1_f2h(d));
        uint8_t * qs = y + (type == 2 ? 2 : 6);
        uint32_t qh = 0;
        for (int j = 0; j < 16; ++j) {
            const int a = (int8_t) wa_qw_trunc(x[j] * id + off), b = (int8_t) wa_qw_trunc(x[16 + j] * id + off);
            const uint8_t q0 = (uint8_t) (a < top ? a : top), q1 = (uint8_t) (b < top ? b : top);
            qs[j] = (uint8_t) ((q0 & 15) | ((q1 & 15) << 4));
            qh |= (uint32_t) ((q0 >> 4) & 1) << j | (uint32_t) ((q1 >> 4) & 1) << (j + 16);
        }
        if (type == 6) memcpy(y + 2, &qh, 4);
        return;
    }
    // Q4_1 / Q5_1
    const int top = type == 3 ? 15 : 31;
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
    for (int j = 0; j < 32; ++j) { if (x[j] < mn) mn = x[j]; if (x[j] > mx) mx = x[j]; }
    const float d = (mx - mn) / (float) top, id = d ? 1.0f / d : 0.0f;
    wa_qw_put16(y, wa_q1_f2h(d)); wa_qw_put16(y + 2, wa_q1_f2h(mn));
    uint8_t * qs = y + (type == 3 ? 4 : 8);
    uint32_t qh = 0;
    for (int j = 0; j < 16; ++j) {
        const int a = wa_qw_trunc((x[j] - mn) * id + 0.5f), b = wa_qw_trunc((x[16 + j] - mn) * id + 0.5f);
        uint8_t q0, q1;
        if (type == 3) { const int a8 = (int8_t) a, b8 = (int8_t) b; q0 = (uint8_t) (a8 < 15 ? a8 : 15); q1 = (uint8_t) (b8 < 15 ? b8 : 15); }
        else { q0 = (uint8_t) a; q1 = (uint8_t) b; }                        // Q5_1 has no clamp: (uint8_t), the low five bits kept
        qs[j] = (uint8_t) ((q0 & 15) | ((q1 & 15) << 4));
        qh |= (uint32_t) ((q0 >> 4) & 1) << j | (uint32_t) ((q1 >> 4) & 1) << (j + 16);
    }
    if (type == 7) memcpy(y + 4, &qh, 4);
}

// ---- make_qkx2_quants, n = 32, squared error ---------------------------------------------------------------------------------------
// One candidate on a given min: the quants (into l[]), the least-squares (scale, min) and its weighted squared error.  False: D <= 0.
inline bool wa_qw_qkx2_candidate(int nmax, const float * x, const float * w, float sum_w, float sum_x, float iscale, float min, uint8_t * l,
                                 float & this_scale, float & this_min, float & mad) {
    float sum_l = 0, sum_l2 = 0, sum_xl = 0;
    for (int i = 0; i < 32; ++i) {
        int q = wa_qw_nearest_int(iscale * (x[i] - min));
        q = q < 0 ? 0 : q > nmax ? nmax : q;
        l[i] = (uint8_t) q;
        const float wl = w[i] * (float) q;
        sum_l += wl; sum_l2 += wl * (float) q; sum_xl += wl * x[i];
    }
    const float D = sum_w * sum_l2 - sum_l * sum_l;
    if (!(D > 0)) return false;
    this_scale = (sum_w * sum_xl - sum_x * sum_l) / D;
    this_min   = (sum_l2 * sum_x - sum_l * sum_xl) / D;
    if (this_min > 0) { this_min = 0; this_scale = sum_xl / sum_l2; }
    mad = 0;
    for (int i = 0; i < 32; ++i) {
        float diff = this_scale * (float) l[i] + this_min - x[i];
        diff = diff * diff;
        mad += w[i] * diff;
    }
    return true;
}
inline float wa_qw_qkx2(int nmax, const float * x, const float * w, uint8_t * L, float * the_min, float rmin, float rdelta, int nstep) {
    float min = x[0], max = x[0], sum_w = w[0], sum_x = sum_w * x[0];
    for (int i = 1; i < 32; ++i) {
        if (x[i] < min) min = x[i];
        if (x[i] > max) max = x[i];
        sum_w += w[i]; sum_x += w[i] * x[i];
    }
    if (min > 0) min = 0;
    if (max == min) { for (int i = 0; i < 32; ++i) L[i] = 0; *the_min = -min; return 0.f; }
    float iscale = (float) nmax / (max - min), scale = 1 / iscale, best_mad = 0;
    for (int i = 0; i < 32; ++i) {
        int q = wa_qw_nearest_int(iscale * (x[i] - min));
        q = q < 0 ? 0 : q > nmax ? nmax : q;
        L[i] = (uint8_t) q;
        float diff = scale * (float) L[i] + min - x[i];
        diff = diff * diff;
        best_mad += w[i] * diff;
    }
    uint8_t aux[32];
    for (int is = 0; is <= nstep; ++is) {
        iscale = (rmin + rdelta * (float) is + (float) nmax) / (max - min);
        float ts, tm, mad;
        if (wa_qw_qkx2_candidate(nmax, x, w, sum_w, sum_x, iscale, min, aux, ts, tm, mad) && mad < best_mad) {
            memcpy(L, aux, 32);
            best_mad = mad; scale = ts; min = tm;
        }
    }
    *the_min = -min;
    return scale;
}

// scales[8], mins[8] -> the 12 scale bytes and d, dmin of a Q4_K / Q5_K block (y: d at 0, dmin at 2, scales at 4); sc[], mn[]: the 6-bit values
inline void wa_qw_k45_scales(const float * scales, const float * mins, uint8_t * y, uint8_t * sc, uint8_t * mn) {
    float max_scale = 0, max_min = 0;
    for (int j = 0; j < 8; ++j) { if (scales[j] > max_scale) max_scale = scales[j]; if (mins[j] > max_min) max_min = mins[j]; }
    const float inv_scale = max_scale > 0 ? 63.f / max_scale : 0.f, inv_min = max_min > 0 ? 63.f / max_min : 0.f;
    uint8_t * s = y + 4;
    memset(s, 0, 12);
    for (int j = 0; j < 8; ++j) {
        uint8_t ls = (uint8_t) wa_qw_nearest_int(inv_scale * scales[j]), lm = (uint8_t) wa_qw_nearest_int(inv_min * mins[j]);
        ls = ls < 63 ? ls : 63; lm = lm < 63 ? lm : 63;
        sc[j] = ls; mn[j] = lm;
        if (j < 4) { s[j] |= ls; s[j + 4] |= lm; }
        else { s[j + 4] = (uint8_t) ((ls & 15) | ((lm & 15) << 4)); s[j - 4] |= (uint8_t) ((ls >> 4) << 6); s[j] |= (uint8_t) ((lm >> 4) << 6); }
    }
    wa_qw_put16(y, wa_q1_f2h(max_scale / 63.f)); wa_qw_put16(y + 2, wa_q1_f2h(max_min / 63.f));
}

inline void wa_qw_block_k45(int type, const float * x, uint8_t * y) {
    const int nmax = type == 12 ? 15 : 31;
    uint8_t L[256], sc[8], mn[8];
    float w[32], scales[8], mins[8];
    for (int j = 0; j < 8; ++j) {
        float sum_x2 = 0;
        for (int l = 0; l < 32; ++l) sum_x2 += x[32 * j + l] * x[32 * j + l];
        const float av_x = sqrtf(sum_x2 / 32);
        for (int l = 0; l < 32; ++l) w[l] = av_x + fabsf(x[32 * j + l]);
        scales[j] = type == 12 ? wa_qw_qkx2(15, x + 32 * j, w, L + 32 * j, &mins[j], -1.f, 0.1f, 20)
                               : wa_qw_qkx2(31, x + 32 * j, w, L + 32 * j, &mins[j], -0.5f, 0.1f, 15);
    }
    wa_qw_k45_scales(scales, mins, y, sc, mn);
    uint16_t dh, mh; memcpy(&dh, y, 2); memcpy(&mh, y + 2, 2);
    for (int j = 0; j < 8; ++j) {
        const float d = wa_q1_h2f(dh) * (float) sc[j];
        if (!d) continue;                                                 // the search's own quants stay
        const float dm = wa_q1_h2f(mh) * (float) mn[j];
        for (int i = 0; i < 32; ++i) {
            const int l = wa_qw_nearest_int((x[32 * j + i] + dm) / d);
            L[32 * j + i] = (uint8_t) (l < 0 ? 0 : l > nmax ? nmax : l);
        }
    }
    if (type == 12) {
        for (int g = 0; g < 4; ++g) for (int l = 0; l < 32; ++l) y[16 + 32 * g + l] = (uint8_t) (L[64 * g + l] | (L[64 * g + 32 + l] << 4));
    } else {
        uint8_t * qh = y + 16, * ql = y + 48;
        memset(qh, 0, 32);
        for (int g = 0; g < 4; ++g) for (int l = 0; l < 32; ++l) {
            const int a = L[64 * g + l], b = L[64 * g + 32 + l];
            qh[l] |= (uint8_t) (((a >> 4) << (2 * g)) | ((b >> 4) << (2 * g + 1)));
            ql[32 * g + l] = (uint8_t) ((a & 15) | ((b & 15) << 4));
        }
    }
}

// ---- make_qx_quants, n = 16, nmax = 32, weights x^2 ---------------------------------------------------------------------------------
// (sumlx, suml2) of one candidate scale
inline void wa_qw_qx_sums(const float * x, float iscale, float & sumlx, float & suml2) {
    sumlx = 0; suml2 = 0;
    for (int i = 0; i < 16; ++i) {
        int l = wa_qw_nearest_int(iscale * x[i]);
        l = l < -32 ? -32 : l > 31 ? 31 : l;
        const float w = x[i] * x[i];
        sumlx += w * x[i] * (float) l;
        suml2 += w * (float) l * (float) l;
    }
}
inline void wa_qw_qx_quants(const float * x, float iscale, int8_t * L) {
    for (int i = 0; i < 16; ++i) { const int l = wa_qw_nearest_int(iscale * x[i]); L[i] = (int8_t) (32 + (l < -32 ? -32 : l > 31 ? 31 : l)); }
}
inline float wa_qw_qx(const float * x, int8_t * L) {
    float max = 0, amax = 0;
    for (int i = 0; i < 16; ++i) { const float ax = fabsf(x[i]); if (ax > amax) { amax = ax; max = x[i]; } }
    if (amax < WA_QW_GROUP_MAX_EPS) { for (int i = 0; i < 16; ++i) L[i] = 0; return 0.f; }
    float iscale = -32.f / max, sumlx, suml2;
    wa_qw_qx_sums(x, iscale, sumlx, suml2);
    wa_qw_qx_quants(x, iscale, L);
    float scale = suml2 ? sumlx / suml2 : 0.0f, best = scale * sumlx;
    for (int is = -9; is <= 9; ++is) {
        if (is == 0) continue;
        iscale = -(32.f + 0.1f * (float) is) / max;
        wa_qw_qx_sums(x, iscale, sumlx, suml2);
        if (suml2 > 0 && sumlx * sumlx > best * suml2) { wa_qw_qx_quants(x, iscale, L); scale = sumlx / suml2; best = scale * sumlx; }
    }
    return scale;
}

inline void wa_qw_block_k6(const float * x, uint8_t * y) {        // ql[128] qh[64] scales[16] d
    int8_t L[256];
    float scales[16], max_scale = 0, max_abs_scale = 0;
    for (int ib = 0; ib < 16; ++ib) {
        scales[ib] = wa_qw_qx(x + 16 * ib, L + 16 * ib);
        const float a = fabsf(scales[ib]);
        if (a > max_abs_scale) { max_abs_scale = a; max_scale = scales[ib]; }
    }
    if (max_abs_scale < WA_QW_GROUP_MAX_EPS) { memset(y, 0, 210); return; }
    const float iscale = -128.f / max_scale;
    const uint16_t dh = wa_q1_f2h(1 / iscale);
    wa_qw_put16(y + 208, dh);
    int8_t * sc = (int8_t *) (y + 192);
    for (int ib = 0; ib < 16; ++ib) { const int s = wa_qw_nearest_int(iscale * scales[ib]); sc[ib] = (int8_t) (s < 127 ? s : 127); }
    for (int j = 0; j < 16; ++j) {
        const float d = wa_q1_h2f(dh) * (float) sc[j];
        if (!d) continue;
        for (int i = 0; i < 16; ++i) { const int l = wa_qw_nearest_int(x[16 * j + i] / d); L[16 * j + i] = (int8_t) (32 + (l < -32 ? -32 : l > 31 ? 31 : l)); }
    }
    for (int h = 0; h < 2; ++h) for (int l = 0; l < 32; ++l) {
        const int a = L[128 * h + l], b = L[128 * h + 32 + l], c = L[128 * h + 64 + l], e = L[128 * h + 96 + l];
        y[64 * h + l] = (uint8_t) ((a & 15) | ((c & 15) << 4));
        y[64 * h + 32 + l] = (uint8_t) ((b & 15) | ((e & 15) << 4));
        y[128 + 32 * h + l] = (uint8_t) ((a >> 4) | ((b >> 4) << 2) | ((c >> 4) << 4) | ((e >> 4) << 6));
    }
}

// n values (a multiple of the type's block) -> n / block blocks at dst.  0, 1: not a type this file quantises, 2: n is no multiple of the
// block, 3: a value that is not finite (dst is then left partly written).
inline int wa_quantw_rows(int type, const float * x, int64_t n, void * dst) {
    const int bv = wa_qw_block_values(type);
    if (!bv) return 1;
    if (n < 0 || n % bv != 0) return 2;
    for (int64_t i = 0; i < n; ++i) if (!wa_qw_finite(x[i])) return 3;
    const size_t bs = wa_qw_block_bytes(type);
    uint8_t * y = (uint8_t *) dst;
    for (int64_t b = 0; b < n / bv; ++b, x += bv, y += bs) {
        if (bv == 32) wa_qw_block32(type, x, y);
        else if (type == 14) wa_qw_block_k6(x, y);
        else wa_qw_block_k45(type, x, y);
    }
    return 0;
}
// the same from F16 values: the exact widening first, a run at a time
inline int wa_quantw_rows_f16(int type, const uint16_t * h, int64_t n, void * dst) {
    const int bv = wa_qw_block_values(type);
    if (!bv) return 1;
    if (n < 0 || n % bv != 0) return 2;
    float x[256];
    uint8_t * y = (uint8_t *) dst;
    for (int64_t b = 0; b < n / bv; ++b, y += wa_qw_block_bytes(type)) {
        for (int i = 0; i < bv; ++i) x[i] = wa_q1_h2f(h[b * bv + i]);
        const int rc = wa_quantw_rows(type, x, bv, y);
        if (rc) return rc;
    }
    return 0;
}

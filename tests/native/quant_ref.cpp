// quant_ref.cpp - TEST INFRASTRUCTURE ONLY: the host reference of the kernels of wa_quant.hip, as C entry points for
// tools/quant_cases.py (tests/test_quant_kernels_gpu.py, tests/test_quant_kernels_math.py).  Variant 0 of every function IS the
// arithmetic of whisper-rust_amd/csrc/wa_quant1.h (wa_q8_1_row, wa_q1_dot, wa_q1_dequant), plus the Q5_0 / Q8_0 product, which has no
// minimum and is stated here in the same style; tests/native/quant_ref_pin.cpp holds variant 0 to the reference library bit for bit.
// Variants 1.. are deliberate WRONG restatements: the CPU test asks that each of them changes an expected output of every group of
// cases, i.e. that a kernel which computed that instead would be caught.  All operands are plain [block][32] arrays.
// Build: g++ -O2 -fPIC -std=c++17 -ffp-contract=off, no -mfma (`a * b + c` is two roundings, fmaf one).
#include "wa_quant1.h"

#define QR_API extern "C" __attribute__((visibility("default")))

// ---- the product ---------------------------------------------------------------------------------
enum { QR_DOT_REF = 0, QR_DOT_HSUM_LINEAR = 1, QR_DOT_MUL_ADD = 2, QR_DOT_MIN_FMA = 3, QR_DOT_MIN_SKIP0 = 4, QR_DOT_VARIANTS = 5 };

static inline float qr_hsum8(const float a[8], int variant) {
    if (variant == QR_DOT_HSUM_LINEAR) return ((((((a[0] + a[1]) + a[2]) + a[3]) + a[4]) + a[5]) + a[6]) + a[7];
    return wa_q1_hsum8(a);
}

static inline void qr_lane_chains(int nb, const int8_t * wq, const float * wd, const int8_t * xq, const float * xd, int variant, float acc[8]) {
    for (int l = 0; l < 8; ++l) acc[l] = 0.0f;
    for (int b = 0; b < nb; ++b) {
        const float dd = wd[b] * xd[b];
        for (int l = 0; l < 8; ++l) {
            int sum4 = 0;
            for (int e = 0; e < 4; ++e) sum4 += (int) wq[32 * b + 4 * l + e] * (int) xq[32 * b + 4 * l + e];
            if (variant == QR_DOT_MUL_ADD) { const float p = dd * (float) sum4; acc[l] = acc[l] + p; }
            else acc[l] = fmaf(dd, (float) sum4, acc[l]);
        }
    }
}

// ggml_vec_dot_q5_0_q8_0 / ggml_vec_dot_q8_0_q8_0 (AVX2): the lane chains and hsum_float_8, nothing else - no minimum chain and no
// final addition, so a -0 sum stays -0
static inline float qr_dot_q0(int nb, const int8_t * wq, const float * wd, const int8_t * xq, const float * xd, int variant) {
    float acc[8];
    qr_lane_chains(nb, wq, wd, xq, xd, variant, acc);
    return qr_hsum8(acc, variant);
}

static inline float qr_dot_q1(int nb, const int8_t * wq, const float * wd, const float * wm, const int8_t * xq, const float * xd, const float * xs,
                              int variant) {
    if (variant == QR_DOT_REF) return wa_q1_dot(nb, wq, wd, wm, xq, xd, xs);
    float acc[8];
    qr_lane_chains(nb, wq, wd, xq, xd, variant, acc);
    float summs = 0.0f;
    for (int b = variant == QR_DOT_MIN_SKIP0 ? 1 : 0; b < nb; ++b) {
        if (variant == QR_DOT_MIN_FMA) summs = fmaf(wm[b], xs[b], summs);
        else { const float p = wm[b] * xs[b]; summs = summs + p; }
    }
    return qr_hsum8(acc, variant) + summs;
}

// out [M][N] = x . w^T; wm == nullptr: the Q5_0 / Q8_0 product, else Q4_1 / Q5_1 (xs must be set).  Returns 0, or -1 for an unknown variant.
QR_API int qref_gemm(int variant, int M, int N, int nb, const int8_t * wq, const float * wd, const float * wm, const int8_t * xq, const float * xd,
                     const float * xs, float * out) {
    if (variant < 0 || variant >= QR_DOT_VARIANTS || (!wm && variant > QR_DOT_MUL_ADD) || (wm && !xs)) return -1;
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            const int8_t * w = wq + (size_t) n * nb * 32, * x = xq + (size_t) m * nb * 32;
            out[(size_t) m * N + n] = wm ? qr_dot_q1(nb, w, wd + (size_t) n * nb, wm + (size_t) n * nb, x, xd + (size_t) m * nb, xs + (size_t) m * nb, variant)
                                         : qr_dot_q0(nb, w, wd + (size_t) n * nb, x, xd + (size_t) m * nb, variant);
        }
    return 0;
}

// ---- the quantiser -------------------------------------------------------------------------------
enum { QR_Q_REF = 0, QR_Q_TIES_AWAY = 1, QR_Q_ID_FROM_D = 2, QR_Q_S_ROUNDED_D = 3, QR_Q_S_FLOAT_SUM = 4, QR_Q_VARIANTS = 5 };

static inline void qr_q8_1_row(const float * x, int nb, int8_t * q, float * d, float * s, int variant) {
    if (variant == QR_Q_REF) { wa_q8_1_row(x, nb, q, d, s); return; }
    for (int b = 0; b < nb; ++b) {
        float a = 0.0f;
        for (int e = 0; e < 32; ++e) a = fmaxf(a, fabsf(x[32 * b + e]));
        const float df = a / 127.f;
        const float dh = wa_q1_h2f(wa_q1_f2h(df));
        const float id = a != 0.0f ? (variant == QR_Q_ID_FROM_D ? 1.0f / df : 127.f / a) : 0.0f;
        int sum = 0;
        float fsum = 0.0f;
        for (int e = 0; e < 32; ++e) {
            const float t = x[32 * b + e] * id;
            const int v = (int) (variant == QR_Q_TIES_AWAY ? roundf(t) : rintf(t));
            q[32 * b + e] = (int8_t) v;
            sum += v;
            const float p = df * (float) (int8_t) v;
            fsum = fsum + p;
        }
        d[b] = dh;
        s[b] = wa_q1_h2f(wa_q1_f2h(variant == QR_Q_S_ROUNDED_D ? dh * (float) sum : variant == QR_Q_S_FLOAT_SUM ? fsum : df * (float) sum));
    }
}

// quantize_row_q8_1 of `rows` rows of 32 nb values (row r at x + r * ldx); q [rows][nb][32], d / s [rows][nb].  The Q8_0 quantiser is
// the same function with s ignored.
QR_API int qref_quantize(int variant, const float * x, int ldx, int rows, int nb, int8_t * q, float * d, float * s) {
    if (variant < 0 || variant >= QR_Q_VARIANTS) return -1;
    for (int r = 0; r < rows; ++r) qr_q8_1_row(x + (size_t) r * ldx, nb, q + (size_t) r * nb * 32, d + (size_t) r * nb, s + (size_t) r * nb, variant);
    return 0;
}

// dequantize_row_q4_1 / q5_1 (m set: q * d, then + m) or q5_0 / q8_0 (m == nullptr: q * d) of n values, each with its own d (and m)
QR_API void qref_dequant(int n, const int8_t * q, const float * d, const float * m, float * out) {
    for (int i = 0; i < n; ++i) out[i] = m ? wa_q1_dequant(q[i], d[i], m[i]) : (float) q[i] * d[i];
}

QR_API float qref_h2f(uint16_t h) { return wa_q1_h2f(h); }
QR_API uint16_t qref_f2h(float f) { return wa_q1_f2h(f); }

// wa_libm.h - glibc 2.35's tanhf and expf restated, for the host and for the device.
//
// The VAD recurrence (wa_vad_host.cpp) calls libm's expf and tanhf, as the reference does; k_vad_lstm (wa_vad_lstm.hip) runs the same recurrence
// on the device and has to give the same bits.  The functions below follow the algorithms of that libm:
//   tanhf   sysdeps/ieee754/flt-32/s_tanhf.c, the fdlibm form: +-1 beyond 22, x (1 + x) below 2^-55, through expm1f(+-2|x|) in between;
//   expm1f  sysdeps/ieee754/flt-32/s_expm1f.c, fdlibm too: ln2 reduction in two parts, a degree-5 rational in x^2/2, the scaling by cases of k.
//           Plain F32 operations in source order (the x86-64 build of it has no FMA);
//   expf    sysdeps/ieee754/flt-32/e_expf.c in its FMA variant (what the ifunc picks on every AVX2 + FMA host): F64 throughout, a 32-entry
//           table of 2^(i/32), a cubic with written fused multiply-adds.  Whole F32 range: +inf above log(2^128), 0 below log(2^-150), the
//           smallest subnormal between that and log(2^-149), subnormal results rounded once by the F64 -> F32 conversion.
// Nothing here contracts: the project builds with -ffp-contract=off, a fused multiply-add is one only where fma() is written.  The device build
// must keep F32 subnormals (hipcc's -fno-gpu-flush-denormals-to-zero, the rule of wa_vad_lstm.hip's object in the Makefile).
// wa_libm_matches_host() is the guard a VAD context runs when it is created: where this process's libm is another one (no FMA unit, another
// glibc), the context keeps the host recurrence, which is right by construction.
// Compiles with g++ alone (tests/native/vad_libm_math.cpp) and under hipcc for both sides.
#pragma once

#include <cstdint>
#include <cstring>

#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define WA_LIBM_HD __host__ __device__ __forceinline__
#else
#define WA_LIBM_HD static inline
#endif

WA_LIBM_HD uint32_t wa_libm_bits(float f)    { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
WA_LIBM_HD float    wa_libm_float(uint32_t u) { float f;    __builtin_memcpy(&f, &u, 4); return f; }

// 2^(i/32) as F64 bit patterns with i << 47 taken off the exponent field (e_exp2f_data.c's table for N = 32)
#define WA_LIBM_EXP2F_TABLE { \
    0x3ff0000000000000ULL, 0x3fefd9b0d3158574ULL, 0x3fefb5586cf9890fULL, 0x3fef9301d0125b51ULL, 0x3fef72b83c7d517bULL, 0x3fef54873168b9aaULL, \
    0x3fef387a6e756238ULL, 0x3fef1e9df51fdee1ULL, 0x3fef06fe0a31b715ULL, 0x3feef1a7373aa9cbULL, 0x3feedea64c123422ULL, 0x3feece086061892dULL, \
    0x3feebfdad5362a27ULL, 0x3feeb42b569d4f82ULL, 0x3feeab07dd485429ULL, 0x3feea47eb03a5585ULL, 0x3feea09e667f3bcdULL, 0x3fee9f75e8ec5f74ULL, \
    0x3feea11473eb0187ULL, 0x3feea589994cce13ULL, 0x3feeace5422aa0dbULL, 0x3feeb737b0cdc5e5ULL, 0x3feec49182a3f090ULL, 0x3feed503b23e255dULL, \
    0x3feee89f995ad3adULL, 0x3feeff76f2fb5e47ULL, 0x3fef199bdd85529cULL, 0x3fef3720dcef9069ULL, 0x3fef5818dcfba487ULL, 0x3fef7c97337b9b5fULL, \
    0x3fefa4afa2a490daULL, 0x3fefd0765b6e4540ULL }

// branch edges of expf, as F32 bit patterns: |x| = 88 (the range check), log(2^128), log(2^-150), log(2^-149)
#define WA_LIBM_EXPF_88      0x42b00000u
#define WA_LIBM_EXPF_OFLOW   0x42b17217u     //  0x1.62e42ep6
#define WA_LIBM_EXPF_UFLOW   0xc2cff1b4u     // -0x1.9fe368p6
#define WA_LIBM_EXPF_MAYUF   0xc2ce8ecfu     // -0x1.9d1d9ep6

// expf over the whole F32 range; `tab` is WA_LIBM_EXP2F_TABLE wherever the caller keeps it (the kernel: LDS, its index depends on x)
WA_LIBM_HD float wa_expf_full(float x, const unsigned long long * tab) {
    const uint32_t ux = wa_libm_bits(x), ax = ux & 0x7fffffffu;
    if (ax >= WA_LIBM_EXPF_88) {
        if (ux == 0xff800000u) return 0.0f;
        if (ax >= 0x7f800000u) return x + x;
        if (x > wa_libm_float(WA_LIBM_EXPF_OFLOW)) return wa_libm_float(0x7f800000u);
        if (x < wa_libm_float(WA_LIBM_EXPF_UFLOW)) return 0.0f;
        if (x < wa_libm_float(WA_LIBM_EXPF_MAYUF)) return wa_libm_float(1u);       // 0x1.4p-75 squared, rounded: the smallest subnormal
    }
    const double InvLn2N = 0x1.71547652b82fep+0 * 32;
    const double C0 = 0x1.c6af84b912394p-5 / 32 / 32 / 32, C1 = 0x1.ebfce50fac4f3p-3 / 32 / 32, C2 = 0x1.62e42ff0c52d6p-1 / 32;
    const double SHIFT = 0x1.8p+52;
    double z = InvLn2N * (double) x;
    double kd = z + SHIFT;
    unsigned long long ki; __builtin_memcpy(&ki, &kd, 8);
    kd = kd - SHIFT;
    const double r = __builtin_fma(InvLn2N, (double) x, -kd);             // the FMA build contracts z - kd, z being a product: the exact residual
    const unsigned long long t = tab[ki & 31] + (ki << 47);
    double s; __builtin_memcpy(&s, &t, 8);
    z = __builtin_fma(C0, r, C1);
    const double r2 = r * r;
    double y = __builtin_fma(C2, r, 1.0);
    y = __builtin_fma(z, r2, y);
    y = y * s;
    return (float) y;
}

// branch edges of expm1f on |x|: 27 ln2, the overflow threshold, ln2/2, 3 ln2/2, 2^-25
#define WA_LIBM_EXPM1_27LN2  0x4195b844u
#define WA_LIBM_EXPM1_OFLOW  0x42b17218u
#define WA_LIBM_EXPM1_HALF   0x3eb17218u
#define WA_LIBM_EXPM1_3HALF  0x3f851592u
#define WA_LIBM_EXPM1_TINY   0x33000000u

WA_LIBM_HD float wa_expm1f_libm(float x) {
    const float ln2_hi = wa_libm_float(0x3f317180u), ln2_lo = wa_libm_float(0x3717f7d1u), invln2 = wa_libm_float(0x3fb8aa3bu);
    const float Q1 = wa_libm_float(0xbd088889u), Q2 = wa_libm_float(0x3ad00d01u), Q3 = wa_libm_float(0xb8a670cdu),
                Q4 = wa_libm_float(0x36867e54u), Q5 = wa_libm_float(0xb457edbbu);
    const uint32_t ux = wa_libm_bits(x), hx = ux & 0x7fffffffu;
    const bool neg = (ux >> 31) != 0;
    if (hx >= WA_LIBM_EXPM1_27LN2) {
        if (hx >= WA_LIBM_EXPM1_OFLOW) {
            if (hx > 0x7f800000u) return x + x;
            if (hx == 0x7f800000u) return neg ? -1.0f : x;
            if (!neg) return wa_libm_float(0x7f800000u);                  // x above the threshold 0x42b17180 (hx >= ..7218 implies it)
        }
        if (neg) return -1.0f;
    }
    float hi, lo, c = 0.0f, t;
    int k = 0;
    if (hx > WA_LIBM_EXPM1_HALF) {
        if (hx < WA_LIBM_EXPM1_3HALF) {
            if (!neg) { hi = x - ln2_hi; lo = ln2_lo; k = 1; }
            else      { hi = x + ln2_hi; lo = -ln2_lo; k = -1; }
        } else {
            k = (int) (invln2 * x + (neg ? -0.5f : 0.5f));
            t = (float) k;
            hi = x - t * ln2_hi;
            lo = t * ln2_lo;
        }
        x = hi - lo;
        c = (hi - x) - lo;
    } else if (hx < WA_LIBM_EXPM1_TINY) {
        return x;
    }
    const float hfx = 0.5f * x;
    const float hxs = x * hfx;
    const float r1 = 1.0f + hxs * (Q1 + hxs * (Q2 + hxs * (Q3 + hxs * (Q4 + hxs * Q5))));
    t = 3.0f - r1 * hfx;
    float e = hxs * ((r1 - t) / (6.0f - x * t));
    if (k == 0) return x - (x * e - hxs);
    e = x * (e - c) - c;
    e -= hxs;
    if (k == -1) return 0.5f * (x - e) - 0.5f;
    if (k == 1) {
        if (x < -0.25f) return -2.0f * (e - (x + 0.5f));
        return 1.0f + 2.0f * (x - e);
    }
    float y;
    if (k <= -2 || k > 56) {
        y = 1.0f - (e - x);
        y = wa_libm_float(wa_libm_bits(y) + ((uint32_t) k << 23));
        return y - 1.0f;
    }
    if (k < 23) {
        t = wa_libm_float(0x3f800000u - (0x1000000u >> k));               // 1 - 2^-k
        y = t - (e - x);
    } else {
        t = wa_libm_float((uint32_t) (0x7f - k) << 23);                   // 2^-k
        y = x - (e + t);
        y += 1.0f;
    }
    return wa_libm_float(wa_libm_bits(y) + ((uint32_t) k << 23));
}

// branch edges of tanhf on |x|: 22, 1, 2^-55
#define WA_LIBM_TANH_BIG     0x41b00000u
#define WA_LIBM_TANH_ONE     0x3f800000u
#define WA_LIBM_TANH_TINY    0x24000000u

WA_LIBM_HD float wa_tanhf_libm(float x) {
    const uint32_t ux = wa_libm_bits(x), ix = ux & 0x7fffffffu;
    const bool neg = (ux >> 31) != 0;
    if (ix >= 0x7f800000u) return neg ? 1.0f / x - 1.0f : 1.0f / x + 1.0f;
    float z;
    if (ix < WA_LIBM_TANH_BIG) {
        if (ix == 0) return x;
        if (ix < WA_LIBM_TANH_TINY) return x * (1.0f + x);
        const float ax = wa_libm_float(ix);
        if (ix >= WA_LIBM_TANH_ONE) {
            const float t = wa_expm1f_libm(2.0f * ax);
            z = 1.0f - 2.0f / (t + 2.0f);
        } else {
            const float t = wa_expm1f_libm(-2.0f * ax);
            z = -t / (t + 2.0f);
        }
    } else z = 1.0f;
    return neg ? -z : z;
}

// sigmoid as the reference's unary op states it
WA_LIBM_HD float wa_sigmoidf_libm(float x, const unsigned long long * tab) { return 1.f / (1.f + wa_expf_full(-x, tab)); }

// -------------------------------------------------------------------------------------------------
// the load-time guard (host functions): a fixed probe set of about 64 K arguments
// -------------------------------------------------------------------------------------------------

// every branch edge of the three functions above, as |x| bit patterns; the probe set holds each with both signs, +-1 ulp
static const uint32_t WA_LIBM_EDGES[] = {
    WA_LIBM_EXPF_88, WA_LIBM_EXPF_OFLOW, WA_LIBM_EXPF_UFLOW & 0x7fffffffu, WA_LIBM_EXPF_MAYUF & 0x7fffffffu,
    WA_LIBM_EXPM1_27LN2, WA_LIBM_EXPM1_OFLOW, WA_LIBM_EXPM1_HALF, WA_LIBM_EXPM1_3HALF, WA_LIBM_EXPM1_TINY,
    WA_LIBM_EXPM1_27LN2 - 0x00800000u, WA_LIBM_EXPM1_HALF - 0x00800000u, WA_LIBM_EXPM1_3HALF - 0x00800000u,    // the same on 2|x|: tanhf's argument
    WA_LIBM_TANH_BIG, WA_LIBM_TANH_ONE, WA_LIBM_TANH_TINY,
    0x00000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0x7f800000u,
};
static const int WA_LIBM_N_EDGES = (int) (sizeof(WA_LIBM_EDGES) / sizeof(WA_LIBM_EDGES[0]));

// F32 bit patterns: edges +-1 ulp with both signs; 96 arguments in every binade 2^-60 .. 2^7 with both signs; a fixed-seed scatter over |x| < 128
static inline std::vector<uint32_t> wa_libm_probe_set() {
    std::vector<uint32_t> p;
    p.reserve(66000);
    for (int i = 0; i < WA_LIBM_N_EDGES; ++i)
        for (int d = -1; d <= 1; ++d) {
            const uint32_t a = WA_LIBM_EDGES[i] + (uint32_t) d;
            if (WA_LIBM_EDGES[i] == 0 && d < 0) continue;
            if (a > 0x7f800000u) continue;
            p.push_back(a); p.push_back(a | 0x80000000u);
        }
    uint32_t lcg = 0x9e3779b9u;
    for (uint32_t e = 127 - 60; e <= 127 + 6; ++e)
        for (int i = 0; i < 96; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            const uint32_t a = (e << 23) | (i < 32 ? (uint32_t) i * 0x00040000u : (lcg >> 9));
            p.push_back(a); p.push_back(a | 0x80000000u);
        }
    while (p.size() < 65536) {
        lcg = lcg * 1664525u + 1013904223u;
        const uint32_t a = lcg & 0x7fffffffu;
        if (a < 0x43000000u) p.push_back((lcg & 0x80000000u) | a);       // |x| < 128: the top bit of an LCG is its best one
    }
    return p;
}

// true where this process's expf and tanhf are the functions above on the whole probe set
static inline bool wa_libm_matches_host(uint32_t * first_bad = nullptr) {
    static const unsigned long long tab[32] = WA_LIBM_EXP2F_TABLE;
    for (uint32_t u : wa_libm_probe_set()) {
        const float x = wa_libm_float(u);
        float (* volatile host_tanhf)(float) = tanhf;                    // volatile: the calls stay calls of libm, not folded or vectorised
        float (* volatile host_expf)(float) = expf;
        const float a = host_tanhf(x), b = wa_tanhf_libm(x), c = host_expf(x), d = wa_expf_full(x, tab);
        const bool same = (wa_libm_bits(a) == wa_libm_bits(b) || (a != a && b != b)) && (wa_libm_bits(c) == wa_libm_bits(d) || (c != c && d != d));
        if (!same) { if (first_bad) *first_bad = u; return false; }
    }
    return true;
}

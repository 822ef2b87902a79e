// wa_quantk_dev.h - what the K-format kernels of wa_quantk.hip, wa_quantk_rows.hip and wa_quantk_mfma.hip share on the device: the vector types, the weight format of
// an instantiation, how a sub-block scale byte is read, and the order of hsum_float_8 (across the 8 lanes of an output, or inside one lane).
#pragma once
#include "wa_device.h"

typedef int wk_i4 __attribute__((ext_vector_type(4)));
typedef int wk_i2 __attribute__((ext_vector_type(2)));

// hsum_float_8 over the 8 lanes of an output (lane l holds acc[l]; the result is valid in lane 0 of the group)
__device__ __forceinline__ float wk_hsum8(float v) {
    v = v + dpp_f32<0x104>(v);          // row_shl:4  acc[l] + acc[l+4]
    v = v + dpp_f32<0x102>(v);          // row_shl:2  (a0+a4)+(a2+a6) | (a1+a5)+(a3+a7)
    v = v + dpp_f32<0x101>(v);          // row_shl:1  the two halves
    return v;
}
// the same sum where one lane holds all eight accumulators
__device__ __forceinline__ float wk_hsum8_local(const float * a) {
    return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
}
enum { WK_Q6 = 0, WK_Q5 = 1, WK_Q2 = 2 };      // the weight format of an instantiation (Q3_K runs as WK_Q6)
// byte g (0..7) of the scale pair s: signed (Q6_K), unsigned (Q5_K, values <= 63) or its low nibble (Q2_K)
template <int F> __device__ __forceinline__ int wk_byte(wk_i2 s, int g) {
    const int w = g < 4 ? s.x : s.y, sh = 8 * (g & 3);
    return F == WK_Q6 ? (w << (24 - sh)) >> 24 : (int) (((unsigned) w >> sh) & (F == WK_Q2 ? 0xfu : 0xffu));
}
__device__ __forceinline__ float wk_from_lane(float v, int m) {      // lane 0 of an 8-lane group reads lane m's value (m constant after unrolling)
    switch (m) {
        case 1: return dpp_f32<0x101>(v); case 2: return dpp_f32<0x102>(v); case 3: return dpp_f32<0x103>(v); case 4: return dpp_f32<0x104>(v);
        case 5: return dpp_f32<0x105>(v); case 6: return dpp_f32<0x106>(v); case 7: return dpp_f32<0x107>(v); default: return v;
    }
}
// the integer sum of one lane over one 256-value block: 8 groups, quads w0 | w1 against x0 | x1, scale bytes s
template <int F> __device__ __forceinline__ int wk_block(wk_i4 w0, wk_i4 w1, wk_i4 x0, wk_i4 x1, wk_i2 s) {
    int t = 0;
    t += wk_byte<F>(s, 0) * __builtin_amdgcn_sdot4(w0.x, x0.x, 0, false);
    t += wk_byte<F>(s, 1) * __builtin_amdgcn_sdot4(w0.y, x0.y, 0, false);
    t += wk_byte<F>(s, 2) * __builtin_amdgcn_sdot4(w0.z, x0.z, 0, false);
    t += wk_byte<F>(s, 3) * __builtin_amdgcn_sdot4(w0.w, x0.w, 0, false);
    t += wk_byte<F>(s, 4) * __builtin_amdgcn_sdot4(w1.x, x1.x, 0, false);
    t += wk_byte<F>(s, 5) * __builtin_amdgcn_sdot4(w1.y, x1.y, 0, false);
    t += wk_byte<F>(s, 6) * __builtin_amdgcn_sdot4(w1.z, x1.z, 0, false);
    t += wk_byte<F>(s, 7) * __builtin_amdgcn_sdot4(w1.w, x1.w, 0, false);
    return t;
}
